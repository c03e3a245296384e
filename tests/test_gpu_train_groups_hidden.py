"""Training-mode convergence groups of state networks with a hidden layer (csrc/kernels_train_group.hpp, the HID instantiations; opt-in:
`model.native_flags |= nat.FLAG_TRAIN_GROUPS_HIDDEN`): `Loop(training=True, groups=...)`, `LoopTrainer.forward_native(groups=...)` on
composite batches and the grouped serial propagation of `LGNN` / `CompositeLGNN` stacks whose state networks are Dense(H) - Dense(state
width) - against the float64 restatement `oracle.torch_train.lgnn_serial_propagate`, with the bars and conventions of
tests/test_gpu_lgnn_serial.py / test_gpu_lgnn_grouped.py, imported: k exact per graph; states, outputs, relabelled columns and moving
statistics within BAR = 2e-5 of float64 (a graph on which the float32 oracle itself is further away: twice that distance); copied data
bit for bit.  With a threshold > 0 the oracle alone is first held to two preconditions: every float64 k at least MARGIN from flipping,
and more than one distinct k among the graphs (the weight scales below were chosen on the CPU so that both hold).

Every case is built by a `*_case` function that needs no GPU (models, graphs, the oracle's answers, the preconditions): the tests run the
device against it."""
import numpy as np
import pytest
import torch

from gnnkeras_amd import GraphObject
from gnnkeras_amd import _native as nat
from gnnkeras_amd.Models.MLP import MLP, get_inout_dims
from gnnkeras_amd.Models.LGNN import LGNN
from gnnkeras_amd.Models.CompositeLGNN import CompositeLGNN
from gnnkeras_amd.Models.training import LoopTrainer
from gnnkeras_amd.Sequencers.GraphSequencers import CompositeMultiGraphSequencer, MultiGraphSequencer
from oracle import torch_train
from oracle.harness import rel_err, _np, _triple
from test_gpu_training import log_rows
from test_gpu_lgnn_serial import (BAR, MARGIN, CLS, mutag_subsets, _refocused, run_serial_chain, operands, oracle_layer, moving_of,
                                  kernel_name, perturb_bn)
from test_gpu_lgnn_grouped import GROUPED, spy_on_propagate, _single_layer
from test_gpu_composite_grouped import CCLS, DIMS, GROUPED_TYPES, MODE, ONE_RUN, comp_stack, typed_graphs

pytestmark = pytest.mark.gpu
HIDDEN, HIDDEN_TYPES = 'train_step: grouped forward kernels (hidden)', 'train_step: grouped forward kernels (types, hidden)'
FLAG = nat.FLAG_TRAIN_GROUPS_HIDDEN
L, A, T = 14, 3, 2                         # MUTAG: node label columns, arc label columns, classes


def padded(S): return 16 if S <= 16 else 32


# ---- models --------------------------------------------------------------------------------------------------------------------------------
def hidden_layer(focus, d, H, bn, thr, acts=('selu', 'selu'), scale=1.0, layer=0, max_it=5, flag=True, seed=0, get_state=True, get_output=True):
    """One homogeneous layer of the serial stack's shape with state network Dense(H, acts[0]) - Dense(S, acts[1]); `scale` shrinks both
    state kernels (a contracting map: graphs stop before max_iteration); the biases sit off zero (b2 must arrive)."""
    rng = np.random.default_rng(7 + seed)
    inp, lay = get_inout_dims('state', L, A, T, focus, d, hidden_units=[H], layer=layer, get_state=get_state, get_output=get_output)
    ns = MLP(inp[0], lay, list(acts), 'lecun_normal', 'lecun_normal', rng=10 + layer + seed, batch_normalization=bn)
    assert ns.units[0] == H and len(ns.units) == 2
    k0 = 4 if bn else 0
    ns.set_weights([a * scale if a.ndim == 2 else (a + 0.05 if i >= k0 else a) for i, a in enumerate(ns.get_weights())])
    inp, lay = get_inout_dims('output', L, A, T, focus, d, layer=layer, get_state=get_state, get_output=get_output)
    no = MLP(inp[0], lay, 'softmax', 'glorot_normal', 'glorot_normal', rng=20 + layer + seed, batch_normalization=bn)
    if bn:
        for n_ in (ns, no): perturb_bn(n_, rng)
    gnn = CLS[focus](ns, no, d, max_it, thr)
    gnn.native_flags = FLAG if flag else 0
    return gnn


def hidden_stack(focus, d, n_layers, H, thr, scale=1.0, flag=True):
    lg = LGNN([hidden_layer(focus, d, H, True, thr, scale=scale, layer=i, flag=flag) for i in range(n_layers)], True, True)
    return lg


COMP_H = (5, 16, 1)
COMP_ACTS = (('sigmoid', 'tanh'), ('tanh', 'selu'), ('softplus', 'tanh'))
COMP_BN = (True, False, True)


def comp_hidden_stack(focus, d, n_layers, thr, hidden=COMP_H, acts=COMP_ACTS, bn=COMP_BN, scale=1.0, max_it=5, flag=True, dims=DIMS, arc_dim=A):
    """`comp_stack` (tests/test_gpu_composite_grouped.py) with type t's state network Dense(hidden[t], acts[t][0]) - Dense(S, acts[t][1])
    and BatchNormalization per type (`bn[t]`); the output network normalises."""
    wrng = np.random.default_rng(19)
    gnns, dl, al = [], np.array(dims), arc_dim
    for layer in range(n_layers):
        S = d if d > 0 else int(dl.max())
        w_comp = int(dl.sum()) + al
        ns = []
        for t, dt in enumerate(dl):
            n_ = MLP((int(dt) + 2 * S + w_comp,), [min(hidden[t], padded(S)), S], list(acts[t]), 'lecun_normal', 'lecun_normal', rng=30 + t + 10 * layer,
                     batch_normalization=bn[t])
            k0 = 4 if bn[t] else 0
            n_.set_weights([a * scale if a.ndim == 2 else (a + 0.05 if i >= k0 else a) for i, a in enumerate(n_.get_weights())])
            if bn[t]: perturb_bn(n_, wrng)
            ns.append(n_)
        no = MLP((2 * S + al if focus == 'a' else S,), [T], 'softmax', 'glorot_normal', 'glorot_normal', rng=50 + layer, batch_normalization=True)
        perturb_bn(no, wrng)
        gnns.append(CCLS[focus](ns, no, d, max_it, thr))
        gnns[-1].native_flags = FLAG if flag else 0
        dl = np.array(dims) + S + (T if focus != 'a' else 0)
        al = arc_dim + (T if focus == 'a' else 0)
    return CompositeLGNN(gnns, True, True)


# ---- graphs --------------------------------------------------------------------------------------------------------------------------------
def synthetic_graphs(rng, sizes):
    """MUTAG-shaped graphs (one-hot node and arc labels, symmetric arcs) of the given node counts; 1 node: no arc."""
    out = []
    for n in sizes:
        nodes = np.eye(L)[rng.integers(0, L, n)]
        if n == 1: arcs = np.zeros((0, 2 + A))
        else:
            ends = np.array([(i, i + 1) for i in range(n - 1)] + [tuple(sorted(rng.choice(n, 2, replace=False))) for _ in range(n // 4)])
            ends = np.unique(ends, axis=0)
            lab = np.eye(A)[rng.integers(0, A, len(ends))]
            arcs = np.concatenate([np.concatenate([ends, lab], 1), np.concatenate([ends[:, ::-1], lab], 1)])
            arcs = arcs[np.lexsort((arcs[:, 1], arcs[:, 0]))]
        out.append(GraphObject(nodes=nodes, arcs=arcs, targets=np.eye(T)[[int(rng.integers(0, T))]], focus='g', aggregation_mode='average'))
    return out


EDGE_SIZES = (1, 16, 17, 64, 65, 256)


def loop_graphs(mutag_graphs, focus):
    """The MUTAG training subset (groups above 64 nodes: several tiles, parked sums) and groups of 1 (no arc), 16, 17, 64, 65 and 256 nodes."""
    tr, _ = mutag_subsets(mutag_graphs)
    graphs = list(tr[:24]) + synthetic_graphs(np.random.default_rng(3), EDGE_SIZES) + list(tr[24:])
    assert max(g.nodes.shape[0] for g in tr) > 64
    if focus == 'a':                       # (a graph without an arc has no row to refocus on)
        graphs = [g for g in graphs if g.arcs.shape[0] > 0]
    return _refocused(graphs, focus, np.random.default_rng(11), False)


# ---- the oracle's side of a case -----------------------------------------------------------------------------------------------------------
def oracle_pair(gnn, ops_, focus, s0s, thr):
    layer, layer32 = oracle_layer(gnn), oracle_layer(gnn, torch.float32)
    want = torch_train.lgnn_serial_propagate(ops_, layer, focus=focus, get_state=True, get_output=True, state0s=s0s)
    want32 = torch_train.lgnn_serial_propagate(ops_, layer32, focus=focus, get_state=True, get_output=True, state0s=s0s)
    if thr > 0:
        low = [(i, m) for i, m in enumerate(want['margin']) if m < MARGIN]
        assert not low, f'borderline (float64 k within {MARGIN} of flipping): {low}'
        assert len(set(want['k'])) > 1, want['k']
    # (threshold 0: max_iteration - but for a one-node graph behind BatchNormalization, whose state stops moving exactly: k = 2)
    return want, want32


# focus, d, H, BatchNormalization, threshold, activations, scale of the state kernels
LOOP_CASES = {
    'n_d0_H16_bn':         ('n', 0, 16, True, 0.0, ('selu', 'selu'), 1.0),
    'n_d0_H5':             ('n', 0, 5, False, 0.0, ('selu', 'selu'), 1.0),
    'a_d0_H1_bn':          ('a', 0, 1, True, 0.0, ('selu', 'selu'), 1.0),
    'g_d0_H5_bn_thr':      ('g', 0, 5, True, 0.01, ('selu', 'selu'), 0.1),
    'g_d8_H16_bn':         ('g', 8, 16, True, 0.0, ('selu', 'selu'), 1.0),
    'n_d8_H1':             ('n', 8, 1, False, 0.0, ('tanh', 'tanh'), 1.0),
    'a_d8_H5_bn_thr':      ('a', 8, 5, True, 0.01, ('selu', 'selu'), 0.1),
    'n_d20_H32_bn':        ('n', 20, 32, True, 0.0, ('selu', 'selu'), 1.0),
    'a_d20_H5':            ('a', 20, 5, False, 0.0, ('selu', 'tanh'), 1.0),
    'g_d20_H1_bn':         ('g', 20, 1, True, 0.0, ('selu', 'selu'), 1.0),
    'n_d20_H32_bn_thr':    ('n', 20, 32, True, 0.01, ('selu', 'selu'), 0.1),
    'n_d20_H5_sigmoid_bn': ('n', 20, 5, True, 0.0, ('sigmoid', 'tanh'), 1.0),      # act(0) != 0 in the columns at or past H
    'g_d8_H5_softplus':    ('g', 8, 5, False, 0.0, ('softplus', 'selu'), 1.0),
}


def loop_case(mutag_graphs, name):
    focus, d, H, bn, thr, acts, scale = LOOP_CASES[name]
    graphs = loop_graphs(mutag_graphs, focus)
    gnn = hidden_layer(focus, d, H, bn, thr, acts, scale)
    rng = np.random.default_rng(5)
    s0s = [rng.normal(0, 0.1, (g.nodes.shape[0], d)).astype(np.float32) for g in graphs] if d > 0 else None
    seq1 = MultiGraphSequencer(list(graphs), focus, 'average', 4, shuffle=False)
    want, want32 = oracle_pair(gnn, operands(seq1, graphs), focus, s0s, thr)
    return gnn, graphs, s0s, want, want32


def check_groups(gnn, graphs, focus, d, s0s, want, want32, x, tag, name, composite=False):
    """ONE grouped call over the merged batch `x` = the oracle's per-graph calls concatenated."""
    S = d if d > 0 else graphs[0].nodes.shape[1]
    begin = np.concatenate([[0], np.cumsum([g.nodes.shape[0] for g in graphs])])
    state0 = torch.from_numpy(np.concatenate(s0s)).cuda() if d > 0 else None
    if composite:
        if getattr(gnn, '_trainer', None) is None: gnn._trainer = LoopTrainer(gnn)
        k, state, out = gnn._trainer.forward_native(x, state0=state0, node_level=True, groups=begin)
    else:
        k, state, out = gnn.Loop(*gnn.process_inputs(x), training=True, groups=begin, state0=state0, node_level=True)
    assert kernel_name() == name, (tag, kernel_name())
    k = [int(v) for v in k.cpu().numpy()]
    print(f'{tag}: k device {sorted(set(k))} float64 {sorted(set(want["k"]))}')
    assert k == want['k'], (tag, k, want['k'])
    state, out = state.cpu().numpy(), out.cpu().numpy()
    worst, o0 = 0.0, 0
    for i, g in enumerate(graphs):
        mask = np.logical_and(np.asarray(g.set_mask).reshape(-1), np.asarray(g.output_mask).reshape(-1))
        w_out = (want['arcs'][i][:, :T] if focus == 'a' else want['nodes'][i][:, S:S + T])[mask]
        w32_out = (want32['arcs'][i][:, :T] if focus == 'a' else want32['nodes'][i][:, S:S + T])[mask]
        e32 = max(rel_err(want32['nodes'][i][:, :S], want['nodes'][i][:, :S]), rel_err(w32_out, w_out) if len(w_out) else 0.0)
        bar = max(BAR, 2 * e32)
        e = rel_err(state[begin[i]:begin[i + 1]], want['nodes'][i][:, :S])
        n_rows = int(mask.sum())
        if n_rows: e = max(e, rel_err(out[o0:o0 + n_rows], w_out))
        o0 += n_rows
        worst = max(worst, e)
        print(f'{tag} graph {i}: n = {g.nodes.shape[0]}, rel_err {e:.2e} (bar {bar:.2e})')
        assert e <= bar, (tag, i, e, bar)
    assert o0 == out.shape[0]
    worst = max(worst, check_moving_where_normalised(gnn, want, tag))
    log_rows(tag, [dict(worst=worst, k=sorted(set(want['k'])))])
    return k, state, out


def check_moving_where_normalised(gnn, want, tag):
    """`check_moving` (tests/test_gpu_lgnn_serial.py) for layers in which only some networks normalise."""
    nets = list(gnn.net_state) if isinstance(gnn.net_state, (list, tuple)) else [gnn.net_state]
    ref = want['moving_state'] if isinstance(want['moving_state'], list) else [want['moving_state']]
    worst = 0.0
    for name, n_, r in [(f'state{i}', n_, r) for i, (n_, r) in enumerate(zip(nets, ref))] + [('output', gnn.net_output, want['moving_output'])]:
        assert (r is None) == (not n_.batch_normalization), (tag, name)
        if r is None: continue
        got = moving_of(n_)
        for part, a, b in (('mean', got[0], r[0]), ('var', got[1], r[1])):
            e = rel_err(a, b)
            worst = max(worst, e)
            print(f'{tag} moving {name} {part}: rel_err {e:.2e}')
            assert e <= BAR, (tag, name, part, e)
    return worst


# ---- 1. Loop(training=True, groups=...), homogeneous ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(LOOP_CASES))
def test_loop_training_groups_hidden_matches_per_graph_oracle(mutag_graphs, name):
    focus, d = LOOP_CASES[name][:2]
    gnn, graphs, s0s, want, want32 = loop_case(mutag_graphs, name)
    sizes = [g.nodes.shape[0] for g in graphs]
    assert set(EDGE_SIZES) - ({1} if focus == 'a' else set()) <= set(sizes) and max(sizes) == nat.TRAIN_GROUP_MAX_NODES
    x = MultiGraphSequencer(list(graphs), focus, 'average', len(graphs), shuffle=False)[0][0]
    check_groups(gnn, graphs, focus, d, s0s, want, want32, x, f'groups_hidden {name}', HIDDEN)


def weighted_case(thr=0.0):
    """Per-arc weights on the adjacency (the HAS_W instantiations): synthetic graphs, node focus, d = 8, H = 5."""
    from gnnkeras_amd.sparse import SparseMatrix
    rng = np.random.default_rng(29)
    d, H = 8, 5
    graphs = _refocused(synthetic_graphs(rng, (17, 70, 16, 200, 65)), 'n', rng, False)
    ws = [rng.uniform(0.2, 1.0, g.arcs.shape[0]) for g in graphs]

    def batch(g, w):
        an = g.getArcNode(); an.data = np.asarray(w, np.float32)
        m = GraphObject(nodes=g.nodes, arcs=g.arcs, targets=g.targets, focus='n', set_mask=g.set_mask, output_mask=g.output_mask, ArcNode=an,
                        NodeGraph=g.NodeGraph)
        seq = MultiGraphSequencer([m], 'n', 'sum', 1, shuffle=False)
        seq.graph_tensors[0].ArcNode = SparseMatrix.from_scipy(m.ArcNode)
        seq.graph_tensors[0].Adjacency = SparseMatrix.from_scipy(m.Adjacency)
        seq._items = [None]
        return seq[0][0]
    merged = GraphObject.merge(graphs, 'n', 'sum')
    begin = np.concatenate([[0], np.cumsum([g.nodes.shape[0] for g in graphs])])
    for i, g in enumerate(graphs):          # the merged arcs are the graphs' arcs one after the other: so are the weights
        e0 = sum(h.arcs.shape[0] for h in graphs[:i])
        assert np.array_equal(merged.arc_ids[e0:e0 + g.arcs.shape[0]] - begin[i], g.arc_ids)
    x = batch(merged, np.concatenate(ws))
    ops_ = []
    for g, w in zip(graphs, ws):
        nodes, arcs, dnl, sm, om, adj, an, _ng = batch(g, w)
        ops_.append(dict(nodes=_np(nodes), arcs=_np(arcs), dim_node_label=_np(dnl).reshape(-1), set_mask=_np(sm).reshape(-1),
                         output_mask=_np(om).reshape(-1), adjacency=_triple(adj), arcnode=_triple(an),
                         t0=dict(nodes=g.nodes, arcs=g.arcs, dim_node_label=g.DIM_NODE_LABEL)))
    gnn = hidden_layer('n', d, H, True, thr, ('selu', 'selu'), 1.0)
    s0s = [rng.normal(0, 0.1, (g.nodes.shape[0], d)).astype(np.float32) for g in graphs]
    want, want32 = oracle_pair(gnn, ops_, 'n', s0s, thr)
    return gnn, graphs, s0s, want, want32, x


def test_loop_training_groups_hidden_with_per_arc_weights():
    gnn, graphs, s0s, want, want32, x = weighted_case()
    assert x[5].matrix.csr().w is not None
    check_groups(gnn, graphs, 'n', 8, s0s, want, want32, x, 'groups_hidden per-arc weights', HIDDEN)


FORMS = [(kind, d, weighted) for kind in ('homogeneous', 'composite') for d in (6, 20) for weighted in (False, True)]


def forms_case(kind, d, weighted):
    """One case of tests/test_gpu_train_group_forms.py (four Erdos-Renyi graphs: one tile, a full tile, one row into a second tile,
    several tiles; per-arc weights on the merged Adjacency and on the oracle's operands) with a hidden layer in every state network."""
    from test_gpu_train_group_forms import K, L as L5, build_case
    _, x, begin, ops_, s0s, graphs = build_case(kind, d, weighted)
    if kind == 'composite': gnn = comp_hidden_stack('n', d, 1, 0.0, max_it=K).gnns[0]
    else:
        wrng = np.random.default_rng(19)
        inp, lay = get_inout_dims('state', L5, A, T, 'n', d, hidden_units=[padded(d) - 3])
        ns = MLP(inp[0], lay, ['softplus', 'selu'], 'lecun_normal', 'lecun_normal', rng=10, batch_normalization=True)
        inp, lay = get_inout_dims('output', L5, A, T, 'n', d)
        no = MLP(inp[0], lay, 'softmax', 'glorot_normal', 'glorot_normal', rng=20, batch_normalization=True)
        for n_ in (ns, no): perturb_bn(n_, wrng)
        gnn = CLS['n'](ns, no, d, K, 0.0)
        gnn.native_flags = FLAG
    want, want32 = oracle_pair(gnn, ops_, 'n', s0s, 0.0)
    assert want['k'] == [K] * len(graphs)
    return gnn, graphs, s0s, want, want32, x


@pytest.mark.parametrize('kind,d,weighted', FORMS)
def test_every_hidden_instantiation_matches_the_float64_oracle(kind, d, weighted):
    """All eight hidden instantiations: model kind x padded width 16 / 32 (state widths 6 / 20: pad columns in both) x per-arc weights."""
    gnn, graphs, s0s, want, want32, x = forms_case(kind, d, weighted)
    assert (x[7 if kind == 'composite' else 5].matrix.csr().w is not None) == weighted
    check_groups(gnn, graphs, 'n', d, s0s, want, want32, x, f'groups_hidden forms {kind} d={d} weighted={weighted}',
                 HIDDEN_TYPES if kind == 'composite' else HIDDEN, composite=kind == 'composite')


# ---- 2. the same for a composite model -----------------------------------------------------------------------------------------------------
COMP_CASES = {'n_d6': ('n', 6, 0.0, 1.0), 'a_d6': ('a', 6, 0.0, 1.0), 'n_d20_thr': ('n', 20, 0.01, 0.2), 'n_d0': ('n', 0, 0.0, 1.0)}


def comp_case(name):
    focus, d, thr, scale = COMP_CASES[name]
    rng = np.random.default_rng(41)
    sizes = (16, 17, 9, 64, 65, 120, 256, 40) if focus != 'a' else (16, 17, 9, 64, 65, 100)
    graphs = typed_graphs(rng, sizes, 500, focus, absent=1, lonely=2)
    assert not np.array(graphs[1].type_mask).reshape(-1, len(DIMS))[:, 2].any()          # one group has no row of one type
    gnn = comp_hidden_stack(focus, d, 1, thr, scale=scale).gnns[0]
    s0s = [rng.normal(0, 0.1, (g.nodes.shape[0], d)).astype(np.float32) for g in graphs] if d > 0 else None
    seq1 = CompositeMultiGraphSequencer(list(graphs), focus, MODE, 4, shuffle=False)
    want, want32 = oracle_pair(gnn, operands(seq1, graphs, True), focus, s0s, thr)
    return gnn, graphs, s0s, want, want32


@pytest.mark.parametrize('name', list(COMP_CASES))
def test_composite_groups_hidden_match_per_graph_oracle(name):
    """Three types; H and both activations differ per type; type 1 has no BatchNormalization."""
    focus, d = COMP_CASES[name][:2]
    gnn, graphs, s0s, want, want32 = comp_case(name)
    x = CompositeMultiGraphSequencer(list(graphs), focus, MODE, len(graphs), shuffle=False)[0][0]
    check_groups(gnn, graphs, focus, d, s0s, want, want32, x, f'composite_groups_hidden {name}', HIDDEN_TYPES, composite=True)


# ---- 3. grouped serial propagation of a stack ----------------------------------------------------------------------------------------------
def stack_sets(mutag_graphs):
    tr, va = mutag_subsets(mutag_graphs)
    rng = np.random.default_rng(11)
    return [_refocused(tr, 'g', rng, False), _refocused(va, 'g', rng, False)]


def comp_sets():
    rng = np.random.default_rng(17)
    return [typed_graphs(rng, (30, 12, 9, 200, 65, 64, 17, 100), 100, 'n', absent=1, lonely=2), typed_graphs(rng, (20, 70, 150, 8), 200, 'n')]


@pytest.mark.parametrize('flag', [True, False])
def test_lgnn_grouped_propagation_with_hidden_state_networks(mutag_graphs, flag):
    """A 2-layer LGNN (d = 0: padded widths 16, then 32), H = 10, threshold 0.01, serial_propagation='grouped': with the flag on every
    layer one library call per run on the hidden kernels; without it the per-graph route (passes before the flag existed)."""
    lg = hidden_stack('g', 0, 2, 10, 0.01, scale=0.1, flag=flag)
    lg.serial_propagation = 'grouped'
    seen = spy_on_propagate(lg)
    sets = stack_sets(mutag_graphs)
    rows = run_serial_chain(lg, sets, 'g', 0, kernels=None, tag=f'lgnn_grouped_hidden flag={flag}')
    assert len(seen) == 4
    for (li, rec, name), n_graphs in zip(seen, [len(s) for _ in range(2) for s in sets]):
        if flag: assert rec == ONE_RUN and name == HIDDEN, (li, rec, name)
        else: assert rec['route'] == 'per_graph' and rec['library_calls'] == n_graphs and name not in (HIDDEN, GROUPED), (li, rec, name)
    assert len(set(k for r_ in rows for k in r_['k'])) > 1


@pytest.mark.parametrize('flag', [True, False])
def test_composite_lgnn_grouped_propagation_with_hidden_state_networks(flag):
    """A 2-layer CompositeLGNN (state 6; H and the activations per type; every network normalises, as run_serial_chain's check of the
    moving statistics expects), threshold 0."""
    lg = comp_hidden_stack('n', 6, 2, 0.0, bn=(True, True, True), flag=flag)
    lg.serial_propagation = 'grouped'
    seen = spy_on_propagate(lg)
    sets = comp_sets()
    run_serial_chain(lg, sets, 'n', 6, seq_cls=CompositeMultiGraphSequencer, tag=f'composite_lgnn_grouped_hidden flag={flag}')
    assert len(seen) == 4
    for (li, rec, name), n_graphs in zip(seen, [len(s) for _ in range(2) for s in sets]):
        if flag: assert rec == ONE_RUN and name == HIDDEN_TYPES, (li, rec, name)
        else: assert rec['route'] == 'per_graph' and rec['library_calls'] == n_graphs and name not in (HIDDEN_TYPES, GROUPED_TYPES), (li, rec, name)


# ---- 4. the flag on a one-layer model changes nothing --------------------------------------------------------------------------------------
def test_the_flag_on_one_layer_models_changes_nothing(mutag_graphs):
    tr, _ = mutag_subsets(mutag_graphs)
    graphs = _refocused(tr, 'n', np.random.default_rng(11), False)
    begin = np.concatenate([[0], np.cumsum([g.nodes.shape[0] for g in graphs])])
    x = MultiGraphSequencer(list(graphs), 'n', 'average', len(graphs), shuffle=False)[0][0]
    got = []
    for flags in (0, FLAG):
        gnn = _single_layer('n', 0, True, 0.01)
        gnn.native_flags = flags
        k, state, out = gnn.Loop(*gnn.process_inputs(x), training=True, groups=begin, node_level=True)
        assert kernel_name() == GROUPED
        got.append([k.cpu().numpy(), state.cpu().numpy(), out.cpu().numpy()] + list(moving_of(gnn.net_state)))
    for a, b in zip(*got): assert np.array_equal(a, b)
    # composite
    rng = np.random.default_rng(41)
    cg = typed_graphs(rng, (16, 70, 9, 130), 500, 'n', absent=1)
    cbegin = np.concatenate([[0], np.cumsum([g.nodes.shape[0] for g in cg])])
    cx = CompositeMultiGraphSequencer(list(cg), 'n', MODE, len(cg), shuffle=False)[0][0]
    s0 = torch.from_numpy(rng.normal(0, 0.1, (cbegin[-1], 6)).astype(np.float32)).cuda()
    got = []
    for flags in (0, FLAG):
        gnn = comp_stack('n', 6, 1, 0.01, scale=0.025).gnns[0]
        gnn.native_flags = flags
        k, state, out = LoopTrainer(gnn).forward_native(cx, state0=s0, node_level=True, groups=cbegin)
        assert kernel_name() == GROUPED_TYPES
        got.append([k.cpu().numpy(), state.cpu().numpy(), out.cpu().numpy()] + [w for n_ in gnn.net_state for w in moving_of(n_)])
    for a, b in zip(*got): assert np.array_equal(a, b)


# ---- 5. group order ------------------------------------------------------------------------------------------------------------------------
def order_case(graphs):
    """Layer 0 of the hidden stack (threshold 0.01) over `graphs` in the given order: the layer and the oracle's answer."""
    lg = hidden_stack('g', 0, 2, 10, 0.01, scale=0.1)
    lg.serial_propagation = 'grouped'
    gnn = lg.gnns[0]
    layer = oracle_layer(gnn)
    seq_now = MultiGraphSequencer(list(graphs), 'g', 'average', 4, shuffle=True)
    want = torch_train.lgnn_serial_propagate(operands(seq_now, graphs), layer, focus='g', get_state=True, get_output=True)
    assert min(want['margin']) >= MARGIN and len(set(want['k'])) > 1
    return lg, gnn, seq_now, want


def _one_pass(graphs, tag):
    lg, gnn, seq_now, want = order_case(graphs)
    seq_t0 = MultiGraphSequencer(list(graphs), 'g', 'average', 4, shuffle=True)
    new_seq, ks = lg._propagate(gnn, seq_now, seq_t0)
    assert lg.last_propagate == ONE_RUN and kernel_name() == HIDDEN
    assert ks == want['k'], (tag, ks, want['k'])
    check_moving_where_normalised(gnn, want, tag)
    return want, (moving_of(gnn.net_state), moving_of(gnn.net_output)), new_seq.data, ks


def test_group_order_decides_the_moving_statistics_hidden(mutag_graphs):
    """The same graphs in reversed order: the moving statistics follow the oracle run in reversed order and differ from the forward-order
    result; k and the relabelled columns of every graph are the same bits in both orders (no arithmetic crosses graphs)."""
    tr, _ = mutag_subsets(mutag_graphs)
    fwd_want, fwd_mov, fwd_graphs, fwd_k = _one_pass(tr, 'hidden order forward')
    rev_want, rev_mov, rev_graphs, rev_k = _one_pass(tr[::-1], 'hidden order reversed')
    gap64 = max(rel_err(a, b) for key in ('moving_state', 'moving_output') for a, b in zip(fwd_want[key], rev_want[key]))
    assert gap64 > 4 * BAR, gap64           # precondition (float64): the order matters by far more than the bar on these graphs
    gap = max(rel_err(a, b) for f, r in zip(fwd_mov, rev_mov) for a, b in zip(f, r))
    assert gap > 2 * BAR, gap
    assert fwd_k == rev_k[::-1]
    for a, b in zip(fwd_graphs, rev_graphs[::-1]):
        assert np.array_equal(a.nodes, b.nodes) and np.array_equal(a.arcs, b.arcs)
    log_rows('lgnn_grouped_hidden order', [dict(gap_float64=gap64, gap_device=gap)])
