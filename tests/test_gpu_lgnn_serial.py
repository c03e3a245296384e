"""Serial LGNN (reference LGNN.py:290-362, the default run of the reference's starter) against the float64 restatement of its
propagation, `oracle.torch_train.lgnn_serial_propagate`: between two layers every graph runs ALONE through the trained layer in training
mode - BatchNormalization on that graph's own statistics, the moving averages moved once per executed call, training graphs first, then
validation graphs - and `update_graph` merges the state / output into the ORIGINAL labels.

The tests hold `LGNN._propagate` and `fit()` to their contract - relabelled graphs, per-graph k, moving statistics - not to how many
library calls a propagation makes.  Bars: the relabelled columns within `rel_err` 2e-5 of float64 (the bar the fuzz tests hold the
forward to), k exact, everything that is copied (labels, targets, masks, the t0 graphs) bit for bit.  With threshold 0.01 every k is
first checked to be at least 1e-3 (relative) away from flipping in float64, so a k mismatch is a kernel error, not a borderline graph."""
import numpy as np
import pytest
import torch

from gnnkeras_amd import GraphObject
from gnnkeras_amd import _native as nat
from gnnkeras_amd.Models.MLP import MLP, get_inout_dims
from gnnkeras_amd.Models.GNN import GNNnodeBased, GNNarcBased, GNNgraphBased
from gnnkeras_amd.Models.LGNN import LGNN
from gnnkeras_amd.Models.training import Adam
from gnnkeras_amd.Sequencers.GraphSequencers import MultiGraphSequencer
from oracle import torch_train
from oracle.harness import rel_err, _np, _triple
from test_gpu_training import log_rows, refocus

pytestmark = pytest.mark.gpu
CLS = {'n': GNNnodeBased, 'a': GNNarcBased, 'g': GNNgraphBased}
BAR = 2e-5              # relabelled columns and moving statistics vs float64 (the forward's fuzz bar)
MARGIN = 1e-3           # with threshold > 0: every k at least this far (relative) from flipping in float64
PERSISTENT, GENERAL = 'train_step: persistent small-graph kernels', 'train_step: general kernels'


def perturb_bn(net, rng):
    """Non-trivial gamma / beta, and moving statistics away from their (0, 1) start: a reset or a frozen average cannot pass."""
    w = net.get_weights()
    w[0] = rng.uniform(0.7, 1.3, w[0].shape).astype(np.float32); w[1] = rng.normal(0, 0.2, w[1].shape).astype(np.float32)
    w[2] = rng.normal(0, 0.5, w[2].shape).astype(np.float32); w[3] = rng.uniform(0.5, 2.0, w[3].shape).astype(np.float32)
    net.set_weights(w)


def serial_stack(focus, d, n_layers, get_state, get_output, thr, max_it=5, T=2, state_scale=1.0):
    """The starter's stack (selu state networks, softmax outputs, no hidden layers), BatchNormalization everywhere; `state_scale` shrinks
    the state kernels (a contracting state map: graphs stop before max_iteration, each at its own k)."""
    rng = np.random.default_rng(7)
    gnns = []
    for i in range(n_layers):
        inp, lay = get_inout_dims('state', 14, 3, T, focus, d, layer=i, get_state=get_state, get_output=get_output)
        ns = MLP(inp[0], lay, 'selu', 'lecun_normal', 'lecun_normal', rng=10 + i, batch_normalization=True)
        ns.set_weights([a * state_scale if a.ndim == 2 else a for a in ns.get_weights()])
        inp, lay = get_inout_dims('output', 14, 3, T, focus, d, layer=i, get_state=get_state, get_output=get_output)
        no = MLP(inp[0], lay, 'softmax', 'glorot_normal', 'glorot_normal', rng=20 + i, batch_normalization=True)
        for n_ in (ns, no): perturb_bn(n_, rng)
        gnns.append(CLS[focus](ns, no, d, max_it, thr))
    return LGNN(gnns, get_state, get_output)


def mutag_subsets(graphs, offset=0):
    """~48 training / 16 validation MUTAG graphs, each set with 4 graphs over 64 nodes (several workgroups of the persistent kernel) and
    4 of at most 8 nodes (BatchNormalization over a handful of rows); in data set order."""
    n = np.array([g.nodes.shape[0] for g in graphs])
    big, small, mid = np.flatnonzero(n > 64), np.flatnonzero(n <= 8), np.flatnonzero((n > 8) & (n <= 64))
    take = lambda a, lo, cnt: [int(i) for i in a[offset + lo:offset + lo + cnt]]
    tr = sorted(take(big, 0, 4) + take(small, 0, 4) + take(mid, 0, 40))
    va = sorted(take(big, 4, 4) + take(small, 4, 4) + take(mid, 40, 8))
    out = []
    for idx in (tr, va):
        gl = [graphs[i].copy() for i in idx]
        for g in gl: g.setAggregation('average')
        out.append(gl)
    return out


def snapshot(g):
    """Every array of a graph (copies), to check what must not change."""
    keys = ('nodes', 'arcs', 'targets', 'set_mask', 'output_mask', 'sample_weight', 'DIM_NODE_LABEL')
    snap = {k: np.array(getattr(g, k), copy=True) for k in keys}
    if hasattr(g, 'type_mask'): snap['type_mask'] = np.array(g.type_mask, copy=True)
    return snap


def assert_same(a, b, what):
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (what, k)


def operands(seq, t0_graphs, composite=False):
    """The oracle's per-graph operands: exactly what a batch-size-1 sequencer over `seq`'s graphs hands to the model, plus the t0
    labels update_graph extends."""
    seq1 = type(seq)(list(seq.data), seq.focus, seq.aggregation_mode, 1, shuffle=False)
    ops_ = []
    for i, g0 in enumerate(t0_graphs):
        x = seq1[i][0]
        if composite:
            nodes, arcs, dnl, tm, sm, om, cas, adj, an, _ng = x
            tm_ = _np(tm)
            extra = dict(type_mask=tm_.reshape(tm_.shape[0], -1), composite_adjacencies=[_triple(c) for c in cas])
        else:
            nodes, arcs, dnl, sm, om, adj, an, _ng = x
            extra = {}
        ops_.append(dict(nodes=_np(nodes), arcs=_np(arcs), dim_node_label=_np(dnl).reshape(-1), set_mask=_np(sm).reshape(-1),
                         output_mask=_np(om).reshape(-1), adjacency=_triple(adj), arcnode=_triple(an),
                         t0=dict(nodes=g0.nodes, arcs=g0.arcs, dim_node_label=g0.DIM_NODE_LABEL), **extra))
    return ops_


def oracle_layer(gnn, dtype=torch.float64):
    composite = isinstance(gnn.net_state, (list, tuple))
    spec_s = [n_.spec() for n_ in gnn.net_state] if composite else gnn.net_state.spec()
    return torch_train.serial_layer(spec_s, gnn.net_output.spec(), gnn.state_vect_dim, gnn.max_iteration, gnn.state_threshold, dtype=dtype)


def merged_err(a_nodes, a_arcs, b_nodes, b_arcs, plus, focus, T):
    """rel_err of the columns update_graph merged in: nodes[:, :plus] (and arcs[:, :T] for arc focus)."""
    e = rel_err(a_nodes[:, :plus], b_nodes[:, :plus])
    return max(e, rel_err(a_arcs[:, :T], b_arcs[:, :T])) if focus == 'a' else e


def moving_of(net):
    w = net.get_weights()
    return w[2], w[3]


def check_moving(gnn, want, tag):
    """The moving mean / variance of both networks of a layer against the oracle's; returns the worst error."""
    nets = list(gnn.net_state) if isinstance(gnn.net_state, (list, tuple)) else [gnn.net_state]
    ref = want['moving_state'] if isinstance(want['moving_state'], list) else [want['moving_state']]
    worst = 0.0
    for name, n_, r in [(f'state{i}', n_, r) for i, (n_, r) in enumerate(zip(nets, ref))] + [('output', gnn.net_output, want['moving_output'])]:
        got = moving_of(n_)
        for part, a, b in (('mean', got[0], r[0]), ('var', got[1], r[1])):
            e = rel_err(a, b)
            worst = max(worst, e)
            assert e <= BAR, (tag, name, part, e)
    return worst


def check_relabelled(got_graphs, want, t0_snaps, plus, focus, T, tag, bars=None):
    """Per graph: shapes and DIM_NODE_LABEL exact, the merged columns within BAR (or `bars[i]`), the copied columns / targets / masks
    bit for bit.  `plus` = state columns in front of the labels (+ T output columns for node / graph focus)."""
    worst = dict(nodes=0.0, arcs=0.0)
    for gi, (g, snap) in enumerate(zip(got_graphs, t0_snaps)):
        bar = BAR if bars is None else bars[gi]
        wn, wa, wl = want['nodes'][gi], want['arcs'][gi], want['dim_node_label'][gi]
        assert g.nodes.shape == wn.shape and g.arcs.shape == wa.shape, (tag, gi, g.nodes.shape, wn.shape, g.arcs.shape, wa.shape)
        assert g.nodes.dtype == np.float32 and g.arcs.dtype == np.float32, (tag, gi)
        assert np.array_equal(np.asarray(g.DIM_NODE_LABEL), np.asarray(wl)), (tag, gi, g.DIM_NODE_LABEL, wl)
        assert np.array_equal(g.nodes[:, plus:], snap['nodes'].astype(np.float32)), (tag, gi, 'original node labels')
        e = rel_err(g.nodes[:, :plus], wn[:, :plus])
        worst['nodes'] = max(worst['nodes'], e)
        assert e <= bar, (tag, gi, 'nodes', e, bar)
        if focus == 'a':
            assert np.array_equal(g.arcs[:, T:], snap['arcs'].astype(np.float32)), (tag, gi, 'original arcs')
            e = rel_err(g.arcs[:, :T], wa[:, :T])
            worst['arcs'] = max(worst['arcs'], e)
            assert e <= bar, (tag, gi, 'arcs', e, bar)
        else:
            assert np.array_equal(g.arcs, snap['arcs'].astype(np.float32)), (tag, gi, 'arcs')
        for k in ('targets', 'set_mask', 'output_mask', 'sample_weight') + (('type_mask',) if 'type_mask' in snap else ()):
            assert np.array_equal(np.asarray(getattr(g, k)), snap[k]), (tag, gi, k)
    return worst


def kernel_name():
    return nat.lib().gnn_last_kernel_name().decode()


# focus, d, get_state, get_output, layers, threshold, the train_step path each layer's forward must take (None: not pinned), one graph
# without output rows.  Threshold 0.01 rows shrink the state kernels to 0.01 (selu behind BatchNormalization only contracts once the
# rows' spread is below sqrt(epsilon)): on these subsets the graphs then stop at k = 3, 4 or 5 ('a_d8_early': 3), every k >= 2.7e-3
# from flipping in float64.
ROWS = {
    'starter':        ('g', 0, True, True, 3, 0.01, [PERSISTENT] * 3, False),
    'starter_thr0':   ('g', 0, True, True, 3, 0.0, [PERSISTENT] * 3, False),
    'g_d8_state':     ('g', 8, True, False, 2, 0.0, [PERSISTENT, GENERAL], False),
    'n_empty_output': ('n', 0, True, True, 2, 0.01, None, True),
    'n_d8_output':    ('n', 8, False, True, 2, 0.0, None, False),
    'a_prepend':      ('a', 0, True, True, 2, 0.0, None, False),
    'a_d8_early':     ('a', 8, False, True, 2, 0.01, None, False),
}


def _refocused(graphs, focus, rng, empty):
    gl = refocus(graphs, focus, rng)
    if empty:
        # one small graph (not the last one: the kernel name is read behind the last) without a single output row
        i = next(i for i, g in enumerate(gl[:-1]) if g.nodes.shape[0] <= 8)
        g = gl[i]
        n = g.nodes.shape[0]
        gl[i] = GraphObject(nodes=g.nodes, arcs=g.arcs, targets=np.zeros((0, 2)), focus=focus, set_mask=np.ones(n, bool),
                            output_mask=np.zeros(n, bool), sample_weight=np.ones(0))
    for g in gl: g.setAggregation('average')
    return gl


def run_serial_chain(lg, sets_t0, focus, d, seq_cls=MultiGraphSequencer, kernels=None, tag=''):
    """Propagate every layer of `lg`: the training set, then the validation set, through `LGNN._propagate`, each against the oracle
    started from the layer's own weights and moving statistics; layer i + 1 is fed the graphs the device relabelled.
    A graph on which the float32 restatement itself lands further than BAR / 2 from float64 (a few nodes, BatchNormalization over
    them, five unscaled selu iterations: measured up to 5.6e-5 on a 4-node graph of 'g_d8_state') is held to twice that distance."""
    rng = np.random.default_rng(5)
    composite = seq_cls is not MultiGraphSequencer
    t0_snaps = [[snapshot(g) for g in gl] for gl in sets_t0]
    cur = [list(gl) for gl in sets_t0]
    rows, names = [], []
    for li, gnn in enumerate(lg.gnns):
        layer, layer32 = oracle_layer(gnn), oracle_layer(gnn, torch.float32)      # (before the device moves the statistics)
        T = gnn.net_output.units[-1]
        S = d if d > 0 else (cur[0][0].nodes.shape[1])
        plus = (S if lg.get_state else 0) + (T if lg.get_output and focus != 'a' else 0)
        new_sets = []
        for si, (graphs_now, graphs_t0) in enumerate(zip(cur, sets_t0)):
            what = f'{tag} layer {li} {"train" if si == 0 else "valid"}'
            now_snaps = [snapshot(g) for g in graphs_now]
            seq_now = seq_cls(list(graphs_now), focus, 'average' if not composite else 'composite_average', 4, shuffle=True)
            seq_t0 = seq_cls(list(graphs_t0), focus, 'average' if not composite else 'composite_average', 4, shuffle=True)
            ops_ = operands(seq_now, graphs_t0, composite)
            s0s = [rng.normal(0, 0.1, (g.nodes.shape[0], d)).astype(np.float32) for g in graphs_now] if d > 0 else None
            want = torch_train.lgnn_serial_propagate(ops_, layer, focus=focus, get_state=lg.get_state, get_output=lg.get_output,
                                                     state0s=s0s)
            want32 = torch_train.lgnn_serial_propagate(ops_, layer32, focus=focus, get_state=lg.get_state, get_output=lg.get_output,
                                                       state0s=s0s)
            e32 = [merged_err(*a, *b, plus, focus, T) for a, b in zip(zip(want32['nodes'], want32['arcs']), zip(want['nodes'], want['arcs']))]
            bars = [max(BAR, 2 * e) for e in e32]
            if gnn.state_threshold > 0:
                low = [(i, m) for i, m in enumerate(want['margin']) if m < MARGIN]
                assert not low, f'{what}: borderline subset (float64 k within {MARGIN} of flipping): {low} - pick another subset'
            new_seq, ks = lg._propagate(gnn, seq_now, seq_t0, None if s0s is None else [torch.from_numpy(s).cuda() for s in s0s])
            if si == 0: names.append(kernel_name())
            assert ks == want['k'], (what, ks, want['k'])
            if gnn.state_threshold == 0: assert set(ks) == {gnn.max_iteration}
            worst = check_relabelled(new_seq.data, want, [snapshot(g) for g in graphs_t0], plus, focus, T, what, bars)
            worst['f32_oracle'] = max(e32)
            worst['widened'] = [(i, b) for i, b in enumerate(bars) if b > BAR]
            worst['moving'] = check_moving(gnn, want, what)
            for g, snap in zip(graphs_now, now_snaps): assert_same(snapshot(g), snap, (what, 'input graph'))
            for g, snap in zip(graphs_t0, t0_snaps[si]): assert_same(snapshot(g), snap, (what, 't0 graph'))
            rows.append(dict(layer=li, set=si, k=sorted(set(want['k'])), min_margin=min(want['margin']), **worst))
            new_sets.append(new_seq.data)
        cur = new_sets
    log_rows(tag, rows, kernels=names)
    if kernels is not None:
        assert names == kernels, (tag, names)
    return rows


@pytest.mark.parametrize('row', list(ROWS))
def test_propagate_matches_float64_oracle(mutag_graphs, row):
    """`LGNN._propagate` of every layer (training set, then validation set) against `lgnn_serial_propagate`, BatchNormalization on."""
    focus, d, get_state, get_output, n_layers, thr, kernels, empty = ROWS[row]
    tr, va = mutag_subsets(mutag_graphs)
    rng = np.random.default_rng(11)
    sets_t0 = [_refocused(tr, focus, rng, empty), _refocused(va, focus, rng, False)]
    lg = serial_stack(focus, d, n_layers, get_state, get_output, thr, state_scale=0.01 if thr > 0 else 1.0)
    rows = run_serial_chain(lg, sets_t0, focus, d, kernels=kernels, tag=f'lgnn_serial {row}')
    if row == 'starter': assert len(set(k for r_ in rows for k in r_['k'])) > 1      # per-graph early exit really happens


def test_composite_propagate_matches_float64_oracle():
    """CompositeLGNN (one state network per node type) on the building-block training forward: 3 types, D = 6, node focus."""
    from gnnkeras_amd import CompositeGraphObject
    from gnnkeras_amd.Models.CompositeGNN import CompositeGNNnodeBased
    from gnnkeras_amd.Models.CompositeLGNN import CompositeLGNN
    from gnnkeras_amd.Sequencers.GraphSequencers import CompositeMultiGraphSequencer
    from gnnkeras_amd.synth import er_composite_graph
    dims, D, T, A = (5, 3, 4), 6, 2, 3
    rng = np.random.default_rng(17)

    def graphs(seed0, count):
        out = []
        for i in range(count):
            n = int(rng.integers(6, 90))
            g = er_composite_graph(n, int(rng.integers(n, 3 * n)), dim_node_label=dims, seed=seed0 + i)
            om = rng.random(n) < 0.7
            out.append(CompositeGraphObject(nodes=g.nodes, arcs=g.arcs, targets=np.eye(T)[rng.integers(0, T, int(om.sum()))],
                                            type_mask=g.type_mask, dim_node_label=dims, focus='n', set_mask=rng.random(n) < 0.8,
                                            output_mask=om, aggregation_mode='composite_average'))
        return out
    gnns = []
    wrng = np.random.default_rng(19)
    for layer in range(2):
        inp, lay = get_inout_dims('state', dims, A, T, 'n', D, layer=layer, get_state=True, get_output=True)
        ns = [MLP(i, lay, 'tanh', 'lecun_normal', 'lecun_normal', rng=30 + t + 10 * layer, batch_normalization=True) for t, i in enumerate(inp)]
        inp, lay = get_inout_dims('output', dims, A, T, 'n', D, layer=layer, get_state=True, get_output=True)
        no = MLP(inp[0], lay, 'softmax', 'glorot_normal', 'glorot_normal', rng=50 + layer, batch_normalization=True)
        for n_ in ns + [no]: perturb_bn(n_, wrng)
        gnns.append(CompositeGNNnodeBased(ns, no, D, 4, 0.0))
    lg = CompositeLGNN(gnns, True, True)
    run_serial_chain(lg, [graphs(100, 12), graphs(200, 6)], 'n', D, seq_cls=CompositeMultiGraphSequencer, tag='lgnn_serial composite')


def test_fit_layer_boundaries_match_float64_oracle(mutag_graphs):
    """`fit()` end to end on the starter stack (3 layers, d = 0, selu / softmax, BatchNormalization, max_iteration 5; threshold 0 so trained
    weights cannot make a k borderline), 2 shuffled epochs per layer with validation data.  At every layer boundary the graphs layer i + 1
    is handed - and layer i's moving statistics at that point - are the oracle's propagation of layer i's input graphs (training set,
    then validation set) with the weights and statistics layer i's fit() ended with."""
    tr_graphs, va_graphs = mutag_subsets(mutag_graphs)
    tr = MultiGraphSequencer(tr_graphs, 'g', 'average', 16, shuffle=True)
    va = MultiGraphSequencer(va_graphs, 'g', 'average', 16, shuffle=False)
    caller = [(list(s.data), [snapshot(g) for g in s.data]) for s in (tr, va)]
    lg = serial_stack('g', 0, 3, True, True, 0.0)
    lg.compile(optimizer=Adam(0.01), loss='categorical_crossentropy', training_mode='serial', average_st_grads=True, metrics=['accuracy'])
    A, B = {}, {}
    spec_of = lambda gnn: (gnn.net_state.spec(), gnn.net_output.spec())
    for i, gnn in enumerate(lg.gnns):
        def wrapped(seq, *args, _i=i, _fit=gnn.fit, **kwargs):
            B[_i] = dict(train=[g.copy() for g in seq.data], valid=[g.copy() for g in kwargs['validation_data'].data],
                         prev=spec_of(lg.gnns[_i - 1]) if _i > 0 else None)
            out = _fit(seq, *args, **kwargs)
            A[_i] = spec_of(lg.gnns[_i])
            return out
        gnn.fit = wrapped
    np.random.seed(3)
    hists = lg.fit(tr, epochs=2, validation_data=va, verbose=0)
    assert len(hists) == 3 and sorted(A) == sorted(B) == [0, 1, 2]
    for s, (order, snaps) in zip((tr, va), caller):                 # the caller's sequencers: same graphs, same order, same arrays
        assert len(s.data) == len(order) and all(a is b for a, b in zip(s.data, order))
        for g, snap in zip(s.data, snaps): assert_same(snapshot(g), snap, 'caller graph')
    rows = []
    for i in range(2):
        layer = torch_train.serial_layer(*A[i], 0, 5, 0.0)
        gnn = lg.gnns[i]
        got = {}
        for key, t0 in (('train', tr_graphs), ('valid', va_graphs)):
            seq_in = MultiGraphSequencer(B[i][key], 'g', 'average', 1, shuffle=False)
            want = torch_train.lgnn_serial_propagate(operands(seq_in, t0), layer, focus='g', get_state=True, get_output=True)
            assert want['k'] == [5] * len(t0)
            plus = B[i][key][0].nodes.shape[1] + 2
            got[key] = check_relabelled(B[i + 1][key], want, [snapshot(g) for g in t0], plus, 'g', 2, f'fit boundary {i} {key}')
        # layer i's statistics as layer i + 1 starts = the oracle's after the training AND the validation graphs
        for (name, (spec, w)), ref in zip((('state', B[i + 1]['prev'][0]), ('output', B[i + 1]['prev'][1])),
                                          (want['moving_state'], want['moving_output'])):
            for part, a, b in (('mean', w[2], ref[0]), ('var', w[3], ref[1])):
                e = rel_err(a, b)
                got.setdefault('moving', 0.0)
                got['moving'] = max(got['moving'], e)
                assert e <= BAR, (f'fit boundary {i}', name, part, e)
            # (and they moved: the propagation really ran in training mode from where fit() left them)
            assert not np.array_equal(w[2], A[i][0 if name == 'state' else 1][1][2])
        rows.append(dict(boundary=i, **{f'{k}_nodes': v['nodes'] for k, v in got.items() if isinstance(v, dict)}, moving=got['moving']))
    log_rows('lgnn_serial fit', rows)
