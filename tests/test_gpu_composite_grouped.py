"""Training-mode convergence groups of HETEROGENEOUS models: `CompositeLGNN` with `serial_propagation = 'grouped'`, the grouped
`LoopTrainer.forward_native(groups=...)` on composite batches, and the composite training-mode forward alone as ONE library call
(`CompositeGNN*.Loop(training=True)`) - against the float64 restatement `oracle.torch_train.lgnn_serial_propagate` (composite layers run
`_composite_forward`), through the checks, bars and helpers of tests/test_gpu_lgnn_serial.py: k exact per graph, merged columns and moving
statistics within rel_err 2e-5 of float64 (a graph on which the float32 oracle itself is further away: twice that distance), copied data bit
for bit; with a threshold every k is first checked to be 1e-3 away from flipping in float64.

Constant input columns of type t's network: Kc_t = d_t + W_comp, W_comp = sum(d_t) + A, at most 64.  The synthetic stack (3 types, labels
(5, 3, 4), A = 3, state 6) has Kc <= 20 at layer 0 and (13, 11, 12) + 39 = up to 52 at layer 1; the reference's composite MUTAG stack
(one type, d = 10) has 14 + 17 = 31, then 26 + 29 = 55."""
import numpy as np
import pytest
import torch

from gnnkeras_amd import CompositeGraphObject
from gnnkeras_amd import _native as nat
from gnnkeras_amd.Models.MLP import MLP
from gnnkeras_amd.Models.CompositeGNN import CompositeGNNnodeBased, CompositeGNNarcBased, CompositeGNNgraphBased
from gnnkeras_amd.Models.CompositeLGNN import CompositeLGNN
from gnnkeras_amd.Models.training import LoopTrainer, Adam
from gnnkeras_amd.Sequencers.GraphSequencers import CompositeMultiGraphSequencer
from gnnkeras_amd.synth import er_composite_graph
from oracle import torch_train
from oracle.harness import rel_err
from test_gpu_training import log_rows
from test_gpu_lgnn_serial import (BAR, MARGIN, mutag_subsets, run_serial_chain, operands, oracle_layer, check_moving, check_relabelled,
                                  moving_of, kernel_name, perturb_bn, snapshot, assert_same)
from test_gpu_lgnn_grouped import spy_on_propagate, _weights

pytestmark = pytest.mark.gpu
GROUPED_TYPES = 'train_step: grouped forward kernels (types)'
ONE_RUN = dict(route='grouped', library_calls=1, runs=1, fallback_graphs=0)
CCLS = {'n': CompositeGNNnodeBased, 'a': CompositeGNNarcBased, 'g': CompositeGNNgraphBased}
DIMS, T, A = (5, 3, 4), 2, 3
MODE = 'composite_average'


def typed_graphs(rng, sizes, seed0, focus='n', absent=None, lonely=None, dims=DIMS):
    """Erdos-Renyi graphs of three node types.  Graph `absent` has its type-2 nodes re-typed to type 0 (a type without a row), graph
    `lonely` keeps exactly one node of type 1 (BatchNormalization over one row: variance 0).  Every graph has an output row."""
    out = []
    for i, n in enumerate(int(v) for v in sizes):
        g = er_composite_graph(n, int(rng.integers(n, 3 * n)), dim_node_label=dims, seed=seed0 + i)
        tm = np.array(g.type_mask, copy=True).reshape(n, len(dims))
        if i == absent:
            mv = tm[:, 2].astype(bool); tm[mv, 0] = True; tm[mv, 2] = False
        if i == lonely:
            mv = np.flatnonzero(tm[:, 1])
            if len(mv) == 0: tm[0, :] = False; tm[0, 1] = True
            else: tm[mv[1:], 0] = True; tm[mv[1:], 1] = False
            assert tm[:, 1].sum() == 1
        rows = g.arcs.shape[0] if focus == 'a' else n
        if focus == 'g': sm, om, n_t = np.ones(n, bool), np.ones(n, bool), 1
        else:
            om, sm = rng.random(rows) < 0.7, rng.random(rows) < 0.8
            om[0] = sm[0] = True
            n_t = int(om.sum())
        out.append(CompositeGraphObject(nodes=g.nodes, arcs=g.arcs, targets=np.eye(T)[rng.integers(0, T, n_t)], type_mask=tm,
                                        dim_node_label=dims, focus=focus, set_mask=sm, output_mask=om, aggregation_mode=MODE))
    return out


def two_sets(focus='n', lo=6, hi=250, seed=17):
    """12 training / 6 validation graphs of 6 .. 250 nodes (<= 256, the group size; some above 64: several tiles per type), one training
    graph with a type absent, one with a type of exactly one row."""
    rng = np.random.default_rng(seed)
    sizes_tr, sizes_va = rng.integers(lo, hi, 12), rng.integers(lo, hi, 6)
    sizes_tr[4] = max(sizes_tr[4], 200)
    sets = [typed_graphs(rng, sizes_tr, 100, focus, absent=1, lonely=2), typed_graphs(rng, sizes_va, 200, focus)]
    n = [g.nodes.shape[0] for s in sets for g in s]
    assert max(n) <= nat.TRAIN_GROUP_MAX_NODES and max(n) > 64
    return sets


def comp_stack(focus, d, n_layers, thr, *, dims=DIMS, arc_dim=A, max_it=5, scale=1.0, bn=True, act='tanh', hidden=None, get_state=True,
               get_output=True):
    """A CompositeLGNN whose networks are sized from the composite input layout itself: network t sees
    [labels[:, :d_t] | state | Adj^T state | aggregated_component] = d_t + 2 S + sum(d_t) + A columns (S = d, or the label width for d = 0),
    the output network the state alone (arc focus: both ends' state and the arc label).  Layer i + 1 sees the ORIGINAL labels widened by
    layer i's state / output.  `hidden`: {type: units} - a hidden layer in that type's state network (layer 0 only)."""
    wrng = np.random.default_rng(19)
    gnns, dl, al = [], np.array(dims), arc_dim
    for layer in range(n_layers):
        S = d if d > 0 else int(dl.max())
        w_comp = int(dl.sum()) + al
        ns = []
        for t, dt in enumerate(dl):
            lay = ([hidden[t]] if (hidden and layer == 0 and t in hidden) else []) + [S]
            n_ = MLP((int(dt) + 2 * S + w_comp,), lay, act, 'lecun_normal', 'lecun_normal', rng=30 + t + 10 * layer, batch_normalization=bn)
            n_.set_weights([a * scale if a.ndim == 2 else a for a in n_.get_weights()])
            ns.append(n_)
        no = MLP((2 * S + al if focus == 'a' else S,), [T], 'softmax', 'glorot_normal', 'glorot_normal', rng=50 + layer, batch_normalization=bn)
        if bn:
            for n_ in ns + [no]: perturb_bn(n_, wrng)
        gnns.append(CCLS[focus](ns, no, d, max_it, thr))
        dl = np.array(dims) + (S if get_state else 0) + (T if get_output and focus != 'a' else 0)
        al = arc_dim + (T if get_output and focus == 'a' else 0)
    return CompositeLGNN(gnns, get_state, get_output)


def grouped_chain(lg, sets, focus, d, tag, covered=None):
    """`run_serial_chain` on the grouped route; every `_propagate` of a covered layer must be ONE run of the *_types kernels."""
    lg.serial_propagation = 'grouped'
    seen = spy_on_propagate(lg)
    rows = run_serial_chain(lg, sets, focus, d, seq_cls=CompositeMultiGraphSequencer, tag=tag)
    assert len(seen) == len(sets) * lg.LAYERS
    for (li, rec, name), n_graphs in zip(seen, [len(s) for _ in range(lg.LAYERS) for s in sets]):
        if covered is None or covered[li]:
            assert rec == ONE_RUN, (tag, li, rec)
            assert name == GROUPED_TYPES, (tag, li, name)
        else:
            assert rec['route'] == 'per_graph' and rec['library_calls'] == n_graphs and name != GROUPED_TYPES, (tag, li, rec, name)
    log_rows(f'{tag} routes', [dict(layer=li, **rec, kernel=name) for li, rec, name in seen])
    return rows, seen


def test_chain_matches_float64_oracle_grouped():
    """Test 1: a 2-layer CompositeLGNN (node focus, state 6, get_state and get_output, threshold 0): the training set, then the validation
    set, both layers grouped - layer 1 has Kc_t up to 52."""
    rows, _ = grouped_chain(comp_stack('n', 6, 2, 0.0), two_sets(), 'n', 6, 'composite_grouped chain')
    assert all(r_['k'] == [5] for r_ in rows)


def test_per_graph_early_exit():
    """Test 2: threshold 0.01 with the state kernels scaled by 0.025: the graphs stop at different k, each exact."""
    rows, _ = grouped_chain(comp_stack('n', 6, 2, 0.01, scale=0.025), two_sets(), 'n', 6, 'composite_grouped early exit')
    assert len(set(k for r_ in rows for k in r_['k'])) > 1


@pytest.mark.parametrize('case', ['arc', 'graph_node_level', 'd0', 'width64'])
def test_foci_and_widths(case):
    """Test 3: arc focus (get_output prepends to the arcs), graph focus at node level, state_vect_dim = 0 (the state is the label matrix),
    a width-64 state (one weight block in LDS, re-loaded per type) with groups of 200+ rows."""
    focus = {'arc': 'a', 'graph_node_level': 'g'}.get(case, 'n')
    d = {'d0': 0, 'width64': 64}.get(case, 6)
    sets = two_sets(focus, hi=120 if case == 'arc' else 250)
    if case == 'width64': assert max(g.nodes.shape[0] for g in sets[0]) >= 200
    layers = 2 if case in ('arc', 'graph_node_level') else 1
    grouped_chain(comp_stack(focus, d, layers, 0.0), sets, focus, d, f'composite_grouped {case}')


def _direct(gnn, graphs, focus, d, tag, s0s=None, **kw):
    """ONE `forward_native(groups=...)` call over the merged graphs = the oracle's per-graph calls concatenated."""
    layer, layer32 = oracle_layer(gnn), oracle_layer(gnn, torch.float32)
    seq1 = CompositeMultiGraphSequencer(list(graphs), focus, MODE, 4, shuffle=False)
    ops_ = operands(seq1, graphs, True)
    want = torch_train.lgnn_serial_propagate(ops_, layer, focus=focus, get_state=True, get_output=True, state0s=s0s)
    want32 = torch_train.lgnn_serial_propagate(ops_, layer32, focus=focus, get_state=True, get_output=True, state0s=s0s)
    if gnn.state_threshold > 0:
        low = [(i, m) for i, m in enumerate(want['margin']) if m < MARGIN]
        assert not low, f'borderline subset (float64 k within {MARGIN} of flipping): {low}'
    S = d if d > 0 else graphs[0].nodes.shape[1]
    x = CompositeMultiGraphSequencer(list(graphs), focus, MODE, len(graphs), shuffle=False)[0][0]
    begin = np.concatenate([[0], np.cumsum([g.nodes.shape[0] for g in graphs])])
    state0 = torch.from_numpy(np.concatenate(s0s)).cuda() if d > 0 else None
    if getattr(gnn, '_trainer', None) is None: gnn._trainer = LoopTrainer(gnn)
    k, state, out = gnn._trainer.forward_native(x, state0=state0, node_level=True, groups=begin, **kw)
    assert kernel_name() == GROUPED_TYPES
    assert [int(v) for v in k.cpu().numpy()] == want['k'], (tag, k, want['k'])
    state, out = state.cpu().numpy(), out.cpu().numpy()
    worst, o0 = 0.0, 0
    for i, g in enumerate(graphs):
        mask = np.logical_and(np.asarray(g.set_mask).reshape(-1), np.asarray(g.output_mask).reshape(-1))
        w_out = (want['arcs'][i][:, :T] if focus == 'a' else want['nodes'][i][:, S:S + T])[mask]
        w32_out = (want32['arcs'][i][:, :T] if focus == 'a' else want32['nodes'][i][:, S:S + T])[mask]
        e32 = max(rel_err(want32['nodes'][i][:, :S], want['nodes'][i][:, :S]), rel_err(w32_out, w_out))
        bar = max(BAR, 2 * e32)
        e = max(rel_err(state[begin[i]:begin[i + 1]], want['nodes'][i][:, :S]), rel_err(out[o0:o0 + int(mask.sum())], w_out))
        o0 += int(mask.sum())
        worst = max(worst, e)
        assert e <= bar, (tag, i, e, bar)
    assert o0 == out.shape[0]
    log_rows(tag, [dict(worst=worst, k=sorted(set(want['k'])))])
    return want


def test_no_batch_normalization():
    """Test 3, BatchNormalization off in all networks: the same kernels with the identity in place of the normalisation."""
    graphs = two_sets()[0]
    rng = np.random.default_rng(5)
    s0s = [rng.normal(0, 0.1, (g.nodes.shape[0], 6)).astype(np.float32) for g in graphs]
    gnn = comp_stack('n', 6, 1, 0.0, bn=False).gnns[0]
    before = _weights(gnn)
    _direct(gnn, graphs, 'n', 6, 'composite_grouped no BatchNormalization', s0s)
    assert all(np.array_equal(a, b) for a, b in zip(before, _weights(gnn)))


def _one_pass(graphs, tag, run_bytes=None):
    """Layer 0 of the early-exit stack over `graphs` in the given order, grouped; the initial states travel with the graphs."""
    lg = comp_stack('n', 6, 2, 0.01, scale=0.025)
    lg.serial_propagation = 'grouped'
    if run_bytes is not None: lg.serial_run_bytes = run_bytes
    gnn = lg.gnns[0]
    layer = oracle_layer(gnn)
    s0s = [np.random.default_rng(1000 + g.nodes.shape[0] + 7 * g.arcs.shape[0]).normal(0, 0.1, (g.nodes.shape[0], 6)).astype(np.float32) for g in graphs]
    seq_now = CompositeMultiGraphSequencer(list(graphs), 'n', MODE, 4, shuffle=True)
    seq_t0 = CompositeMultiGraphSequencer(list(graphs), 'n', MODE, 4, shuffle=True)
    want = torch_train.lgnn_serial_propagate(operands(seq_now, graphs, True), layer, focus='n', get_state=True, get_output=True, state0s=s0s)
    assert min(want['margin']) >= MARGIN, min(want['margin'])
    new_seq, ks = lg._propagate(gnn, seq_now, seq_t0, [torch.from_numpy(s).cuda() for s in s0s])
    assert lg.last_propagate['route'] == 'grouped' and kernel_name() == GROUPED_TYPES
    assert ks == want['k'], (tag, ks, want['k'])
    check_moving(gnn, want, tag)
    return want, [moving_of(n_) for n_ in gnn.net_state] + [moving_of(gnn.net_output)], new_seq.data, ks, dict(lg.last_propagate)


def test_order_and_cuts():
    """Test 4: a smaller workspace cuts the same graphs into several runs - the same k, the moving statistics the same bits; the reversed
    order follows the oracle run in reversed order, moves the statistics elsewhere and leaves every graph's own results bit-identical."""
    graphs = two_sets()[0]
    fwd_want, fwd_mov, fwd_graphs, fwd_k, rec = _one_pass(graphs, 'composite order forward')
    assert rec == ONE_RUN
    _, cut_mov, cut_graphs, cut_k, rec = _one_pass(graphs, 'composite order cut', run_bytes=1)
    assert rec['runs'] > 1 and rec['library_calls'] == rec['runs'] and rec['fallback_graphs'] == 0, rec
    assert cut_k == fwd_k
    for a, b in zip(fwd_mov, cut_mov):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])          # the literal recurrence: the cut does not change a bit
    for a, b in zip(fwd_graphs, cut_graphs): assert np.array_equal(a.nodes, b.nodes)
    rev_want, rev_mov, rev_graphs, rev_k, _ = _one_pass(graphs[::-1], 'composite order reversed')
    pairs64 = list(zip(fwd_want['moving_state'] + [fwd_want['moving_output']], rev_want['moving_state'] + [rev_want['moving_output']]))
    gap64 = max(rel_err(a, b) for f, r in pairs64 for a, b in zip(f, r))
    assert gap64 > 4 * BAR, gap64      # precondition (float64): the order matters by far more than the bar on these graphs
    gap = max(rel_err(a, b) for f, r in zip(fwd_mov, rev_mov) for a, b in zip(f, r))
    assert gap > 2 * BAR, gap
    assert fwd_k == rev_k[::-1] and len(set(fwd_k)) > 1
    for a, b in zip(fwd_graphs, rev_graphs[::-1]):
        assert np.array_equal(a.nodes, b.nodes) and np.array_equal(a.arcs, b.arcs)
    log_rows('composite_grouped order', [dict(gap_float64=gap64, gap_device=gap, runs_cut=rec['runs'])])


def test_a_graph_above_the_group_size_takes_one_call_between_two_runs(monkeypatch):
    """Test 5: a 300-node graph in the middle of the list: two runs and ONE library call for that graph - the composite training-mode
    forward alone is one `gnn_train_step(forward_only)` call - everything within the bars of the oracle."""
    rng = np.random.default_rng(23)
    sizes = [int(v) for v in rng.integers(6, 120, 7)]
    sizes[3] = 300
    sets = [typed_graphs(rng, sizes, 300, 'n', absent=1), typed_graphs(rng, rng.integers(6, 120, 4), 400, 'n')]
    lg = comp_stack('n', 6, 1, 0.0)
    lg.serial_propagation = 'grouped'
    lib = nat.lib()
    calls, real = [], lib.gnn_train_step

    def counting(args):
        calls.append(1)
        return real(args)
    monkeypatch.setattr(lib, 'gnn_train_step', counting)
    seen = spy_on_propagate(lg)
    run_serial_chain(lg, sets, 'n', 6, seq_cls=CompositeMultiGraphSequencer, tag='composite_grouped oversized')
    assert [rec for _, rec, _ in seen] == [dict(route='grouped', library_calls=3, runs=2, fallback_graphs=1), ONE_RUN], seen
    assert seen[0][2] == GROUPED_TYPES               # (the last call of the training set is its second run)
    assert len(calls) == 3 + 1


def test_uncovered_layer_takes_the_per_graph_route():
    """Test 6: a hidden layer in ONE type's state network: the whole layer takes 'per_graph' (one library call per graph, the general
    composite kernels).  The refusal comes before any launch: weights and moving statistics are untouched by it."""
    sets = two_sets(hi=100)
    lg = comp_stack('n', 6, 1, 0.0, hidden={1: 8})
    gnn = lg.gnns[0]
    graphs = sets[0]
    x = CompositeMultiGraphSequencer(list(graphs), 'n', MODE, len(graphs), shuffle=False)[0][0]
    begin = np.concatenate([[0], np.cumsum([g.nodes.shape[0] for g in graphs])])
    gnn._trainer = LoopTrainer(gnn)
    before = _weights(gnn)
    name_before = kernel_name()
    with pytest.raises(NotImplementedError, match='do not cover'):
        gnn._trainer.forward_native(x, node_level=True, groups=begin)
    assert all(np.array_equal(a, b) for a, b in zip(before, _weights(gnn))) and kernel_name() == name_before
    _, seen = grouped_chain(lg, sets, 'n', 6, 'composite_grouped uncovered', covered=[False])
    assert 'general' in seen[0][2], seen[0][2]


@pytest.mark.parametrize('path', ['persistent', 'general', 'row-streaming'])
def test_forward_only_in_one_library_call_equals_the_building_blocks(path, monkeypatch):
    """Test 7: `CompositeGNN*.Loop(training=True)` as ONE `gnn_train_step(forward_only)` call against the same forward on the building
    blocks (`LoopTrainer.forward`): k exact, state / outputs / every network's moving statistics within the bar - on the persistent
    small-graph path (a merged batch), the general path (a hidden layer in one type's state network) and the large-graph path
    (40 000 nodes, 300 000 arcs)."""
    from test_gpu_round6 import composite_nets
    d, K = (64, 4) if path == 'row-streaming' else (6, 4)
    if path == 'row-streaming':
        g = er_composite_graph(40_000, 300_000, dim_node_label=(14, 8, 4), aggregation_mode='average', seed=77 + d, focus='n')
        x = CompositeMultiGraphSequencer([g], 'n', 'average', 1, shuffle=False)[0][0]
        build = lambda: CompositeGNNnodeBased(*composite_nets((14, 8, 4), 3, 2, 'n', d, True, 'selu'), d, K, 0.0)
    else:
        graphs = typed_graphs(np.random.default_rng(31), [20, 90, 33, 8, 140, 61, 17, 45], 500, 'n', absent=1)
        x = CompositeMultiGraphSequencer(graphs, 'n', MODE, len(graphs), shuffle=False)[0][0]
        build = lambda: comp_stack('n', d, 1, 0.0, max_it=K, scale=0.5, hidden={1: 8} if path == 'general' else None).gnns[0]
    a, b = build(), build()
    b._trainer = LoopTrainer(b)
    b._trainer.use_native_step = False
    s0 = torch.from_numpy(np.random.default_rng(5).normal(0, 0.1, (x[0].shape[0], d)).astype(np.float32)).cuda()
    lib = nat.lib()
    calls, real = [], lib.gnn_train_step

    def counting(args):
        calls.append(1)
        return real(args)
    monkeypatch.setattr(lib, 'gnn_train_step', counting)
    rows = []
    for rep in range(2):                                         # twice: the moving statistics carry over
        del calls[:]
        ka, sa, oa = a.Loop(*a.process_inputs(x), training=True, state0=s0, seed=7 + rep)
        name = kernel_name()
        assert len(calls) == 1 and name.startswith('train_step composite') and path in name, (len(calls), name)
        kb, sb, ob = b.Loop(*b.process_inputs(x), training=True, state0=s0, seed=7 + rep)
        assert len(calls) == 1
        assert float(ka) == float(kb) == float(K), (float(ka), float(kb))
        assert tuple(oa.shape) == tuple(ob.shape) and tuple(sa.shape) == tuple(sb.shape)
        es, eo = rel_err(sa.cpu().numpy(), sb.cpu().numpy()), rel_err(oa.cpu().numpy(), ob.cpu().numpy())
        assert es <= BAR and eo <= BAR, (path, rep, es, eo)
        em = 0.0
        for na, nb in zip(list(a.net_state) + [a.net_output], list(b.net_state) + [b.net_output]):
            for wa, wb in zip(moving_of(na), moving_of(nb)): em = max(em, rel_err(wa, wb))
            for wa, wb in zip(na.get_weights(), nb.get_weights()): assert wa.shape == wb.shape
        assert em <= BAR, (path, rep, em)
        rows.append(dict(rep=rep, state=es, out=eo, moving=em, kernel=name))
    log_rows(f'composite forward_only {path}', rows)


def test_reference_composite_mutag_shape():
    """Test 8: the shape of the reference's second starter: the composite MUTAG graphs (one node type), graph focus, state 10,
    selu / softmax with BatchNormalization, 3 layers.  Layers 1 and 2 have Kc = 26 + 29 = 55."""
    from gnnkeras_amd.load_MUTAG import load_composite_graphs
    sets = mutag_subsets(load_composite_graphs())
    for s in sets:
        for g in s: g.setAggregation(MODE)
    assert max(g.nodes.shape[0] for s in sets for g in s) <= nat.TRAIN_GROUP_MAX_NODES
    lg = comp_stack('g', 10, 3, 0.0, dims=(14,), act='selu')
    assert [n_.input_dim for gnn in lg.gnns for n_ in gnn.net_state] == [51, 75, 75]
    grouped_chain(lg, sets, 'g', 10, 'composite_grouped mutag')


def test_fit_grouped_layer_boundaries_match_float64_oracle():
    """Test 9: a serial `CompositeLGNN.fit()` compiled with serial_propagation='grouped' (3 layers, 3 node types, state = labels so the
    oracle needs no drawn initial state, threshold 0, 2 shuffled epochs per layer with validation data): at every layer boundary the graphs
    layer i + 1 is handed - and layer i's moving statistics at that point - are the oracle's propagation of layer i's input graphs with
    the weights layer i's fit() ended with.  Four grouped propagations, one run each."""
    tr_graphs, va_graphs = two_sets(hi=120)
    tr = CompositeMultiGraphSequencer(tr_graphs, 'n', MODE, 4, shuffle=True)
    va = CompositeMultiGraphSequencer(va_graphs, 'n', MODE, 4, shuffle=False)
    caller = [(list(s.data), [snapshot(g) for g in s.data]) for s in (tr, va)]
    lg = comp_stack('n', 0, 3, 0.0)
    lg.compile(optimizer=Adam(0.01), loss='categorical_crossentropy', training_mode='serial', average_st_grads=True, metrics=['accuracy'],
               serial_propagation='grouped')
    assert lg.serial_propagation == 'grouped'
    records, orig_grouped = [], lg._propagate_grouped

    def grouped(*aa, **kk):
        out = orig_grouped(*aa, **kk)
        records.append((out is not None, dict(lg.last_propagate) if out is not None else None, kernel_name()))
        return out
    lg._propagate_grouped = grouped
    A_, B_ = {}, {}
    spec_of = lambda gnn: ([n_.spec() for n_ in gnn.net_state], gnn.net_output.spec())
    for i, gnn in enumerate(lg.gnns):
        def wrapped(seq, *args, _i=i, _fit=gnn.fit, **kwargs):
            B_[_i] = dict(train=[g.copy() for g in seq.data], valid=[g.copy() for g in kwargs['validation_data'].data],
                          prev=spec_of(lg.gnns[_i - 1]) if _i > 0 else None)
            out = _fit(seq, *args, **kwargs)
            A_[_i] = spec_of(lg.gnns[_i])
            return out
        gnn.fit = wrapped
    np.random.seed(3)
    hists = lg.fit(tr, epochs=2, validation_data=va, verbose=0)
    assert len(hists) == 3 and sorted(A_) == sorted(B_) == [0, 1, 2]
    for s, (order, snaps) in zip((tr, va), caller):                 # the caller's sequencers: same graphs, same arrays
        assert len(s.data) == len(order) and all(a is b for a, b in zip(s.data, order))
        for g, snap in zip(s.data, snaps): assert_same(snapshot(g), snap, 'caller graph')
    assert len(records) == 4                                        # two boundaries x (training set, validation set)
    for done, rec, name in records:
        assert done and rec == ONE_RUN and name == GROUPED_TYPES, (done, rec, name)
    rows = []
    for i in range(2):
        layer = torch_train.serial_layer(*A_[i], 0, 5, 0.0)
        got = {}
        for key in ('train', 'valid'):
            ins = B_[i][key]
            t0_in_order = tr_graphs if key == 'train' else va_graphs        # (fit() shuffles its own views: the propagation walks the caller's order)
            seq_in = CompositeMultiGraphSequencer(ins, 'n', MODE, 1, shuffle=False)
            want = torch_train.lgnn_serial_propagate(operands(seq_in, t0_in_order, True), layer, focus='n', get_state=True, get_output=True)
            assert want['k'] == [5] * len(ins)
            outs = B_[i + 1][key]
            assert len(outs) == len(ins)
            plus = ins[0].nodes.shape[1] + 2
            got[key] = check_relabelled(outs, want, [snapshot(g) for g in t0_in_order], plus, 'n', 2, f'composite fit boundary {i} {key}')
        names = [f'state{t}' for t in range(len(DIMS))] + ['output']
        prev = B_[i + 1]['prev']
        refs = want['moving_state'] + [want['moving_output']]
        ends = A_[i][0] + [A_[i][1]]
        for name, (spec, w), ref, (_, w_end) in zip(names, prev[0] + [prev[1]], refs, ends):
            for part, a, b in (('mean', w[2], ref[0]), ('var', w[3], ref[1])):
                e = rel_err(a, b)
                got['moving'] = max(got.get('moving', 0.0), e)
                assert e <= BAR, (f'composite fit boundary {i}', name, part, e)
            assert not np.array_equal(w[2], w_end[2])               # (they moved: the propagation ran in training mode from where fit() left them)
        rows.append(dict(boundary=i, **{f'{k}_nodes': v['nodes'] for k, v in got.items() if isinstance(v, dict)}, moving=got['moving']))
    log_rows('composite_grouped fit', rows)
