"""Training-mode convergence groups (C ABI 10): `Loop(training=True, groups=...)` and the grouped serial LGNN propagation
(`LGNN.serial_propagation = 'grouped'`) against the float64 restatement `oracle.torch_train.lgnn_serial_propagate` - the checks, bars,
subsets and stacks of tests/test_gpu_lgnn_serial.py, taken through `run_serial_chain` unchanged: k exact per graph, merged columns and
moving statistics within rel_err 2e-5 of float64 (a graph on which the float32 oracle itself is further away: twice that distance),
copied data bit for bit.  One workgroup computes one graph and nothing but the moving-average recurrence crosses graphs, so every
per-graph result is independent of where the graph sits in a run: the k margins the existing test asserts carry over.

Coverage of the grouped kernels on the rows of ROWS (constant input columns Kc = 2 L + A for d > 0, A for d = 0, must be <= 32):
    starter / starter_thr0   d = 0, A = 3: all three layers
    g_d8_state               layer 0 (Kc = 31); layer 1 has L = 22: Kc = 47 - falls back
    n_empty_output           both layers (d = 0)
    n_d8_output              layer 0 (Kc = 31); layer 1 has L = 16: Kc = 35 - falls back
    a_prepend                both layers (d = 0; A = 3, then 5)
    a_d8_early               layer 0 (Kc = 31); layer 1 has A = 5: Kc = 33 - falls back
The largest graph of the subsets has 165 nodes (< 256, the library's group size): no graph may take the per-graph call on a covered layer."""
import numpy as np
import pytest
import torch

from gnnkeras_amd import _native as nat
from gnnkeras_amd.Models.MLP import MLP, get_inout_dims
from gnnkeras_amd.Models.LGNN import LGNN
from gnnkeras_amd.Sequencers.GraphSequencers import MultiGraphSequencer
from oracle import torch_train
from oracle.harness import rel_err
from test_gpu_training import log_rows
import test_gpu_lgnn_serial as base
from test_gpu_lgnn_serial import (BAR, MARGIN, CLS, ROWS, serial_stack, mutag_subsets, _refocused, run_serial_chain, operands, oracle_layer,
                                  check_moving, moving_of, kernel_name, perturb_bn)

pytestmark = pytest.mark.gpu
GROUPED = 'train_step: grouped forward kernels'
COVERED = {'starter': [True, True, True], 'starter_thr0': [True, True, True], 'g_d8_state': [True, False], 'n_empty_output': [True, True],
           'n_d8_output': [True, False], 'a_prepend': [True, True], 'a_d8_early': [True, False]}


def spy_on_propagate(lg):
    """Record (layer, route record, kernel name) of every `_propagate` call of `lg`."""
    seen, orig = [], lg._propagate

    def spy(gnn, *a, **k):
        out = orig(gnn, *a, **k)
        seen.append((lg.gnns.index(gnn), dict(lg.last_propagate), kernel_name()))
        return out
    lg._propagate = spy
    return seen


@pytest.mark.parametrize('row', list(ROWS))
def test_grouped_propagate_matches_float64_oracle(mutag_graphs, row):
    """Test 1: every layer of the rows of ROWS (training set, then validation set) on the grouped route."""
    focus, d, get_state, get_output, n_layers, thr, _kernels, empty = ROWS[row]
    tr, va = mutag_subsets(mutag_graphs)
    assert max(g.nodes.shape[0] for g in tr + va) <= nat.TRAIN_GROUP_MAX_NODES and max(g.nodes.shape[0] for g in tr + va) > 64
    rng = np.random.default_rng(11)
    sets_t0 = [_refocused(tr, focus, rng, empty), _refocused(va, focus, rng, False)]
    lg = serial_stack(focus, d, n_layers, get_state, get_output, thr, state_scale=0.01 if thr > 0 else 1.0)
    lg.serial_propagation = 'grouped'
    seen = spy_on_propagate(lg)
    rows = run_serial_chain(lg, sets_t0, focus, d, kernels=None, tag=f'lgnn_grouped {row}')
    assert len(seen) == 2 * n_layers
    for (li, rec, name), n_graphs in zip(seen, [len(s) for _ in range(n_layers) for s in sets_t0]):
        if COVERED[row][li]:
            # one run = one library call, no graph on the per-graph call, and the grouped kernels did the work
            assert rec == dict(route='grouped', library_calls=1, runs=1, fallback_graphs=0), (row, li, rec)
            assert name == GROUPED, (row, li, name)
        else:
            assert rec['route'] == 'per_graph' and rec['library_calls'] == n_graphs and name != GROUPED, (row, li, rec, name)
    log_rows(f'lgnn_grouped {row} routes', [dict(layer=li, fell_back=not COVERED[row][li], **rec, kernel=name) for li, rec, name in seen])
    if row == 'starter': assert len(set(k for r_ in rows for k in r_['k'])) > 1      # per-graph early exit really happens


def _one_pass(graphs, tag):
    """Layer 0 of the starter stack (threshold 0.01) over `graphs` in the given order, grouped: the oracle's answer, the device's
    moving statistics, the relabelled graphs and k."""
    lg = serial_stack('g', 0, 3, True, True, 0.01, state_scale=0.01)
    lg.serial_propagation = 'grouped'
    gnn = lg.gnns[0]
    layer = oracle_layer(gnn)
    seq_now = MultiGraphSequencer(list(graphs), 'g', 'average', 4, shuffle=True)
    seq_t0 = MultiGraphSequencer(list(graphs), 'g', 'average', 4, shuffle=True)
    want = torch_train.lgnn_serial_propagate(operands(seq_now, graphs), layer, focus='g', get_state=True, get_output=True)
    assert min(want['margin']) >= MARGIN
    new_seq, ks = lg._propagate(gnn, seq_now, seq_t0)
    assert lg.last_propagate['route'] == 'grouped' and kernel_name() == GROUPED
    assert ks == want['k'], (tag, ks, want['k'])
    check_moving(gnn, want, tag)
    return want, (moving_of(gnn.net_state), moving_of(gnn.net_output)), new_seq.data, ks


def test_group_order_decides_the_moving_statistics(mutag_graphs):
    """Test 2: the same graphs in reversed order: the moving statistics follow the oracle run in reversed order and differ from the
    forward-order result; k and the relabelled columns of every graph are the same bits in both orders (no arithmetic crosses graphs)."""
    tr, _ = mutag_subsets(mutag_graphs)
    fwd_want, fwd_mov, fwd_graphs, fwd_k = _one_pass(tr, 'order forward')
    rev_want, rev_mov, rev_graphs, rev_k = _one_pass(tr[::-1], 'order reversed')
    # precondition (float64): the order matters by far more than the bar on these graphs
    gap64 = max(rel_err(a, b) for key in ('moving_state', 'moving_output') for a, b in zip(fwd_want[key], rev_want[key]))
    assert gap64 > 4 * BAR, gap64
    gap = max(rel_err(a, b) for f, r in zip(fwd_mov, rev_mov) for a, b in zip(f, r))
    assert gap > 2 * BAR, gap           # (>= gap64 - 2 BAR by the two oracle checks above)
    assert fwd_k == rev_k[::-1]
    for a, b in zip(fwd_graphs, rev_graphs[::-1]):
        assert np.array_equal(a.nodes, b.nodes) and np.array_equal(a.arcs, b.arcs)
    log_rows('lgnn_grouped order', [dict(gap_float64=gap64, gap_device=gap)])


def _single_layer(focus, d, bn, thr):
    """One layer of the serial stack's shape; `bn` False: no BatchNormalization in either network."""
    if bn: return serial_stack(focus, d, 2, True, True, thr, state_scale=0.01 if thr > 0 else 1.0).gnns[0]
    inp, lay = get_inout_dims('state', 14, 3, 2, focus, d, layer=0, get_state=True, get_output=True)
    ns = MLP(inp[0], lay, 'selu', 'lecun_normal', 'lecun_normal', rng=10, batch_normalization=False)
    inp, lay = get_inout_dims('output', 14, 3, 2, focus, d, layer=0, get_state=True, get_output=True)
    no = MLP(inp[0], lay, 'softmax', 'glorot_normal', 'glorot_normal', rng=20, batch_normalization=False)
    return CLS[focus](ns, no, d, 5, thr)


LOOP_CASES = [(f, d, bn, 0.0) for f in 'nag' for d in (0, 8) for bn in (True, False)] + [('g', 0, True, 0.01), ('n', 0, True, 0.01), ('a', 8, True, 0.01)]


@pytest.mark.parametrize('focus,d,bn,thr', LOOP_CASES)
def test_loop_training_groups_matches_per_graph_oracle(mutag_graphs, focus, d, bn, thr):
    """Test 3: ONE `Loop(training=True, groups=...)` call over the merged training subset = the oracle's per-graph calls concatenated."""
    tr, _ = mutag_subsets(mutag_graphs)
    graphs = _refocused(tr, focus, np.random.default_rng(11), False)
    gnn = _single_layer(focus, d, bn, thr)
    layer, layer32 = oracle_layer(gnn), oracle_layer(gnn, torch.float32)
    rng = np.random.default_rng(5)
    s0s = [rng.normal(0, 0.1, (g.nodes.shape[0], d)).astype(np.float32) for g in graphs] if d > 0 else None
    seq1 = MultiGraphSequencer(list(graphs), focus, 'average', 4, shuffle=False)
    ops_ = operands(seq1, graphs)
    want = torch_train.lgnn_serial_propagate(ops_, layer, focus=focus, get_state=True, get_output=True, state0s=s0s)
    want32 = torch_train.lgnn_serial_propagate(ops_, layer32, focus=focus, get_state=True, get_output=True, state0s=s0s)
    if thr > 0:
        low = [(i, m) for i, m in enumerate(want['margin']) if m < MARGIN]
        assert not low, f'borderline subset (float64 k within {MARGIN} of flipping): {low}'
    S, T = (d if d > 0 else 14), 2
    merged = MultiGraphSequencer(list(graphs), focus, 'average', len(graphs), shuffle=False)
    x = merged[0][0]
    begin = np.concatenate([[0], np.cumsum([g.nodes.shape[0] for g in graphs])])
    state0 = torch.from_numpy(np.concatenate(s0s)).cuda() if d > 0 else None
    k, state, out = gnn.Loop(*gnn.process_inputs(x), training=True, groups=begin, state0=state0, node_level=True)
    assert kernel_name() == GROUPED
    assert [int(v) for v in k.cpu().numpy()] == want['k']
    if thr == 0: assert set(want['k']) == {gnn.max_iteration}
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
        assert e <= bar, (i, e, bar)
    assert o0 == out.shape[0]
    if bn: worst = max(worst, check_moving(gnn, want, f'loop groups {focus} d{d}'))
    log_rows(f'loop_groups {focus} d={d} bn={bn} thr={thr}', [dict(worst=worst, k=sorted(set(want['k'])))])


def _weights(gnn):
    nets = (list(gnn.net_state) if isinstance(gnn.net_state, (list, tuple)) else [gnn.net_state]) + [gnn.net_output]
    return [np.array(w, copy=True) for n_ in nets for w in n_.get_weights()]


def test_loop_training_groups_rejects(mutag_graphs):
    """Test 3, the refusals: an arc across a group boundary raises NativeError; a two-layer state network and a composite model raise
    NotImplementedError and leave every weight - the moving statistics among them - bit for bit."""
    tr, _ = mutag_subsets(mutag_graphs)
    graphs = _refocused(tr[:6], 'n', np.random.default_rng(11), False)
    sizes = [g.nodes.shape[0] for g in graphs]
    begin = np.concatenate([[0], np.cumsum(sizes)])
    x = MultiGraphSequencer(list(graphs), 'n', 'average', len(graphs), shuffle=False)[0][0]
    gnn = _single_layer('n', 0, True, 0.0)
    crossing = begin.copy(); crossing[1] += 1                # the first node of graph 1 joins group 0: its arcs leave the group
    with pytest.raises(nat.NativeError, match='leaves its group'):
        gnn.Loop(*gnn.process_inputs(x), training=True, groups=crossing, node_level=True)
    with pytest.raises(ValueError):
        gnn.Loop(*gnn.process_inputs(x), training=True, groups=begin[:-1], node_level=True)      # does not span the nodes
    # two Dense layers in the state network
    inp, lay = get_inout_dims('state', 14, 3, 2, 'n', 0, hidden_units=[20], layer=0, get_state=True, get_output=True)
    ns = MLP(inp[0], lay, 'selu', 'lecun_normal', 'lecun_normal', rng=10, batch_normalization=True)
    inp, lay = get_inout_dims('output', 14, 3, 2, 'n', 0, layer=0, get_state=True, get_output=True)
    no = MLP(inp[0], lay, 'softmax', 'glorot_normal', 'glorot_normal', rng=20, batch_normalization=True)
    wrng = np.random.default_rng(3)
    for n_ in (ns, no): perturb_bn(n_, wrng)
    deep = CLS['n'](ns, no, 0, 5, 0.0)
    before = _weights(deep)
    with pytest.raises(NotImplementedError):
        deep.Loop(*deep.process_inputs(x), training=True, groups=begin, node_level=True)
    assert all(np.array_equal(a, b) for a, b in zip(before, _weights(deep)))
    # a composite model
    from gnnkeras_amd import CompositeGraphObject
    from gnnkeras_amd.Models.CompositeGNN import CompositeGNNnodeBased
    from gnnkeras_amd.Sequencers.GraphSequencers import CompositeMultiGraphSequencer
    from gnnkeras_amd.synth import er_composite_graph
    dims, D, T, A = (5, 3, 4), 6, 2, 3
    cg = []
    for i in range(3):
        g = er_composite_graph(12 + i, 30, dim_node_label=dims, seed=40 + i)
        cg.append(CompositeGraphObject(nodes=g.nodes, arcs=g.arcs, targets=np.eye(T)[np.zeros(12 + i, int)], type_mask=g.type_mask,
                                       dim_node_label=dims, focus='n', set_mask=np.ones(12 + i, bool), output_mask=np.ones(12 + i, bool),
                                       aggregation_mode='composite_average'))
    inp, lay = get_inout_dims('state', dims, A, T, 'n', D)
    cns = [MLP(i, lay, 'tanh', 'lecun_normal', 'lecun_normal', rng=30 + t, batch_normalization=True) for t, i in enumerate(inp)]
    inp, lay = get_inout_dims('output', dims, A, T, 'n', D)
    cno = MLP(inp[0], lay, 'softmax', 'glorot_normal', 'glorot_normal', rng=50, batch_normalization=True)
    for n_ in cns + [cno]: perturb_bn(n_, wrng)
    comp = CompositeGNNnodeBased(cns, cno, D, 4, 0.0)
    cx = CompositeMultiGraphSequencer(cg, 'n', 'composite_average', 3, shuffle=False)[0][0]
    before = _weights(comp)
    with pytest.raises(NotImplementedError):
        comp.Loop(*comp.process_inputs(cx), training=True, groups=[0, 12, 25, 39])
    assert all(np.array_equal(a, b) for a, b in zip(before, _weights(comp)))


def test_fit_grouped_layer_boundaries_match_float64_oracle(mutag_graphs, monkeypatch):
    """Test 4: `fit()` of the starter stack compiled with serial_propagation='grouped', held to the checks of
    test_fit_layer_boundaries_match_float64_oracle at both layer boundaries (that test's body, run on a stack whose compile() selects
    the grouped route)."""
    records, made = [], []
    orig_stack = base.serial_stack

    def stack(*a, **k):
        lg = orig_stack(*a, **k)
        orig_compile, orig_grouped = lg.compile, lg._propagate_grouped
        lg.compile = lambda *aa, **kk: orig_compile(*aa, serial_propagation='grouped', **kk)

        def grouped(*aa, **kk):
            out = orig_grouped(*aa, **kk)
            records.append((out is not None, dict(lg.last_propagate) if out is not None else None, kernel_name()))
            return out
        lg._propagate_grouped = grouped
        made.append(lg)
        return lg
    monkeypatch.setattr(base, 'serial_stack', stack)
    base.test_fit_layer_boundaries_match_float64_oracle(mutag_graphs)
    assert len(made) == 1 and made[0].serial_propagation == 'grouped'
    assert len(records) == 4                                  # two boundaries x (training set, validation set)
    for done, rec, name in records:
        assert done and rec == dict(route='grouped', library_calls=1, runs=1, fallback_graphs=0) and name == GROUPED, (done, rec, name)


def test_no_hidden_fallback_one_library_call_per_run(mutag_graphs, monkeypatch):
    """Test 5: one `_propagate` of the starter row makes ONE gnn_train_step call per run, plus one per graph the library reports as too
    large - and on these subsets (largest graph 165 nodes, group size 256) that second number is 0."""
    tr, _ = mutag_subsets(mutag_graphs)
    graphs = _refocused(tr, 'g', np.random.default_rng(11), False)
    too_large = sum(g.nodes.shape[0] > nat.TRAIN_GROUP_MAX_NODES for g in graphs)
    assert too_large == 0 and nat.TRAIN_GROUP_MAX_NODES >= 256
    lg = serial_stack('g', 0, 3, True, True, 0.01, state_scale=0.01)
    lg.serial_propagation = 'grouped'
    lib = nat.lib()
    calls, real = [], lib.gnn_train_step

    def counting(args):
        calls.append(1)
        return real(args)
    monkeypatch.setattr(lib, 'gnn_train_step', counting)
    seq_now = MultiGraphSequencer(list(graphs), 'g', 'average', 4, shuffle=True)
    seq_t0 = MultiGraphSequencer(list(graphs), 'g', 'average', 4, shuffle=True)
    new_seq, ks = lg._propagate(lg.gnns[0], seq_now, seq_t0)
    assert lg.last_propagate == dict(route='grouped', library_calls=1, runs=1, fallback_graphs=0)
    assert len(calls) == 1 + too_large and len(ks) == len(graphs) and kernel_name() == GROUPED
    # a smaller workspace cuts the same graphs into several runs: one call each, same k
    lg2 = serial_stack('g', 0, 3, True, True, 0.01, state_scale=0.01)
    lg2.serial_propagation, lg2.serial_run_bytes = 'grouped', 1
    del calls[:]
    _, ks2 = lg2._propagate(lg2.gnns[0], MultiGraphSequencer(list(graphs), 'g', 'average', 4, shuffle=True),
                            MultiGraphSequencer(list(graphs), 'g', 'average', 4, shuffle=True))
    assert lg2.last_propagate['runs'] > 1 and len(calls) == lg2.last_propagate['runs'] and lg2.last_propagate['fallback_graphs'] == 0
    assert ks2 == ks
    for part, a, b in zip('mvmv', moving_of(lg.gnns[0].net_state) + moving_of(lg.gnns[0].net_output),
                          moving_of(lg2.gnns[0].net_state) + moving_of(lg2.gnns[0].net_output)):
        assert np.array_equal(a, b), part            # the literal recurrence: the cut into runs does not change a bit
