"""Dropout / AlphaDropout in FRONT of the first Dense (position 0, reference MLP.py:58-71 with dropout_pos = 0) inside `gnn_train_step`
(gnnkeras_amd/csrc/kernels_train_front.hpp, train_loop.hpp; opt-in: `model.native_flags |= nat.FLAG_TRAIN_DROPOUT_FRONT`): the step and
the training-mode forward of a homogeneous model with such a layer in its state and / or output network run inside the library, on the
general kernels, with the masks the building blocks draw.  Every test carries the flag and asserts through `gnn_last_kernel_name()`
that the route ran (without the feature the step silently takes the building blocks); the oracle tests compare against the float64
autograd oracle fed the same masks (oracle/torch_train.py) at the bars of tests/test_gpu_training.py - `BARS` per tensor with the counted
kink allowance, `Y_PRED_BAR`, loss within 1e-5, k exact, moving statistics within 1e-5 (all inside `check_step`).

The rule (one layer at position 0 per network, homogeneous, whole calls) is pinned on the host by tests/test_train_dropout_front_plan_host.py."""
import numpy as np
import pytest
import torch

from gnnkeras_amd import GraphObject
from gnnkeras_amd import _native as nat
from gnnkeras_amd.Models.GNN import GNNgraphBased
from gnnkeras_amd.Models.LGNN import LGNN
from gnnkeras_amd.Models.MLP import MLP, get_inout_dims
from gnnkeras_amd.Models.training import SGD, LoopTrainer
from gnnkeras_amd.Sequencers.GraphSequencers import MultiGraphSequencer
from gnnkeras_amd.synth import er_graph
from test_gpu_training import CLS, Y_PRED_BAR, check_step, nets, refocus
from test_gpu_train_hidden_small import names_of_steps, small_graphs
from test_gpu_train_dropout_small import _predicate_ratios, close_to_the_other_route, grads_of, last_name

pytestmark = pytest.mark.gpu
FRONT = nat.FLAG_TRAIN_DROPOUT_FRONT
FRONT_NAME = 'train_step: general kernels (dropout in front)'


def front_nets(focus, d, bn, state=(0.2,), state_pos=(0,), out=None, alpha=False, **kw):
    """`nets` of tests/test_gpu_training.py with Dropout (AlphaDropout: `alpha`) layers of the rates `state` at the positions `state_pos` of
    the state network (None: none) and one of rate `out` at position 0 of the output network (None: none)."""
    ns, no = nets(focus, d, bn, **kw)
    if state is not None: ns.dropout_rate, ns.dropout_pos, ns.alphadropout = list(state), list(state_pos), alpha
    if out is not None: no.dropout_rate, no.dropout_pos, no.alphadropout = [out], [0], alpha
    return ns, no


def flagged_step(model, x, y, sw, s0, seed=5, **kw):
    """`check_step` on the in-library step (the oracle comparison at the project's bars, the oracle fed the masks of `seed`) with the
    flag set, and which kernels ran."""
    model.native_flags = FRONT
    out = check_step(model, x, y, sw, s0, native=True, seed=seed, **kw)
    assert last_name() == FRONT_NAME, last_name()
    return out


def state0(rng, x, d):
    return rng.normal(0, 0.1, (x[0].shape[0], d)).astype(np.float32) if d > 0 else None


# ---- 1. one row ---------------------------------------------------------------------------------------------------------------------------------
def test_one_output_row(mutag_graphs):
    """A single graph whose set_mask & output_mask leaves ONE node: the output network - Dropout 0.3 in front of its Dense - sees one row
    (one wave's first lanes, one row chunk).  Node focus, no layer in the state network.  (No BatchNormalization: the statistics of one
    row normalise it to beta and its input gradient to exactly nothing.)"""
    g = mutag_graphs[0]
    n = g.nodes.shape[0]
    om = np.zeros(n, dtype=bool); om[n // 2] = True
    one = GraphObject(nodes=g.nodes, arcs=g.arcs, targets=np.array([[0.0, 1.0]]), focus='n', set_mask=np.ones(n, dtype=bool), output_mask=om)
    x, y, sw = MultiGraphSequencer([one], 'n', 'average', 1, shuffle=False)[0]
    rng = np.random.default_rng(31)
    ns, no = front_nets('n', 8, False, state=None, out=0.3, act='tanh')
    res, want = flagged_step(CLS['n'](ns, no, 8, 3, 0.0), x, y, sw, state0(rng, x, 8))
    assert want['y_pred'].shape[0] == 1 and res['k'] == 3


# ---- 2. odd widths, every focus -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('focus,bn,alpha', [('g', True, False), ('n', False, False), ('a', True, True), ('n', True, False)])
def test_odd_widths(mutag_graphs, focus, bn, alpha):
    """The configurations of test_dropout_in_front_of_the_first_dense (tests/test_gpu_training.py), on the flag's route: d = 5 - 41 input
    columns, no multiple of 4 or 16, the label segments 14 wide - ten graphs, layers at positions 0 and 1 of a [8, 5] state network and at
    position 0 of the output network (arc focus: both end nodes' segments and the arc labels), 3 iterations."""
    rng = np.random.default_rng(21)
    gl = refocus([g.copy() for g in mutag_graphs[:10]], focus, rng)
    x, y, sw = MultiGraphSequencer(gl, focus, 'average', 10, shuffle=False)[0]
    d = 5
    inp, lay = get_inout_dims('state', 14, 3, 2, focus, d, hidden_units=[8])
    ns = MLP(inp[0], lay, ['selu' if alpha else 'tanh', 'tanh'], 'lecun_normal', 'lecun_normal', dropout_rate=[0.2, 0.1], dropout_pos=[0, 1],
             alphadropout=alpha, batch_normalization=bn, rng=0)
    assert ns.input_dim == 41
    inp, lay = get_inout_dims('output', 14, 3, 2, focus, d)
    no = MLP(inp[0], lay, 'softmax', 'glorot_normal', 'glorot_normal', dropout_rate=0.15, dropout_pos=0, alphadropout=alpha,
             batch_normalization=bn, rng=1)
    if bn:
        r2 = np.random.default_rng(3)
        for n in (ns, no):
            w = n.get_weights()
            w[0] = r2.uniform(0.7, 1.3, w[0].shape).astype(np.float32); w[1] = r2.normal(0, 0.2, w[1].shape).astype(np.float32)
            n.set_weights(w)
    res, want = flagged_step(CLS[focus](ns, no, d, 3, 0.0), x, y, sw, state0(rng, x, d))
    assert res['k'] == 3


# ---- 3. d = 0 ---------------------------------------------------------------------------------------------------------------------------------------
def test_state_dim_0_sum_aggregation(mutag_graphs):
    """The state is the 14 label columns, the segments are [state | agg | arcs] (31 columns, no label segments); 'sum' aggregation,
    BatchNormalization, Dropout 0.3 in front of both networks."""
    x, y, sw = MultiGraphSequencer(mutag_graphs[:16], 'g', 'sum', 16, shuffle=False)[0]
    ns, no = front_nets('g', 0, True, state=(0.3,), out=0.3, act='tanh', scale=0.2)
    assert ns.input_dim == 31
    res, want = flagged_step(GNNgraphBased(ns, no, 0, 4, 0.0), x, y, sw, None)
    assert res['k'] == 4


# ---- 4. a thin first layer ---------------------------------------------------------------------------------------------------------------------------
def test_thin_first_layers(mutag_graphs):
    """Dense 0 of the state network has 3 units, Dense 0 of the output network 2: both take the thin-dense kernel - over X0, with the raw
    weights (without the layer a thin first layer behind BatchNormalization takes a centred fold)."""
    rng = np.random.default_rng(41)
    gl = refocus([g.copy() for g in mutag_graphs[:12]], 'n', rng)
    x, y, sw = MultiGraphSequencer(gl, 'n', 'average', 12, shuffle=False)[0]
    ns, no = front_nets('n', 6, True, state=(0.2,), out=0.2, hidden_state=[3], act='tanh')
    assert list(ns.units) == [3, 6] and list(no.units) == [2]
    res, want = flagged_step(CLS['n'](ns, no, 6, 3, 0.0), x, y, sw, state0(rng, x, 6))
    assert res['k'] == 3


# ---- 5. more than one row chunk ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_nodes,n_arcs,chunks', [(65, 400, 2), (2113, 8000, 34)])
def test_several_row_chunks(n_nodes, n_arcs, chunks):
    """One Erdos-Renyi graph, node focus, every node an output row: the rows of both networks' calls fall into `chunks` chunks of 64
    (rows_per_chunk_for: 65 rows = 2 chunks, the second of ONE row; 2113 rows = 34 chunks, the second of one row again) - up to 32 chunks
    net_backward sums the weight-gradient partials inside the parameter-gradient kernel, beyond that in a reduction launch of their own, and
    the column partials of the layer's backward launch meet in quarters of the chunks.  d = 16, 2 iterations, BatchNormalization."""
    assert -(-n_nodes // 64) == chunks
    g = er_graph(n_nodes, n_arcs, focus='n', aggregation_mode='average', seed=77)
    x, y, sw = MultiGraphSequencer([g], 'n', 'average', 1, shuffle=False)[0]
    ns, no = front_nets('n', 16, True, state=(0.2,), out=0.2, hidden_state=[12], act='tanh', scale=0.3)
    s0 = np.random.default_rng(8).normal(0, 0.1, (n_nodes, 16)).astype(np.float32)
    res, want = flagged_step(CLS['n'](ns, no, 16, 2, 0.0), x, y, sw, s0)
    assert res['k'] == 2


# ---- 6. one iteration -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bn', [False, True])
def test_max_iteration_1(mutag_graphs, bn):
    """No earlier iteration to back-propagate into: the layer's backward launch leaves its column partials, no input gradient."""
    rng = np.random.default_rng(51)
    x, y, sw = MultiGraphSequencer(mutag_graphs[:8], 'g', 'average', 8, shuffle=False)[0]
    ns, no = front_nets('g', 8, bn, state=(0.2,), out=0.1, act='tanh')
    res, want = flagged_step(GNNgraphBased(ns, no, 8, 1, 0.0), x, y, sw, state0(rng, x, 8))
    assert res['k'] == 1


# ---- 7. early exit -------------------------------------------------------------------------------------------------------------------------------------------
EXIT = dict(d=12, H=16, rate=0.05, scale=0.1, threshold=0.12, seed=5, max_it=30)      # chosen on the CPU with the float64 oracle (its k: 4): see the test


def test_early_exit(mutag_graphs):
    """The loop stops on its own.  Fresh masks in front of the first Dense keep every node's state moving from iteration to iteration, so
    the threshold is of the size of that movement; Dropout rate, weight scale and threshold (`EXIT`) were chosen with the float64 oracle
    so that its k is strictly between 1 and max_iteration and no node's ratio at any executed evaluation of the condition lies within 1e-3
    (relative) of the threshold - float32 cannot flip k; both are asserted here before the kernels run.  k must then be exact (the gate
    words skip the launches of the iterations behind it: the moving statistics - checked - move k times), and `average_st_grads` divides
    every gradient of the state network by that k."""
    c = EXIT
    x, y, sw = MultiGraphSequencer(small_graphs(mutag_graphs, 24), 'g', 'average', 24, shuffle=False)[0]
    ns, no = front_nets('g', c['d'], True, state=(c['rate'],), out=0.1, hidden_state=[c['H']], hidden_out=[7], act='tanh', scale=c['scale'])
    s0 = np.random.default_rng(6).normal(0, 0.1, (x[0].shape[0], c['d'])).astype(np.float32)
    ratios = _predicate_ratios(ns, x, s0, c['seed'], c['max_it'])
    k_want = next(t for t, r in enumerate(ratios) if not (r > c['threshold']).any())
    executed = np.concatenate(ratios[:k_want + 1])
    margin = float(np.min(np.abs(executed / c['threshold'] - 1.0)))
    print(f'oracle k {k_want}, closest ratio to the threshold: {margin:.3e} relative')
    assert 1 < k_want < c['max_it'] and margin > 1e-3
    res, want = flagged_step(GNNgraphBased(ns, no, c['d'], c['max_it'], c['threshold']), x, y, sw, s0, seed=c['seed'], avg=True)
    assert want['k'] == k_want and res['k'] == want['k']


# ---- 8. mean squared error behind a sigmoid head ------------------------------------------------------------------------------------------------------------
def test_mse_behind_a_sigmoid_head_with_averaged_state_gradients(mutag_graphs):
    rng = np.random.default_rng(61)
    x, y, sw = MultiGraphSequencer(mutag_graphs[:16], 'g', 'average', 16, shuffle=False)[0]
    ns, no = front_nets('g', 8, True, state=(0.2,), out=0.2, act='tanh', out_act='sigmoid')
    res, want = flagged_step(GNNgraphBased(ns, no, 8, 4, 0.0), x, y, sw, state0(rng, x, 8), loss='mse', avg=True)
    assert res['k'] == 4


# ---- 9. the switch, the masks, repeatability ----------------------------------------------------------------------------------------------------------------
def test_the_switch_the_masks_and_repeatability(mutag_graphs, monkeypatch):
    """Without the flag the building blocks run the step; with it the same seed draws the same masks (k, loss and every gradient of the two
    routes agree as two float32 results that each keep a bar: 2 x BARS['kernel']); another seed draws others; the same seed twice gives
    the same bits (no atomics anywhere on the route: node focus, every output row its own node)."""
    rng = np.random.default_rng(9)
    gl = refocus(small_graphs(mutag_graphs, 16), 'n', rng)
    x, y, sw = MultiGraphSequencer(gl, 'n', 'average', 16, shuffle=False)[0]
    s0 = torch.from_numpy(rng.normal(0, 0.1, (x[0].shape[0], 16)).astype(np.float32)).cuda()

    def step(flags, seed):
        ns, no = front_nets('n', 16, True, state=(0.2, 0.1), state_pos=(0, 1), out=0.15, hidden_state=[12], act='tanh')
        m = CLS['n'](ns, no, 16, 4, 0.0)
        m.compile(optimizer=SGD(0.0), loss='categorical_crossentropy')
        m.native_flags = flags
        tr = LoopTrainer(m)
        with names_of_steps(monkeypatch) as spy:
            res = tr.train_step(x, y, sw, state0=s0, apply=False, seed=seed)
        torch.cuda.synchronize()
        return spy.names, int(res['k']), float(res['loss']), grads_of(tr)

    off = step(0, 3)
    assert off[0] == [], off[0]                                        # the building blocks: no library step at all
    on = step(FRONT, 3)
    assert on[0] == [FRONT_NAME], on[0]
    assert on[1] == off[1] == 4
    assert abs(on[2] - off[2]) <= 2e-5 * max(1.0, abs(off[2])), (on[2], off[2])
    print('worst gradient entry against the building blocks:', close_to_the_other_route(on[3], off[3]))
    other, again = step(FRONT, 4), step(FRONT, 3)
    assert other[0] == again[0] == [FRONT_NAME]
    assert abs(other[2] - on[2]) > 1e-7
    assert any(float(np.max(np.abs(u - v))) > 1e-3 * float(np.max(np.abs(v))) for a, b in zip(other[3], on[3]) for u, v in zip(a, b))
    assert again[2] == on[2]
    for a, b in zip(again[3], on[3]):
        for u, v in zip(a, b): assert np.array_equal(u, v)


# ---- 10. the training-mode forward alone ------------------------------------------------------------------------------------------------------------------------
def test_loop_training_is_one_library_call(mutag_graphs, monkeypatch):
    """`Loop(..., training=True)` with the flag: ONE `gnn_train_step(forward_only)` call on the route, against the building-block forward
    of a twin without the flag at the same seed - k, the state and the output rows at Y_PRED_BAR, and both networks' moving statistics,
    which moved k times (state network) and once (output network); twice: they carry over."""
    gs = small_graphs(mutag_graphs, 8)
    x = MultiGraphSequencer(gs, 'g', 'average', 8, shuffle=False)[0][0]

    def build(flags):
        ns, no = front_nets('g', 16, True, state=(0.2,), out=0.15, act='tanh')
        m = GNNgraphBased(ns, no, 16, 4, 0.0)
        m.native_flags = flags
        return m
    a, b = build(FRONT), build(0)
    first = [w.copy() for w in a.net_state.get_weights()[2:4]]
    s0 = torch.from_numpy(np.random.default_rng(5).normal(0, 0.1, (x[0].shape[0], 16)).astype(np.float32)).cuda()
    rel = lambda u, v: float((u - v).abs().max() / v.abs().max().clamp(min=1e-30))
    for rep in range(2):
        with names_of_steps(monkeypatch) as spy:
            ka, sa, oa = a.Loop(*a.process_inputs(x), training=True, state0=s0, seed=7 + rep)
        assert spy.names == [FRONT_NAME], spy.names
        with names_of_steps(monkeypatch) as spy:
            kb, sb, ob = b.Loop(*b.process_inputs(x), training=True, state0=s0, seed=7 + rep)
        assert spy.names == [], spy.names                              # the building blocks
        assert float(ka) == float(kb) == 4.0, (float(ka), float(kb))
        assert rel(sa, sb) <= Y_PRED_BAR and rel(oa, ob) <= Y_PRED_BAR, (rep, rel(sa, sb), rel(oa, ob))
        for na, nb in ((a.net_state, b.net_state), (a.net_output, b.net_output)):
            for wa, wb in zip(na.get_weights()[2:4], nb.get_weights()[2:4]):
                assert float(np.max(np.abs(wa - wb))) <= 1e-5 * float(np.max(np.abs(wb))), rep
    assert all(float(np.max(np.abs(u - v))) > 1e-4 for u, v in zip(first, a.net_state.get_weights()[2:4]))


# ---- 11. fit() -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_fit_starter_shape(mutag_graphs, monkeypatch):
    """Two epochs of fit() with Adam over 32 graphs in one batch, the starter shape (d = 0: nothing is drawn but the masks), the flag
    set: every step on the route, finite losses, and the first step's loss equal to the one the building blocks compute from the same
    weights with the same masks (the same model object: the masks of an unseeded step derive from the model and its step counter).
    Inference afterwards ignores the layers, as Keras does."""
    seq = MultiGraphSequencer([g.copy() for g in mutag_graphs[:32]], 'g', 'average', 32, shuffle=False)
    assert len(seq) == 1
    ns, no = front_nets('g', 0, True, state=(0.2,), out=0.2, act='tanh', scale=0.2)
    m = GNNgraphBased(ns, no, 0, 5, 0.001)
    start = [ns.get_weights(), no.get_weights()]

    def fit(flags, epochs):
        ns.set_weights(start[0]); no.set_weights(start[1])
        m.compile(optimizer='adam', loss='categorical_crossentropy')
        m.native_flags, m._dropout_step, m._trainer = flags, 0, None
        with names_of_steps(monkeypatch) as spy:
            h = m.fit(seq, epochs=epochs, verbose=0)
        return spy.names, [float(v) for v in h['loss']]

    names_off, loss_off = fit(0, 1)
    assert names_off == [], names_off                                  # the building blocks
    names_on, loss_on = fit(FRONT, 2)
    assert names_on == [FRONT_NAME] * 2, names_on
    assert all(np.isfinite(loss_on)) and abs(loss_on[0] - loss_off[0]) <= 1e-5 * max(1.0, abs(loss_off[0])), (loss_on, loss_off)
    x = seq[0][0]
    out = m(x)
    assert out.shape == (32, 2) and bool(torch.isfinite(out).all()) and torch.equal(out, m(x))


# ---- 12. serial LGNN propagation ------------------------------------------------------------------------------------------------------------------------------------------
def test_lgnn_serial_propagation_takes_the_library_call(mutag_graphs, monkeypatch):
    """A two-layer stack, the flag on every layer, training_mode='serial': what fit() runs between its layers - the training-mode forward
    of the first layer on every single graph - is one library call per graph on the route, and the relabelled graphs equal those of
    the flag-off propagation (the building blocks; the same layer object from the same moving statistics and step counter: the same
    masks) within 1e-5."""
    gl = [g.copy() for g in mutag_graphs[:6]]
    d = 6
    gnns = []
    for i in range(2):
        inp, lay = get_inout_dims('state', 14, 3, 2, 'g', d, layer=i, get_state=True, get_output=True)
        ns = MLP(inp[0], lay, 'tanh', 'lecun_normal', 'lecun_normal', rng=10 + i, batch_normalization=True, dropout_rate=[0.2], dropout_pos=[0])
        ns.set_weights([a * 0.5 if a.ndim == 2 else a for a in ns.get_weights()])
        inp, lay = get_inout_dims('output', 14, 3, 2, 'g', d, layer=i, get_state=True, get_output=True)
        no = MLP(inp[0], lay, 'softmax', 'glorot_normal', 'glorot_normal', rng=20 + i, batch_normalization=True, dropout_rate=[0.1], dropout_pos=[0])
        gnns.append(GNNgraphBased(ns, no, d, 3, 0.0))
    lg = LGNN(gnns, True, True)
    lg.compile(optimizer=SGD(0.0), loss='categorical_crossentropy', training_mode='serial')
    gnn = lg.gnns[0]
    start = [gnn.net_state.get_weights(), gnn.net_output.get_weights()]
    s0s = [torch.from_numpy(np.random.default_rng(70 + i).normal(0, 0.1, (g.nodes.shape[0], d)).astype(np.float32)).cuda() for i, g in enumerate(gl)]

    def propagate(flags):
        gnn.net_state.set_weights(start[0]); gnn.net_output.set_weights(start[1])
        for g_ in lg.gnns: g_.native_flags = flags
        gnn._dropout_step = 0
        seq_now, seq_t0 = (MultiGraphSequencer([g.copy() for g in gl], 'g', 'average', 1, shuffle=False) for _ in range(2))
        with names_of_steps(monkeypatch) as spy:
            new_seq, ks = lg._propagate(gnn, seq_now, seq_t0, s0s)
        return spy.names, ks, [np.asarray(g.nodes, dtype=np.float64).copy() for g in new_seq.data]

    names_off, ks_off, nodes_off = propagate(0)
    assert names_off == [], names_off                                  # the building blocks
    names_on, ks_on, nodes_on = propagate(FRONT)
    assert names_on == [FRONT_NAME] * len(gl), names_on
    assert ks_on == ks_off == [3] * len(gl)
    for u, v in zip(nodes_on, nodes_off):
        assert u.shape == v.shape and u.shape[1] == 14 + d + 2
        assert float(np.max(np.abs(u - v))) <= 1e-5 * max(1.0, float(np.max(np.abs(v))))
