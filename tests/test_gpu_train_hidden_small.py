"""The hidden-layer form of the persistent small-graph training kernels (gnnkeras_amd/csrc/kernels_train_small.hpp, HID instantiations;
opt-in: `model.native_flags |= nat.FLAG_TRAIN_HIDDEN_SMALL`): a state network Dense(H) - Dense(state width) trains with all iterations
of a sweep in one launch.  Every test carries the flag, asserts through `gnn_last_kernel_name()` that the hidden form ran, and compares
against the float64 autograd oracle (oracle/torch_train.py) at the bars of tests/test_gpu_training.py: `BARS` per tensor with the counted
kink allowance, `Y_PRED_BAR`, loss within 1e-5, k exact, moving statistics within 1e-5 (all inside `check_step`); both gradients of the
second Dense layer are among the tensors (`check_step` walks every kernel and bias of the network).  MUTAG-sized inputs.

The hidden form ships for the padded state widths 16 and 32 (at 64 the backward kernel does not fit the register file): a state of
33 .. 64 columns keeps the general kernels with the flag set - tests/test_train_hidden_plan_host.py pins that side of the rule."""
import numpy as np
import pytest
import torch

from gnnkeras_amd import _native as nat
from gnnkeras_amd.Models.GNN import GNNgraphBased
from gnnkeras_amd.Models.LGNN import LGNN
from gnnkeras_amd.Models.MLP import MLP, get_inout_dims
from gnnkeras_amd.Models.training import Adam, SGD, LoopTrainer
from gnnkeras_amd.Sequencers.GraphSequencers import MultiGraphSequencer
from gnnkeras_amd.synth import er_graph
from oracle import torch_train
from oracle.harness import _np, _triple
from test_gpu_training import BARS, CLS, check_network_grads, check_step, nets, refocus
from test_gpu_joint_step import LABEL_BAR, _close, _everything, _label_oracle, batch, stack

pytestmark = pytest.mark.gpu
HIDDEN = 'train_step: persistent small-graph kernels (hidden layer)'
GENERAL = 'train_step: general kernels'
ONE_LAYER = 'train_step: persistent small-graph kernels'


def last_name():
    return nat.lib().gnn_last_kernel_name().decode()


def small_graphs(mutag_graphs, n):
    """The first n graphs of at most 64 nodes (the data set has graphs of up to 417): a merged batch of them is cut into tiles at graph boundaries."""
    return [g.copy() for g in [g for g in mutag_graphs if g.nodes.shape[0] <= 64][:n]]


def flagged_step(model, x, y, sw, s0, flag=True, name=HIDDEN, **kw):
    """`check_step` on the in-library step (the oracle comparison at the project's bars) with the flag set, and which kernels ran."""
    model.native_flags = nat.FLAG_TRAIN_HIDDEN_SMALL if flag else 0
    out = check_step(model, x, y, sw, s0, native=True, **kw)
    assert last_name() == name, last_name()
    return out


class names_of_steps:
    """Records `gnn_last_kernel_name()` behind every `gnn_train_step` / `gnn_train_step_ex` call inside the block."""
    def __init__(self, monkeypatch):
        self.names, self.mp = [], monkeypatch

    def __enter__(self):
        lib = nat.lib()
        for fn in ('gnn_train_step', 'gnn_train_step_ex'):
            orig = getattr(lib, fn)
            def wrapped(*a, _orig=orig):
                rc = _orig(*a)
                self.names.append(last_name())
                return rc
            self.mp.setattr(lib, fn, wrapped, raising=False)
        return self

    def __exit__(self, *exc):
        self.mp.undo()
        return False


# ---- 1. LOCAL form, one tile ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bn', [False, True])
@pytest.mark.parametrize('max_it', [1, 6])
def test_one_tile(mutag_graphs, bn, max_it):
    """Three graphs, at most 64 nodes together: one workgroup, no partner at any barrier.  d = 16, H = 16, tanh / tanh."""
    gl = [g for g in small_graphs(mutag_graphs, 40) if g.nodes.shape[0] <= 20][:3]
    assert len(gl) == 3 and sum(g.nodes.shape[0] for g in gl) <= 64
    x, y, sw = MultiGraphSequencer(gl, 'g', 'average', 3, shuffle=False)[0]
    ns, no = nets('g', 16, bn, hidden_state=[16], act='tanh')
    s0 = np.random.default_rng(21).normal(0, 0.1, (x[0].shape[0], 16)).astype(np.float32)
    flagged_step(GNNgraphBased(ns, no, 16, max_it, 0.0), x, y, sw, s0)
    assert x[5].matrix.tiles(64) is not None and len(x[5].matrix.tiles(64)) == 2


# ---- 2. LOCAL form, several tiles -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('focus,bn,d,H,act,mode,loss', [
    ('g', True, 32, 20, 'relu', 'average', 'categorical_crossentropy'),          # a padded hidden width (20 of 32), SQ = 2
    ('n', False, 32, 20, 'selu', 'average', 'categorical_crossentropy'),
    ('a', True, 32, 20, 'tanh', 'average', 'categorical_crossentropy'),
    ('g', True, 0, 9, 'tanh', 'average', 'categorical_crossentropy'),            # state = the 14 label columns, 9 hidden: both padded, SQ = 1
    ('n', False, 0, 9, 'selu', 'average', 'categorical_crossentropy'),
    ('a', True, 0, 14, 'relu', 'sum', 'categorical_crossentropy'),
    ('n', True, 20, 32, 'tanh', 'average', 'categorical_crossentropy'),          # a padded state (20 of 32) under a full hidden width
    ('g', True, 32, 32, 'selu', 'normalized', 'categorical_crossentropy'),       # per-ARC weights: the HAS_W instantiations
    ('n', False, 16, 12, 'tanh', 'normalized', 'categorical_crossentropy'),
    ('g', True, 16, 16, 'tanh', 'average', 'mse'),                               # mean squared error behind a sigmoid head
])
def test_several_tiles(mutag_graphs, focus, bn, d, H, act, mode, loss):
    """16 graphs in tiles cut at graph boundaries (the state never leaves LDS; the tiles meet for the BatchNorm statistics and the loop
    condition).  The state layer keeps the network's activation (selu / relu kinks are counted by the oracle)."""
    rng = np.random.default_rng(50 + d + H)
    gl = refocus(small_graphs(mutag_graphs, 16), focus, rng)
    x, y, sw = MultiGraphSequencer(gl, focus, mode, 16, shuffle=False)[0]
    assert x[5].matrix.tiles(64) is not None and len(x[5].matrix.tiles(64)) > 2
    ns, no = nets(focus, d, bn, hidden_state=[H], act=act, out_act='sigmoid' if loss == 'mse' else 'softmax', scale=0.2 if mode == 'sum' else 0.5)
    s0 = rng.normal(0, 0.1, (x[0].shape[0], d)).astype(np.float32) if d > 0 else None
    flagged_step(CLS[focus](ns, no, d, 5, 0.0), x, y, sw, s0, loss=loss)


# ---- 3. early exit, gradients averaged over k ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bn', [False, True])
def test_early_exit_and_average(mutag_graphs, bn):
    """The loop stops on its own (the float64 oracle: k = 3 without, 13 with BatchNormalization): the backward sweep runs k iterations and
    `average_st_grads` divides every gradient of the state network, the second layer's included."""
    x, y, sw = MultiGraphSequencer(small_graphs(mutag_graphs, 24), 'g', 'average', 24, shuffle=False)[0]
    ns, no = nets('g', 12, bn, hidden_state=[16], hidden_out=[7], act='tanh', scale=0.25)
    s0 = np.random.default_rng(6).normal(0, 0.1, (x[0].shape[0], 12)).astype(np.float32)
    res, want = flagged_step(GNNgraphBased(ns, no, 12, 30, 0.02), x, y, sw, s0, avg=True)
    assert 1 < want['k'] < 30 and res['k'] == want['k']


# ---- 4. general form: arcs cross tiles ---------------------------------------------------------------------------------------------------------
def test_general_form_on_one_connected_graph():
    """One Erdos-Renyi graph of 150 nodes and 3 000 arcs (mean in-degree 20: rows beyond 16 arcs take the gather's tail loop): three tiles
    of 64 / 64 / 22 consecutive nodes, neighbour rows exchanged through memory behind the second barrier."""
    g = er_graph(150, 3000, focus='n', aggregation_mode='average', seed=77)
    x, y, sw = MultiGraphSequencer([g], 'n', 'average', 1, shuffle=False)[0]
    assert x[5].matrix.tiles(64) is None
    deg = np.bincount(_np(x[1])[:, 1].astype(np.int64), minlength=150)
    assert deg.max() > 16 and deg.min() >= 1
    ns, no = nets('n', 32, True, hidden_state=[32], act='tanh', scale=0.3)
    s0 = np.random.default_rng(8).normal(0, 0.1, (150, 32)).astype(np.float32)
    flagged_step(CLS['n'](ns, no, 32, 5, 0.0), x, y, sw, s0)


# ---- 5. the switch -------------------------------------------------------------------------------------------------------------------------------
def test_without_the_flag_the_general_kernels_run(mutag_graphs):
    rng = np.random.default_rng(9)
    gl = refocus(small_graphs(mutag_graphs, 16), 'n', rng)
    x, y, sw = MultiGraphSequencer(gl, 'n', 'average', 16, shuffle=False)[0]
    s0 = rng.normal(0, 0.1, (x[0].shape[0], 16)).astype(np.float32)
    def model():
        ns, no = nets('n', 16, True, hidden_state=[16], act='tanh')
        return CLS['n'](ns, no, 16, 4, 0.0)
    flagged_step(model(), x, y, sw, s0, flag=False, name=GENERAL)
    flagged_step(model(), x, y, sw, s0)


def test_a_one_layer_model_does_not_see_the_flag(mutag_graphs):
    """Bit-identical losses, predictions and gradients with and without the flag, on the one-layer persistent kernels both times."""
    rng = np.random.default_rng(10)
    gl = refocus(small_graphs(mutag_graphs, 16), 'n', rng)
    x, y, sw = MultiGraphSequencer(gl, 'n', 'average', 16, shuffle=False)[0]
    s0 = torch.from_numpy(rng.normal(0, 0.1, (x[0].shape[0], 16)).astype(np.float32)).cuda()
    runs = []
    for flags in (0, nat.FLAG_TRAIN_HIDDEN_SMALL, nat.FLAG_TRAIN_HIDDEN_SMALL | nat.FLAG_UNFUSED | nat.FLAG_NO_EARLY_EXIT):
        ns, no = nets('n', 16, True)
        m = CLS['n'](ns, no, 16, 4, 0.0)
        m.compile(optimizer=SGD(0.0), loss='categorical_crossentropy')
        m.native_flags = flags
        tr = LoopTrainer(m)
        res = tr.train_step(x, y, sw, state0=s0, apply=False, seed=3)
        assert last_name() == ONE_LAYER, last_name()
        torch.cuda.synchronize()
        runs.append([res['loss'].reshape(1).cpu().numpy(), res['y_pred'].cpu().numpy()] + [g.detach().cpu().numpy().copy() for g in tr.gs.gradients() + tr.go.gradients()])
    for other in runs[1:]:
        assert len(other) == len(runs[0])
        for u, v in zip(runs[0], other): assert np.array_equal(u, v)


def test_the_other_flag_bits_do_not_reach_a_training_step(mutag_graphs):
    """`LoopTrainer` passes this bit alone: a hidden-layer model with inference flags set beside it runs the hidden form all the same."""
    x, y, sw = MultiGraphSequencer(small_graphs(mutag_graphs, 8), 'g', 'average', 8, shuffle=False)[0]
    ns, no = nets('g', 16, False, hidden_state=[16], act='tanh')
    m = GNNgraphBased(ns, no, 16, 3, 0.0)
    m.compile(optimizer=SGD(0.0), loss='categorical_crossentropy')
    m.native_flags = nat.FLAG_TRAIN_HIDDEN_SMALL | nat.FLAG_UNFUSED | nat.FLAG_NO_EARLY_EXIT | nat.FLAG_FUSED_GEN2
    LoopTrainer(m).train_step(x, y, sw, apply=False, seed=1)
    assert last_name() == HIDDEN
    m.native_flags = nat.FLAG_UNFUSED | nat.FLAG_NO_EARLY_EXIT
    LoopTrainer(m).train_step(x, y, sw, apply=False, seed=1)
    assert last_name() == GENERAL


# ---- 6. the training-mode forward alone ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('focus,node_level,d,H', [('g', False, 16, 16), ('g', True, 32, 20), ('n', False, 0, 9)])
def test_forward_only_equals_the_building_blocks(mutag_graphs, focus, node_level, d, H):
    """`Loop(..., training=True)` as one `gnn_train_step(forward_only)` call on the hidden form against the same forward on the building
    blocks: k, state, output rows and the moving statistics both leave behind, at what
    test_training_mode_forward_in_one_library_call_equals_the_building_blocks allows (2e-6 of the largest entry)."""
    rng = np.random.default_rng(11)
    graphs = refocus(small_graphs(mutag_graphs, 12), focus, rng)
    for g in graphs: g.setAggregation('average')
    x = MultiGraphSequencer(graphs, focus, 'average', 12, shuffle=False)[0][0]

    def build():
        ns, no = nets(focus, d, True, hidden_state=[H], act='tanh')
        return CLS[focus](ns, no, d, 4, 0.0)
    weights = lambda m: [w.copy() for w in m.net_state.get_weights() + m.net_output.get_weights()]
    a, b = build(), build()
    a.native_flags = nat.FLAG_TRAIN_HIDDEN_SMALL
    b._trainer = LoopTrainer(b)
    b._trainer.use_native_step = False
    s0 = None if d == 0 else torch.from_numpy(np.random.default_rng(5).normal(0, 0.1, (x[0].shape[0], d)).astype(np.float32)).cuda()
    for rep in range(2):                                         # twice: the moving statistics carry over
        ka, sa, oa = a.Loop(*a.process_inputs(x), training=True, state0=s0, seed=7 + rep, node_level=node_level)
        assert last_name() == HIDDEN, last_name()
        kb, sb, ob = b.Loop(*b.process_inputs(x), training=True, state0=s0, seed=7 + rep, node_level=node_level)
        assert float(ka) == float(kb) == 4.0, (float(ka), float(kb))
        assert tuple(oa.shape) == tuple(ob.shape) and tuple(sa.shape) == tuple(sb.shape)
        for got, want, what in ((sa, sb, 'state'), (oa, ob, 'output')):
            err = float((got - want).abs().max() / want.abs().max().clamp(min=1e-30))
            assert err <= 2e-6, (what, rep, err)
        for wa, wb in zip(weights(a), weights(b)):
            assert np.allclose(wa, wb, rtol=2e-6, atol=1e-7), float(np.max(np.abs(wa - wb)))


# ---- 7. phases, label gradients, the joint LGNN step -------------------------------------------------------------------------------------------------
def _hidden_model(focus, d, bn, H=12):
    m = stack(focus, d, 1, True, True, bn, hidden_state=[H]).gnns[0]
    m.compile(optimizer=SGD(0.0), loss='categorical_crossentropy')
    m.native_flags = nat.FLAG_TRAIN_HIDDEN_SMALL
    return m


def test_phase_split_equals_the_whole_step(mutag_graphs):
    """As test_gpu_joint_step.test_phase_split_equals_the_whole_step: where two whole steps agree bit for bit the split agrees bit for bit
    with them; where they do not (float atomics of the scatter-add behind the output network) the per-tensor bar applies."""
    (x, y, sw), rng = batch(mutag_graphs, 'n')
    s0 = torch.from_numpy(rng.normal(0, 0.1, (x[0].shape[0], 8)).astype(np.float32)).cuda()
    runs = []
    for split in (False, False, True):
        m = _hidden_model('n', 8, True)
        tr = LoopTrainer(m)
        if not split:
            res = tr._train_step_native(x, y, sw, s0, None, False)
            tr.gs = [tr.gs]
        else:
            h = tr.forward_phase(x, state0=s0)
            assert last_name() == HIDDEN, last_name()
            tr.backward_phase(h, y, sw)
            tr.finish(h, apply=False)
            res = dict(loss=h.loss[0], y_pred=h.y_pred, state=h.state)
            tr.gs, tr.go = h.gs, h.go
        assert last_name() == HIDDEN, last_name()
        torch.cuda.synchronize()
        runs.append(_everything(m, res, tr))
    a, b, c = runs
    bitwise = all(np.array_equal(u, v) for u, v in zip(a, b))
    print(f'two whole steps agree bit for bit: {bitwise}')
    assert len(a) == len(c)
    for u, v in zip(a, c):
        assert u.shape == v.shape
        if bitwise: assert np.array_equal(u, v), float(np.max(np.abs(u - v)))
        else: assert float(np.max(np.abs(u - v))) <= BARS['kernel'] * max(float(np.max(np.abs(u))), 1e-30)


@pytest.mark.parametrize('focus,d,bn', [('n', 8, True), ('g', 20, True), ('a', 8, False), ('n', 0, False), ('a', 0, True)])
def test_label_gradients_against_autograd(mutag_graphs, focus, d, bn):
    """d loss / d nodes and d loss / d arc labels of phase 2 (the LAB instantiations: sum of dZ of the FIRST layer, d loss / d state_0)
    with random upstream gradients on the final state and on the output rows, against float64 autograd at the bar of
    test_gpu_joint_step.py (2e-5 of the tensor's largest entry)."""
    (x, y, sw), rng = batch(mutag_graphs, focus)
    m = _hidden_model(focus, d, bn)
    N, S = x[0].shape[0], d if d else 14
    s0 = rng.normal(0, 0.1, (N, d)).astype(np.float32) if d else None
    tr = LoopTrainer(m)
    h = tr.forward_phase(x, state0=None if s0 is None else torch.from_numpy(s0).cuda())
    dS = rng.normal(0, 0.01, (N, S)).astype(np.float32)
    dO = rng.normal(0, 0.01, (h.M, h.T)).astype(np.float32)
    tr.backward_phase(h, y, sw, d_state_extra=torch.from_numpy(dS).cuda(), d_out_extra=torch.from_numpy(dO).cuda(), want_label_grads=True,
                      want_arc_label_grads=True)
    assert last_name() == HIDDEN, last_name()
    k, gX, gA = _label_oracle(m, x, y, sw, s0, dS, dO, focus, d)
    assert h.k == k == 4
    _close('d_nodes', h.d_nodes, gX, LABEL_BAR)
    _close('d_arc_labels', h.d_arc_labels, gA, LABEL_BAR)


@pytest.mark.parametrize('mode', ['parallel', 'residual'])
@pytest.mark.parametrize('focus,d,get_state,get_output', [('n', 8, True, True), ('g', 8, False, True)])
def test_joint_lgnn_step_with_hidden_layers(mutag_graphs, monkeypatch, mode, focus, d, get_state, get_output):
    """Three layers with a hidden Dense in every state network, the flag on every layer, `joint_step='library'`, against
    `torch_train.lgnn_train_step`.  Layer 0 reads the 14 node labels (31 constant columns): the hidden form; the layers above read the
    labels with the layer below's state / output beside them - more than 32 constant columns: the general kernels, by the rule."""
    data, rng = batch(mutag_graphs, focus)
    x, y, sw = data
    lg = stack(focus, d, 3, get_state, get_output, True, hidden_state=[12])
    for g in lg.gnns: g.native_flags = nat.FLAG_TRAIN_HIDDEN_SMALL
    lg.compile(optimizer=SGD(0.0), loss='categorical_crossentropy', training_mode=mode, average_st_grads=False, joint_step='library')
    N = x[0].shape[0]
    s0s = [rng.normal(0, 0.1, (N, d)).astype(np.float32) for _ in lg.gnns]
    nodes, arcs, _, sm, om, adj, an, ng = x
    mask = np.logical_and(_np(sm).reshape(-1), _np(om).reshape(-1))
    layers = [dict(net_state=g.net_state.spec(), net_output=g.net_output.spec(), state_vect_dim=d, max_iteration=g.max_iteration, state_threshold=0.0)
              for g in lg.gnns]
    want = torch_train.lgnn_train_step(_np(nodes), _np(arcs), _triple(adj), _triple(an), _triple(ng), mask, layers=layers, get_state=get_state,
                                       get_output=get_output, focus=focus, state0s=s0s, y=_np(y), sample_weight=_np(sw),
                                       loss='categorical_crossentropy', training_mode=mode, average_st_grads=False)
    with names_of_steps(monkeypatch) as spy:
        logs = lg.train_step((x, y, sw), state0=[torch.from_numpy(s).cuda() for s in s0s], apply=False)
    assert lg.last_joint_route == 'library'
    assert logs['k'] == want['k']
    assert abs(float(logs['loss']) - want['loss']) <= 1e-5 * max(1.0, abs(want['loss']))
    # phase 1 of the layers bottom-up, then phase 2 top-down: the name of every call
    extra = (d if get_state else 0) + (2 if get_output else 0)
    rule = [HIDDEN if 2 * (14 + (extra if i else 0)) + 3 <= 32 else GENERAL for i in range(3)]
    assert rule[0] == HIDDEN and spy.names == rule + rule[::-1], spy.names
    nets_ = []
    for li, tp in enumerate(lg._last_tapes):
        nets_ += [(f'layer{li}.state', tp.gs[0], want['grads'][li][0], None, N), (f'layer{li}.output', tp.go, want['grads'][li][1], None, N)]
    check_network_grads('', nets_)


# ---- 8. fit() -------------------------------------------------------------------------------------------------------------------------------------
def test_fit_with_and_without_the_flag(mutag_graphs, monkeypatch):
    """Two epochs of Adam on 64 graphs in batches of 32: the losses of the flagged run are finite and equal those of the same run on the
    general kernels within 1e-4 relative (same seed, no shuffle, no Dropout)."""
    gs = small_graphs(mutag_graphs, 64)
    for g in gs: g.setAggregation('average')
    hist = {}
    for flag in (False, True):
        seq = MultiGraphSequencer(gs, 'g', 'average', 32, shuffle=False)
        ns, no = nets('g', 16, True, hidden_state=[16], act='tanh')
        gnn = GNNgraphBased(ns, no, 16, 5, 0.01)
        gnn.compile(optimizer=Adam(learning_rate=0.01), loss='categorical_crossentropy', average_st_grads=False, run_eagerly=True)
        gnn.native_flags = nat.FLAG_TRAIN_HIDDEN_SMALL if flag else 0
        np.random.seed(0); torch.manual_seed(0)
        with names_of_steps(monkeypatch) as spy:
            hist[flag] = gnn.fit(seq, epochs=2, verbose=0)['loss']
        assert len(spy.names) == 4 and set(spy.names) == {HIDDEN if flag else GENERAL}, spy.names
    on, off = np.asarray(hist[True], dtype=np.float64), np.asarray(hist[False], dtype=np.float64)
    print('fit losses, flag on', on, 'flag off', off)
    assert np.isfinite(on).all() and len(on) == 2
    assert np.all(np.abs(on - off) <= 1e-4 * np.abs(off)), (on, off)
