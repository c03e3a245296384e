"""The Dropout form of the persistent small-graph training kernels (gnnkeras_amd/csrc/kernels_train_small.hpp, DROP instantiations;
opt-in: `model.native_flags |= nat.FLAG_TRAIN_DROPOUT_SMALL`, together with `FLAG_TRAIN_HIDDEN_SMALL` for a state network with a hidden
layer): a state network with Dropout / AlphaDropout behind its Dense layers trains with all iterations of a sweep in one launch.  The
oracle tests carry the flag(s), assert through `gnn_last_kernel_name()` that the Dropout form ran, and compare against the float64
autograd oracle fed the same masks (oracle/torch_train.py: `Net._dropout`) at the bars of tests/test_gpu_training.py: `BARS` per tensor
with the counted kink allowance, `Y_PRED_BAR`, loss within 1e-5, k exact, moving statistics within 1e-5 (all inside `check_step`).
MUTAG-sized inputs, the sizes of tests/test_gpu_train_hidden_small.py.

The rule (padded widths 16 / 32, at most one layer per position, positions behind Dense layers) is pinned on the host by
tests/test_train_dropout_plan_host.py."""
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
from test_gpu_training import BARS, CLS, check_step, nets, refocus
from test_gpu_joint_step import LABEL_BAR, batch, stack
from test_gpu_train_hidden_small import names_of_steps, small_graphs

pytestmark = pytest.mark.gpu
DROPOUT = 'train_step: persistent small-graph kernels (dropout)'
HIDDEN_DROPOUT = 'train_step: persistent small-graph kernels (hidden layer, dropout)'
GENERAL = 'train_step: general kernels'
BOTH = nat.FLAG_TRAIN_DROPOUT_SMALL | nat.FLAG_TRAIN_HIDDEN_SMALL


def last_name():
    return nat.lib().gnn_last_kernel_name().decode()


def drop_nets(focus, d, bn, rate, pos, hidden=None, alpha=False, **kw):
    """`nets` of tests/test_gpu_training.py with Dropout (AlphaDropout: `alpha`) layers of rate `rate` at the positions `pos` of the state network."""
    ns, no = nets(focus, d, bn, hidden_state=None if hidden is None else [hidden], **kw)
    ns.dropout_rate, ns.dropout_pos, ns.alphadropout = [rate] * len(pos), list(pos), alpha
    return ns, no


def flagged_step(model, x, y, sw, s0, flags=None, name=None, seed=5, **kw):
    """`check_step` on the in-library step (the oracle comparison at the project's bars, the oracle fed the masks of `seed`) with the
    flag(s) set, and which kernels ran."""
    hidden = len(model.net_state.units) == 2
    model.native_flags = (BOTH if hidden else nat.FLAG_TRAIN_DROPOUT_SMALL) if flags is None else flags
    out = check_step(model, x, y, sw, s0, native=True, seed=seed, **kw)
    want = name or (HIDDEN_DROPOUT if hidden else DROPOUT)
    assert last_name() == want, last_name()
    return out


def grads_of(tr):
    return [[g.detach().cpu().numpy().copy() for g in h.gradients()] for h in (tr.gs, tr.go)]


def close_to_the_other_route(got, ref):
    """Two float32 results that each keep a bar differ by at most twice the bar (the rule of
    test_joint_step_library_route_with_dropout_behind_dense_layers): per tensor, relative to its largest entry or the network's."""
    worst = 0.0
    for net_a, net_b in zip(got, ref):
        assert len(net_a) == len(net_b)
        scale = max(float(np.max(np.abs(t))) for t in net_b)
        assert scale > 0
        for u, v in zip(net_a, net_b):
            err = float(np.max(np.abs(u - v))) / max(float(np.max(np.abs(v))), scale)
            worst = max(worst, err)
            assert err <= 2 * BARS['kernel'], err
    return worst


# ---- 1. LOCAL form, one tile ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bn', [False, True])
@pytest.mark.parametrize('max_it', [1, 6])
def test_one_tile(mutag_graphs, bn, max_it):
    """Three graphs, at most 64 nodes together: one workgroup, no partner at any barrier.  One layer, d = 16, Dropout 0.25 behind it."""
    gl = [g for g in small_graphs(mutag_graphs, 40) if g.nodes.shape[0] <= 20][:3]
    assert len(gl) == 3 and sum(g.nodes.shape[0] for g in gl) <= 64
    x, y, sw = MultiGraphSequencer(gl, 'g', 'average', 3, shuffle=False)[0]
    ns, no = drop_nets('g', 16, bn, 0.25, [1], act='tanh')
    s0 = np.random.default_rng(21).normal(0, 0.1, (x[0].shape[0], 16)).astype(np.float32)
    res, want = flagged_step(GNNgraphBased(ns, no, 16, max_it, 0.0), x, y, sw, s0)
    assert res['k'] == max_it


# ---- 2. LOCAL form, several tiles -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('focus,bn,d,H,pos,rate,alpha,act,mode,loss', [
    ('g', True, 32, None, [1], 0.2, False, 'tanh', 'average', 'categorical_crossentropy'),
    ('n', False, 20, None, [1], 0.1, True, 'selu', 'average', 'categorical_crossentropy'),      # 20 of 32 columns: AlphaDropout's fill stays out of the pads
    ('a', True, 0, None, [1], 0.3, False, 'tanh', 'sum', 'categorical_crossentropy'),           # state = the 14 label columns (of 16)
    ('g', True, 32, 20, [1], 0.2, False, 'tanh', 'average', 'categorical_crossentropy'),        # a padded hidden width (20 of 32)
    ('n', False, 0, 9, [1, 2], 0.1, True, 'selu', 'average', 'categorical_crossentropy'),       # both pads, AlphaDropout at both positions
    ('a', False, 16, 16, [2], 0.2, False, 'tanh', 'average', 'categorical_crossentropy'),
    ('g', False, 32, 32, [1, 2], 0.2, False, 'tanh', 'normalized', 'categorical_crossentropy'), # per-ARC weights: the HAS_W instantiations
    ('g', True, 16, None, [1], 0.2, False, 'tanh', 'average', 'mse'),                           # mean squared error behind a sigmoid head
])
def test_several_tiles(mutag_graphs, focus, bn, d, H, pos, rate, alpha, act, mode, loss):
    """16 graphs in tiles cut at graph boundaries (the state never leaves LDS; the tiles meet for the BatchNorm statistics and the loop
    condition).  The masks are hashed from the node's GLOBAL row: a tile that used its local row would draw other masks than the oracle."""
    rng = np.random.default_rng(50 + d + (H or 0))
    gl = refocus(small_graphs(mutag_graphs, 16), focus, rng)
    x, y, sw = MultiGraphSequencer(gl, focus, mode, 16, shuffle=False)[0]
    assert x[5].matrix.tiles(64) is not None and len(x[5].matrix.tiles(64)) > 2
    ns, no = drop_nets(focus, d, bn, rate, pos, hidden=H, alpha=alpha, act=act, out_act='sigmoid' if loss == 'mse' else 'softmax',
                       scale=0.2 if mode == 'sum' else 0.5)
    s0 = rng.normal(0, 0.1, (x[0].shape[0], d)).astype(np.float32) if d > 0 else None
    res, want = flagged_step(CLS[focus](ns, no, d, 5, 0.0), x, y, sw, s0, loss=loss)
    assert res['k'] == 5


# ---- 3. early exit on the dropped-out state -----------------------------------------------------------------------------------------------------
EXIT = dict(d=12, H=16, rate=0.05, scale=0.25, threshold=0.307, seed=5)      # chosen on the CPU with the float64 oracle: see the test


def _predicate_ratios(ns, x, s0, seed, max_it):
    """||state_t - state_(t-1)|| / ||state_(t-1)|| of every node at every evaluation of the loop condition (t = 0: against the all-ones
    state of the reference), in float64 with the oracle's network and masks - the loop of torch_train.train_step without its exit."""
    nodes, arcs, _, sm, om, adj, an, ng = x
    dt = torch.float64
    net = torch_train.Net(*ns.spec(), dtype=dt, net_id=0, step_seed=torch_train.mix32(0x5EED, seed))
    X, lab = torch.tensor(_np(nodes), dtype=dt), torch.tensor(_np(arcs)[:, 2:], dtype=dt)
    At, ANt = torch_train._sp(_triple(adj), dt), torch_train._sp(_triple(an), dt)
    agg_arcs, agg_nodes = torch.sparse.mm(ANt, lab), torch.sparse.mm(At, X)
    state, out = torch.tensor(s0, dtype=dt), []
    old = torch.ones_like(state)
    with torch.no_grad():
        for t in range(max_it + 1):
            out.append((torch.sqrt(((state - old) ** 2).sum(1)) / torch.sqrt((old ** 2).sum(1))).numpy())
            if t < max_it: state, old = net(torch.cat([state, X, torch.sparse.mm(At, state), agg_nodes, agg_arcs], dim=1)), state
    return out


def test_early_exit_on_the_dropped_out_state(mutag_graphs):
    """The loop stops on its own, and what it watches is the dropped-out state: fresh masks every iteration keep every node moving by a
    few tenths of its norm, so the threshold is of that size.  Dropout rate, weight scale and threshold (`EXIT`) were chosen with the
    float64 oracle so that its k is strictly between 1 and 30 and no node's ratio at any executed evaluation of the condition lies
    within 1e-3 (relative) of the threshold - float32 cannot flip k; both are asserted here before the kernels run.
    `average_st_grads` divides every gradient of the state network by that k."""
    c = EXIT
    x, y, sw = MultiGraphSequencer(small_graphs(mutag_graphs, 24), 'g', 'average', 24, shuffle=False)[0]
    ns, no = drop_nets('g', c['d'], True, c['rate'], [1], hidden=c['H'], hidden_out=[7], act='tanh', scale=c['scale'])
    s0 = np.random.default_rng(6).normal(0, 0.1, (x[0].shape[0], c['d'])).astype(np.float32)
    ratios = _predicate_ratios(ns, x, s0, c['seed'], 30)
    k_want = next(t for t, r in enumerate(ratios) if not (r > c['threshold']).any())
    executed = np.concatenate(ratios[:k_want + 1])
    margin = float(np.min(np.abs(executed / c['threshold'] - 1.0)))
    print(f'oracle k {k_want}, closest ratio to the threshold: {margin:.3e} relative')
    assert 1 < k_want < 30 and margin > 1e-3
    res, want = flagged_step(GNNgraphBased(ns, no, c['d'], 30, c['threshold']), x, y, sw, s0, seed=c['seed'], avg=True)
    assert want['k'] == k_want and res['k'] == want['k']


# ---- 4. general form: arcs cross tiles ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H', [None, 32])
def test_general_form_on_one_connected_graph(H):
    """One Erdos-Renyi graph of 150 nodes and 3 000 arcs (mean in-degree 20: rows beyond 16 arcs take the gather's tail loop): three tiles
    of 64 / 64 / 22 consecutive nodes, neighbour rows - dropped-out states when the layer sits behind the last Dense - exchanged through
    memory.  One layer with Dropout behind it; a hidden layer of 32 with Dropout between the two."""
    g = er_graph(150, 3000, focus='n', aggregation_mode='average', seed=77)
    x, y, sw = MultiGraphSequencer([g], 'n', 'average', 1, shuffle=False)[0]
    assert x[5].matrix.tiles(64) is None
    deg = np.bincount(_np(x[1])[:, 1].astype(np.int64), minlength=150)
    assert deg.max() > 16 and deg.min() >= 1
    ns, no = drop_nets('n', 32, True, 0.2, [1], hidden=H, act='tanh', scale=0.3)
    s0 = np.random.default_rng(8).normal(0, 0.1, (150, 32)).astype(np.float32)
    flagged_step(CLS['n'](ns, no, 32, 5, 0.0), x, y, sw, s0)


# ---- 5. the switch and the masks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,pos', [(None, [1]), (16, [1, 2])])
def test_the_switch_and_the_masks(mutag_graphs, H, pos):
    """Without the flag the general kernels run; with it the same seed draws the same masks (k, loss and every gradient of the two routes
    agree as two float32 results that each keep a bar); another seed draws others; the same seed twice the same."""
    rng = np.random.default_rng(9)
    gl = refocus(small_graphs(mutag_graphs, 16), 'n', rng)
    x, y, sw = MultiGraphSequencer(gl, 'n', 'average', 16, shuffle=False)[0]
    s0 = torch.from_numpy(rng.normal(0, 0.1, (x[0].shape[0], 16)).astype(np.float32)).cuda()

    def step(flags, seed):
        ns, no = drop_nets('n', 16, True, 0.2, pos, hidden=H, act='tanh')
        m = CLS['n'](ns, no, 16, 4, 0.0)
        m.compile(optimizer=SGD(0.0), loss='categorical_crossentropy')
        m.native_flags = flags
        tr = LoopTrainer(m)
        res = tr.train_step(x, y, sw, state0=s0, apply=False, seed=seed)
        torch.cuda.synchronize()
        return last_name(), int(res['k']), float(res['loss']), grads_of(tr)

    flags = nat.FLAG_TRAIN_DROPOUT_SMALL if H is None else BOTH
    off = step(0, 3)
    assert off[0] == GENERAL, off[0]
    if H is not None: assert step(nat.FLAG_TRAIN_HIDDEN_SMALL, 3)[0] == GENERAL          # (the HIDDEN flag alone does not admit Dropout)
    on = step(flags, 3)
    assert on[0] == (DROPOUT if H is None else HIDDEN_DROPOUT), on[0]
    assert on[1] == off[1] == 4
    assert abs(on[2] - off[2]) <= 2e-5 * max(1.0, abs(off[2])), (on[2], off[2])
    print('worst gradient entry against the general kernels:', close_to_the_other_route(on[3], off[3]))
    other, again = step(flags, 4), step(flags, 3)
    assert abs(other[2] - on[2]) > 1e-7
    assert abs(again[2] - on[2]) <= 1e-6 * abs(on[2])


# ---- 6. the training-mode forward alone ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,pos', [(None, [1]), (16, [1, 2])])
def test_forward_only_equals_the_general_kernels(mutag_graphs, H, pos):
    """`Loop(..., training=True)` as one `gnn_train_step(forward_only)` call, flag on against flag off at the same seed, on 8 graphs: k, the
    state and the state network's moving statistics (twice: they carry over)."""
    gs = small_graphs(mutag_graphs, 8)
    for g in gs: g.setAggregation('average')
    x = MultiGraphSequencer(gs, 'g', 'average', 8, shuffle=False)[0][0]

    def build(flags):
        ns, no = drop_nets('g', 16, True, 0.2, pos, hidden=H, act='tanh')
        m = GNNgraphBased(ns, no, 16, 4, 0.0)
        m.native_flags = flags
        return m
    a, b = build(nat.FLAG_TRAIN_DROPOUT_SMALL if H is None else BOTH), build(0)
    s0 = torch.from_numpy(np.random.default_rng(5).normal(0, 0.1, (x[0].shape[0], 16)).astype(np.float32)).cuda()
    for rep in range(2):
        ka, sa, oa = a.Loop(*a.process_inputs(x), training=True, state0=s0, seed=7 + rep)
        assert last_name() == (DROPOUT if H is None else HIDDEN_DROPOUT), last_name()
        kb, sb, ob = b.Loop(*b.process_inputs(x), training=True, state0=s0, seed=7 + rep)
        assert last_name() == GENERAL, last_name()
        assert float(ka) == float(kb) == 4.0, (float(ka), float(kb))
        err = float((sa - sb).abs().max() / sb.abs().max().clamp(min=1e-30))
        assert err <= 1e-5, (rep, err)
        for wa, wb in zip(a.net_state.get_weights()[2:4], b.net_state.get_weights()[2:4]):
            assert float(np.max(np.abs(wa - wb))) <= 1e-5 * float(np.max(np.abs(wb))), rep


# ---- 7. the joint LGNN step ------------------------------------------------------------------------------------------------------------------------
def test_joint_lgnn_step_with_dropout_in_the_state_networks(mutag_graphs, monkeypatch):
    """Two layers, d = 8, H = 12, Dropout 0.2 between the Dense layers of every state network, BatchNormalization, 'parallel',
    `joint_step='library'`, both flags on every layer, against the flag-off run at the same seed.  Layer 0 reads the 14 node labels (31
    constant columns): the Dropout form, and its gradients arrive through `d_nodes` of layer 1 - the LAB instantiations; layer 1 reads
    more than 32 constant columns: the general kernels, by the rule."""
    (x, y, sw), rng = batch(mutag_graphs, 'n')
    s0s = [torch.from_numpy(rng.normal(0, 0.1, (x[0].shape[0], 8)).astype(np.float32)).cuda() for _ in range(2)]

    def run(flags):
        gnns = []
        for i in range(2):
            inp, lay = get_inout_dims('state', 14, 3, 2, 'n', 8, hidden_units=[12], layer=i, get_state=True, get_output=True)
            ns = MLP(inp[0], lay, 'tanh', 'lecun_normal', 'lecun_normal', rng=10 + i, batch_normalization=True, dropout_rate=[0.2], dropout_pos=[1])
            ns.set_weights([a * 0.5 if a.ndim == 2 else a for a in ns.get_weights()])
            inp, lay = get_inout_dims('output', 14, 3, 2, 'n', 8, layer=i, get_state=True, get_output=True)
            no = MLP(inp[0], lay, 'softmax', 'glorot_normal', 'glorot_normal', rng=20 + i, batch_normalization=True)
            gnns.append(CLS['n'](ns, no, 8, 4, 0.0))
            gnns[-1].native_flags = flags
        lg = LGNN(gnns, True, True)
        lg.compile(optimizer=SGD(0.0), loss='categorical_crossentropy', training_mode='parallel', joint_step='library')
        with names_of_steps(monkeypatch) as spy:
            logs = lg.train_step((x, y, sw), state0=s0s, seed=7, apply=False)
        assert lg.last_joint_route == 'library' and logs['k'] == [4, 4]
        grads = [[g.detach().cpu().numpy().copy() for g in g_.gradients()] for tp in lg._last_tapes for g_ in (tp.gs[0], tp.go)]
        return spy.names, float(logs['loss']), grads

    names_off, loss_off, grads_off = run(0)
    names_on, loss_on, grads_on = run(BOTH)
    assert set(names_off) == {GENERAL}, names_off
    # phase 1 of the layers bottom-up, then phase 2 top-down
    assert names_on == [HIDDEN_DROPOUT, GENERAL, GENERAL, HIDDEN_DROPOUT], names_on
    assert abs(loss_on - loss_off) <= 2e-5 * max(1.0, abs(loss_off)), (loss_on, loss_off)
    print('worst gradient entry against the general kernels:', close_to_the_other_route(grads_on, grads_off))


@pytest.mark.parametrize('focus,d,H,pos', [('n', 8, None, [1]), ('a', 8, 12, [1, 2]), ('n', 0, 12, [1])])
def test_label_gradients_equal_the_general_kernels(mutag_graphs, focus, d, H, pos):
    """d loss / d nodes and d loss / d arc labels of phase 2 - the LAB instantiations of the Dropout form: the sum of dZ of the FIRST layer
    and, with state_0 = nodes (d = 0), d loss / d state_0 - with random upstream gradients on the final state and on the output rows, flag
    on against flag off at the same seed: two float32 results that each keep LABEL_BAR of the tensor's largest entry."""
    (x, y, sw), rng = batch(mutag_graphs, focus)
    N, S = x[0].shape[0], d if d else 14
    s0 = torch.from_numpy(rng.normal(0, 0.1, (N, d)).astype(np.float32)).cuda() if d else None
    got = {}
    for flags in (0, nat.FLAG_TRAIN_DROPOUT_SMALL if H is None else BOTH):
        m = stack(focus, d, 1, True, True, True, hidden_state=None if H is None else [H]).gnns[0]
        m.net_state.dropout_rate, m.net_state.dropout_pos = [0.2] * len(pos), list(pos)
        m.compile(optimizer=SGD(0.0), loss='categorical_crossentropy')
        m.native_flags = flags
        tr = LoopTrainer(m)
        h = tr.forward_phase(x, state0=s0, seed=9)
        if not got:
            dS = torch.from_numpy(rng.normal(0, 0.01, (N, S)).astype(np.float32)).cuda()
            dO = torch.from_numpy(rng.normal(0, 0.01, (h.M, h.T)).astype(np.float32)).cuda()
        tr.backward_phase(h, y, sw, d_state_extra=dS, d_out_extra=dO, want_label_grads=True, want_arc_label_grads=True)
        assert last_name() == (GENERAL if not flags else DROPOUT if H is None else HIDDEN_DROPOUT), last_name()
        torch.cuda.synchronize()
        assert h.k == 4
        got[flags] = [h.d_nodes.cpu().numpy().copy(), h.d_arc_labels.cpu().numpy().copy()]
    off, on = got[0], got[max(got)]
    for name, u, v in zip(('d_nodes', 'd_arc_labels'), on, off):
        scale = float(np.max(np.abs(v)))
        assert scale > 0 and float(np.max(np.abs(u - v))) <= 2 * LABEL_BAR * scale, (name, float(np.max(np.abs(u - v))), scale)


# ---- 8. two applied steps -----------------------------------------------------------------------------------------------------------------------------
def test_two_applied_steps_equal_the_general_kernels(mutag_graphs):
    """Adam(0.01) on two batches with given seeds, flag on, against a twin on the general kernels: every weight (moving statistics
    included) at the tolerance of test_a_failed_forward_launch_does_not_condemn_the_step_before_it."""
    gs = small_graphs(mutag_graphs, 32)
    for g in gs: g.setAggregation('average')

    def model(flags):
        ns, no = drop_nets('g', 16, True, 0.2, [1, 2], hidden=16, act='tanh')
        m = GNNgraphBased(ns, no, 16, 5, 0.0)
        m.compile(optimizer=Adam(learning_rate=0.01), loss='categorical_crossentropy', average_st_grads=False, run_eagerly=True)
        m.native_flags = flags
        return m
    seq = MultiGraphSequencer(gs, 'g', 'average', 16, shuffle=False)
    assert len(seq) == 2
    s0 = [torch.from_numpy(np.random.default_rng(i).normal(0, 0.1, (seq[i][0][0].shape[0], 16)).astype(np.float32)).cuda() for i in range(2)]
    weights = lambda m: [w.copy() for w in m.net_state.get_weights() + m.net_output.get_weights()]
    a, b = model(BOTH), model(0)
    for m, name in ((a, HIDDEN_DROPOUT), (b, GENERAL)):
        for i in range(2):
            m.train_step(seq[i], state0=s0[i], seed=11 + i)
            assert last_name() == name, last_name()
        m._trainer.resolve_pending()
        assert m._optimizer_obj().iterations == 2
    for wa, wb in zip(weights(a), weights(b)):
        assert np.allclose(wa, wb, rtol=1e-5, atol=1e-6), float(np.max(np.abs(wa - wb)))
