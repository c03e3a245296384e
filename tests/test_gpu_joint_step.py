"""The joint LGNN step inside the library (docs/joint_lgnn_step.md): `gnn_train_step_ex` phases 1 and 2 per layer, upstream gradients in,
label gradients out - against the float64 autograd oracle (oracle/torch_train.py) with the per-tensor bars of tests/test_gpu_training.py,
against the whole step (phase 0) and against the building-block route.  MUTAG's first 12 graphs (about 200 nodes), 3 layers,
max_iteration 4."""
import numpy as np
import pytest
import torch

from gnnkeras_amd import GraphObject
from gnnkeras_amd.Models.MLP import MLP, get_inout_dims
from gnnkeras_amd.Models.LGNN import LGNN
from gnnkeras_amd.Models.training import Adam, SGD, LoopTrainer
from gnnkeras_amd.Sequencers.GraphSequencers import MultiGraphSequencer
from oracle import torch_train
from oracle.harness import _np, _triple
from test_gpu_training import BARS, CLS, check_network_grads, lgnn_stack, refocus

pytestmark = pytest.mark.gpu
LABEL_BAR = 2e-5                 # label gradients: the bar of the parameter gradients, relative to the tensor's largest entry


def stack(focus, d, n_layers, get_state, get_output, bn, T=2, hidden_state=None, max_it=4):
    """`lgnn_stack` with an optional hidden layer in every state network (two Dense layers: the general kernels)."""
    if hidden_state is None: return lgnn_stack(focus, d, n_layers, get_state, get_output, bn, max_it=max_it, T=T)
    gnns = []
    for i in range(n_layers):
        inp, lay = get_inout_dims('state', 14, 3, T, focus, d, hidden_units=hidden_state, layer=i, get_state=get_state, get_output=get_output)
        ns = MLP(inp[0], lay, 'tanh', 'lecun_normal', 'lecun_normal', rng=10 + i, batch_normalization=bn)
        ns.set_weights([a * 0.5 if a.ndim == 2 else a for a in ns.get_weights()])
        inp, lay = get_inout_dims('output', 14, 3, T, focus, d, layer=i, get_state=get_state, get_output=get_output)
        no = MLP(inp[0], lay, 'softmax', 'glorot_normal', 'glorot_normal', rng=20 + i, batch_normalization=bn)
        gnns.append(CLS[focus](ns, no, d, max_it, 0.0))
    return LGNN(gnns, get_state, get_output)


def batch(mutag_graphs, focus, n_graphs=12, seed=12):
    rng = np.random.default_rng(seed)
    gl = refocus([g.copy() for g in mutag_graphs[:n_graphs]], focus, rng)
    return MultiGraphSequencer(gl, focus, 'average', n_graphs, shuffle=False)[0], rng


def arc_batch(mutag_graphs, T, seed=31):
    rng = np.random.default_rng(seed)
    gl = []
    for g in mutag_graphs[:10]:
        n = g.arcs.shape[0]
        om = rng.random(n) < 0.7
        t = np.zeros((int(om.sum()), T)); t[np.arange(len(t)), rng.integers(0, T, len(t))] = 1
        gl.append(GraphObject(nodes=g.nodes, arcs=g.arcs, targets=t, focus='a', set_mask=rng.random(n) < 0.8, output_mask=om,
                              sample_weight=rng.uniform(0.5, 1.5, len(t))))
    return MultiGraphSequencer(gl, 'a', 'average', 10, shuffle=False)[0], rng


def joint_step_against_oracle(lg, data, rng, focus, d, get_state, get_output, mode, avg):
    x, y, sw = data
    lg.compile(optimizer=SGD(0.0), loss='categorical_crossentropy', training_mode=mode, average_st_grads=avg, joint_step='library')
    N = x[0].shape[0]
    s0s = [rng.normal(0, 0.1, (N, d)).astype(np.float32) if d else None for _ in lg.gnns]
    nodes, arcs, _, sm, om, adj, an, ng = x
    mask = np.logical_and(_np(sm).reshape(-1), _np(om).reshape(-1))
    layers = [dict(net_state=g.net_state.spec(), net_output=g.net_output.spec(), state_vect_dim=d, max_iteration=g.max_iteration,
                   state_threshold=0.0) for g in lg.gnns]
    want = torch_train.lgnn_train_step(_np(nodes), _np(arcs), _triple(adj), _triple(an), _triple(ng), mask, layers=layers,
                                       get_state=get_state, get_output=get_output, focus=focus, state0s=s0s, y=_np(y),
                                       sample_weight=_np(sw), loss='categorical_crossentropy', training_mode=mode, average_st_grads=avg)
    logs = lg.train_step((x, y, sw), state0=[None if s is None else torch.from_numpy(s).cuda() for s in s0s], apply=False)
    assert lg.last_joint_route == 'library'
    assert logs['k'] == want['k']
    rel = abs(float(logs['loss']) - want['loss']) / max(1.0, abs(want['loss']))
    print('loss', float(logs['loss']), want['loss'], 'rel', rel)
    assert rel <= 1e-5
    nets_ = []
    for li, tp in enumerate(lg._last_tapes):       # (tanh / softmax networks: no activation kinks)
        nets_ += [(f'layer{li}.state', tp.gs[0], want['grads'][li][0], None, N), (f'layer{li}.output', tp.go, want['grads'][li][1], None, N)]
    rows = check_network_grads('', nets_)
    print('worst gradient error: relative to the tensor', max(r['err_own'] for r in rows), 'relative to the network', max(r['err_scale'] for r in rows))
    return want


# ---- 1. route and parity -------------------------------------------------------------------------------------------------------------------
GRID = [('g', 8, True, True), ('n', 8, True, False), ('n', 0, True, True), ('g', 8, False, True), ('a', 6, True, False)]


@pytest.mark.parametrize('focus,d,get_state,get_output', GRID)
@pytest.mark.parametrize('mode', ['parallel', 'residual'])
def test_joint_step_library_route_matches_the_oracle(mutag_graphs, focus, d, get_state, get_output, mode):
    """The parameter grid of test_lgnn_joint_training_gradients on the library route.  d = 0 (state_0 = nodes) needs iteration 0's input
    gradient; its three layers are 14, 30 and 46 wide: one persistent-kernel instantiation each (16 / 32 / 64)."""
    data, rng = batch(mutag_graphs, focus)
    joint_step_against_oracle(lgnn_stack(focus, d, 3, get_state, get_output, d != 0), data, rng, focus, d, get_state, get_output, mode, True)


@pytest.mark.parametrize('focus,get_state,get_output,mode', [('g', True, True, 'parallel'), ('n', True, False, 'residual'), ('g', False, True, 'residual'),
                                                             ('a', True, False, 'parallel')])
def test_joint_step_library_route_without_batch_normalization(mutag_graphs, focus, get_state, get_output, mode):
    data, rng = batch(mutag_graphs, focus)
    joint_step_against_oracle(lgnn_stack(focus, 8, 3, get_state, get_output, False), data, rng, focus, 8, get_state, get_output, mode, True)


@pytest.mark.parametrize('T,get_state', [(4, True), (2, False), (3, False)])
@pytest.mark.parametrize('mode', ['parallel', 'residual'])
def test_joint_step_library_route_arc_focus_with_get_output(mutag_graphs, T, get_state, mode):
    """The cases of test_lgnn_arc_focused_joint_training_with_get_output (sample weights; the offset-by-2 rule of the prepended output
    columns): the gradient reaches the layer below through d loss / d arc labels - the transposed ArcNode aggregate of the aggregated-arc
    columns plus the output network's arc-label segment."""
    data, rng = arc_batch(mutag_graphs, T)
    lg = lgnn_stack('a', 6, 3, get_state, True, True, T=T)
    want = joint_step_against_oracle(lg, data, rng, 'a', 6, get_state, True, mode, False)
    if T > 2:       # the chain through the arc labels carries a real gradient into layer 0's output network
        assert float(np.max(np.abs(want['grads'][0][1][-1]))) > 0 and float(lg._last_tapes[0].go.gradients()[-1].abs().max()) > 0


@pytest.mark.parametrize('focus,d,get_state,get_output,hidden,mode', [('n', 16, True, False, None, 'parallel'),      # state width 16
                                                                       ('g', 40, True, True, None, 'residual'),       # 33 .. 64
                                                                       ('n', 8, True, True, [12], 'parallel'),        # two Dense layers per state network
                                                                       ('a', 6, True, True, [10], 'residual')])
def test_joint_step_library_route_other_widths_and_depths(mutag_graphs, focus, d, get_state, get_output, hidden, mode):
    data, rng = batch(mutag_graphs, focus)
    joint_step_against_oracle(stack(focus, d, 3, get_state, get_output, True, hidden_state=hidden), data, rng, focus, d, get_state, get_output, mode, False)


def test_joint_step_library_route_with_dropout_behind_dense_layers(mutag_graphs):
    """Dropout layers behind Dense layers (state network: the general kernels; output network) draw the masks of the step's seed on both
    routes: the library route against the building-block route of the same checkout, the same seed.  Two float32 results that each
    keep a bar differ by at most twice the bar."""
    (x, y, sw), rng = batch(mutag_graphs, 'n')
    def model(route):
        gnns = []
        for i in range(2):
            inp, lay = get_inout_dims('state', 14, 3, 2, 'n', 8, hidden_units=[12], layer=i, get_state=True, get_output=True)
            ns = MLP(inp[0], lay, 'tanh', 'lecun_normal', 'lecun_normal', rng=10 + i, batch_normalization=True, dropout_rate=[0.2], dropout_pos=[1])
            inp, lay = get_inout_dims('output', 14, 3, 2, 'n', 8, hidden_units=[10], layer=i, get_state=True, get_output=True)
            no = MLP(inp[0], lay, ['tanh', 'softmax'], 'glorot_normal', 'glorot_normal', rng=20 + i, batch_normalization=True, dropout_rate=[0.3], dropout_pos=[1])
            gnns.append(CLS['n'](ns, no, 8, 4, 0.0))
        lg = LGNN(gnns, True, True)
        lg.compile(optimizer=SGD(0.0), loss='categorical_crossentropy', training_mode='parallel', joint_step=route)
        return lg
    s0s = [torch.from_numpy(rng.normal(0, 0.1, (x[0].shape[0], 8)).astype(np.float32)).cuda() for _ in range(2)]
    got = {}
    for route in ('library', 'blocks'):
        lg = model(route)
        logs = lg.train_step((x, y, sw), state0=s0s, seed=7, apply=False)
        assert lg.last_joint_route == route and logs['k'] == [4, 4]
        got[route] = (float(logs['loss']), [[g.detach().cpu().numpy().copy() for g in g_.gradients()] for tp in lg._last_tapes for g_ in (tp.gs[0], tp.go)])
    assert abs(got['library'][0] - got['blocks'][0]) <= 2e-5 * max(1.0, abs(got['blocks'][0]))
    for net_l, net_b in zip(got['library'][1], got['blocks'][1]):
        scale = max(float(np.max(np.abs(t))) for t in net_b)
        assert scale > 0
        for u, v in zip(net_l, net_b):
            assert float(np.max(np.abs(u - v))) <= 2 * BARS['kernel'] * max(float(np.max(np.abs(v))), scale)


def test_joint_step_keyword(mutag_graphs):
    lg = lgnn_stack('g', 8, 2, True, True, True)
    with pytest.raises(ValueError, match='joint_step'):
        lg.compile(optimizer=SGD(0.0), loss='categorical_crossentropy', joint_step='nonsense')
    lg.compile(optimizer=SGD(0.0), loss='categorical_crossentropy')
    assert lg.joint_step == 'auto' and lg.last_joint_route is None
    (x, y, sw), _ = batch(mutag_graphs, 'g')
    lg.train_step((x, y, sw), apply=False)
    assert lg.last_joint_route == 'library'
    lg.compile(optimizer=SGD(0.0), loss='categorical_crossentropy', joint_step='blocks')
    lg.train_step((x, y, sw), apply=False)
    assert lg.last_joint_route == 'blocks'


# ---- 2. phase 1 + phase 2 against the whole step ---------------------------------------------------------------------------------------------
def _plain_model(d=8):
    lg = lgnn_stack('n', d, 1, True, True, True)
    m = lg.gnns[0]
    m.compile(optimizer=SGD(0.0), loss='categorical_crossentropy')
    return m


def _everything(m, res, tr):
    out = [res['loss'].reshape(1), res['y_pred'], res['state']] + list(tr.gs[0].gradients()) + list(tr.go.gradients())
    out = [t.detach().cpu().numpy().copy() for t in out]
    return out + [np.array(w) for w in m.net_state.get_weights() + m.net_output.get_weights()]      # (moving statistics included)


@pytest.mark.parametrize('path', ['small', 'general'])
def test_phase_split_equals_the_whole_step(mutag_graphs, path, monkeypatch):
    """Phase 1 followed by phase 2 issues the launches of the whole step in the same order: where two whole steps agree bit for bit, the
    split must agree bit for bit with them as well; where they do not (float atomics of the scatter-add behind the output network), the
    per-tensor bars apply.  The case that held is printed."""
    if path == 'general': monkeypatch.setenv('GNN_TRAIN_SMALL', '0')
    (x, y, sw), rng = batch(mutag_graphs, 'n')
    s0 = torch.from_numpy(rng.normal(0, 0.1, (x[0].shape[0], 8)).astype(np.float32)).cuda()
    runs = []
    for split in (False, False, True):
        m = _plain_model()
        tr = LoopTrainer(m)
        if not split:
            res = tr._train_step_native(x, y, sw, s0, None, False)
            tr.gs = [tr.gs]
        else:
            h = tr.forward_phase(x, state0=s0)
            tr.backward_phase(h, y, sw)
            tr.finish(h, apply=False)
            res = dict(loss=h.loss[0], y_pred=h.y_pred, state=h.state)
            tr.gs, tr.go = h.gs, h.go
        torch.cuda.synchronize()
        runs.append(_everything(m, res, tr))
    a, b, c = runs
    bitwise = all(np.array_equal(u, v) for u, v in zip(a, b))
    print(f'{path}: two whole steps agree bit for bit: {bitwise}')
    assert len(a) == len(c)
    for u, v in zip(a, c):
        assert u.shape == v.shape
        if bitwise: assert np.array_equal(u, v), float(np.max(np.abs(u - v)))
        else: assert float(np.max(np.abs(u - v))) <= BARS['kernel'] * max(float(np.max(np.abs(u))), 1e-30)


# ---- 3. the label gradients themselves --------------------------------------------------------------------------------------------------------
def _label_oracle(m, x, y, sw, s0, dS, dO, focus, d):
    dt = torch.float64
    nodes, arcs, _, sm, om, adj, an, ng = x
    mask = torch.from_numpy(np.logical_and(_np(sm).reshape(-1), _np(om).reshape(-1)))
    X = torch.tensor(_np(nodes), dtype=dt, requires_grad=True)
    lab = torch.tensor(_np(arcs)[:, 2:], dtype=dt, requires_grad=True)
    At, ANt = torch_train._sp(_triple(adj), dt), torch_train._sp(_triple(an), dt)
    NGt = torch_train._sp(_triple(ng), dt) if focus == 'g' else None
    ns, no = torch_train.Net(*m.net_state.spec(), dtype=dt), torch_train.Net(*m.net_output.spec(), dtype=dt)
    k, state, out, task = torch_train._homogeneous_forward(ns, no, X, lab, At, torch.sparse.mm(ANt, lab), d, m.max_iteration, 0.0,
                                                           None if d == 0 else torch.tensor(s0, dtype=dt), mask, focus, _triple(adj), NGt)
    yt = torch.tensor(_np(y), dtype=dt)
    L = torch_train.keras_loss('categorical_crossentropy', yt, task, torch.ones(yt.shape[0], dtype=dt) if sw is None else torch.tensor(_np(sw), dtype=dt))
    L = L + (state * torch.tensor(dS, dtype=dt)).sum() + (out * torch.tensor(dO, dtype=dt)).sum()
    gX, gA = torch.autograd.grad(L, [X, lab])
    return k, gX.numpy(), gA.numpy()


def _close(name, got, ref, bar):
    got = got.detach().cpu().numpy()
    err = float(np.max(np.abs(got - ref))) / max(float(np.max(np.abs(ref))), 1e-30)
    print(name, 'error relative to the largest entry', err, 'bar', bar)
    assert got.shape == ref.shape and err <= bar, (name, err)


@pytest.mark.parametrize('focus,d,bn,path', [('n', 8, True, 'small'), ('g', 20, True, 'small'), ('a', 40, True, 'small'), ('a', 8, False, 'small'),
                                             ('n', 0, False, 'small'), ('g', 8, True, 'general'), ('a', 6, True, 'general'), ('n', 0, False, 'general'),
                                             ('n', 0, True, 'small'), ('a', 0, True, 'small'), ('g', 0, True, 'general')])
def test_label_gradients_against_autograd_and_the_building_blocks(mutag_graphs, focus, d, bn, path, monkeypatch):
    """One layer, random upstream gradients on the final state and on the output rows: d loss / d nodes and d loss / d arc labels of the
    library against float64 autograd (bar: 2e-5 of the tensor's largest entry, the bar of the parameter gradients) and against
    `LoopTrainer.backward(want_label_grads=True, want_arc_label_grads=True)`: two float32 results that each keep the bar differ by at
    most twice the bar.  State widths 8 / 20 / 40: the 16-, 32- and 64-wide persistent kernels each store their sum of dZ."""
    if path == 'general': monkeypatch.setenv('GNN_TRAIN_SMALL', '0')
    (x, y, sw), rng = batch(mutag_graphs, focus)
    m = lgnn_stack(focus, d, 1, True, True, bn).gnns[0]
    m.compile(optimizer=SGD(0.0), loss='categorical_crossentropy')
    N, S = x[0].shape[0], d if d else 14
    s0 = rng.normal(0, 0.1, (N, d)).astype(np.float32) if d else None
    s0d = None if s0 is None else torch.from_numpy(s0).cuda()
    tr = LoopTrainer(m)
    h = tr.forward_phase(x, state0=s0d)
    dS = rng.normal(0, 0.01, (N, S)).astype(np.float32)
    dO = rng.normal(0, 0.01, (h.M, h.T)).astype(np.float32)
    tr.backward_phase(h, y, sw, d_state_extra=torch.from_numpy(dS).cuda(), d_out_extra=torch.from_numpy(dO).cuda(), want_label_grads=True,
                      want_arc_label_grads=True)
    k, gX, gA = _label_oracle(m, x, y, sw, s0, dS, dO, focus, d)
    assert h.k == k == 4
    _close('d_nodes', h.d_nodes, gX, LABEL_BAR)
    _close('d_arc_labels', h.d_arc_labels, gA, LABEL_BAR)
    # the building blocks on the same inputs
    tb = LoopTrainer(m)
    tp = tb.forward(x, state0=s0d, node_level=focus == 'g')
    y_pred = LGNN._pool(x[-1], tp.out_nodes) if focus == 'g' else tp.y_pred
    _, dpred = tb.loss_and_grad(tp, y_pred, y, sw)
    G = (tb.pool_backward(tp, dpred) if focus == 'g' else dpred.clone()) + torch.from_numpy(dO).cuda()
    d_nodes = tb.backward(tp, G.contiguous(), d_state_extra=torch.from_numpy(dS).cuda(), want_label_grads=True, want_arc_label_grads=True)
    _close('d_nodes vs blocks', h.d_nodes, d_nodes.detach().cpu().numpy(), 2 * LABEL_BAR)
    _close('d_arc_labels vs blocks', h.d_arc_labels, tp.d_arc_labels.detach().cpu().numpy(), 2 * LABEL_BAR)


# ---- 4. composite stacks keep the building blocks ---------------------------------------------------------------------------------------------
def _composite_stack(mode, joint_step):
    from gnnkeras_amd import CompositeGraphObject
    from gnnkeras_amd.Models.CompositeGNN import CompositeGNNnodeBased
    from gnnkeras_amd.Models.CompositeLGNN import CompositeLGNN
    from gnnkeras_amd.Sequencers.GraphSequencers import CompositeMultiGraphSequencer
    rng = np.random.default_rng(41)
    dims, A, T, D = (4, 2, 3), 2, 2, 6

    def cg(n, e):
        pairs = set()
        while len(pairs) < e:
            a, b = rng.integers(0, n, 2)
            if a != b: pairs.add((int(a), int(b)))
        ids = np.array(sorted(pairs), dtype=float)
        types = rng.integers(0, 3, n); types[:3] = [0, 1, 2]
        tm = np.zeros((n, 3), bool); tm[np.arange(n), types] = True
        om = rng.random(n) < 0.8
        tg = np.zeros((int(om.sum()), T)); tg[np.arange(len(tg)), rng.integers(0, T, len(tg))] = 1
        return CompositeGraphObject(nodes=rng.normal(size=(n, 4)), arcs=np.concatenate([ids, rng.normal(size=(e, A))], 1), targets=tg,
                                    type_mask=tm, dim_node_label=dims, focus='n', aggregation_mode='composite_average', output_mask=om)
    seq = CompositeMultiGraphSequencer([cg(50, 160), cg(40, 120)], 'n', 'composite_average', 2, shuffle=False)
    gnns = []
    for layer in range(2):
        inp, lay = get_inout_dims('state', dims, A, T, 'n', D, layer=layer, get_state=True, get_output=True)
        ns = [MLP(i, lay, 'tanh', 'lecun_normal', 'lecun_normal', rng=60 + t + 10 * layer, batch_normalization=True) for t, i in enumerate(inp)]
        inp, lay = get_inout_dims('output', dims, A, T, 'n', D, layer=layer, get_state=True, get_output=True)
        no = MLP(inp[0], lay, 'softmax', 'glorot_normal', 'glorot_normal', rng=80 + layer)
        gnns.append(CompositeGNNnodeBased(ns, no, D, 3, 0.0))
    lg = CompositeLGNN(gnns, True, True)
    lg.compile(optimizer=SGD(0.0), loss='categorical_crossentropy', training_mode=mode, joint_step=joint_step)
    x, y, sw = seq[0]
    s0s = [torch.from_numpy(rng.normal(0, 0.1, (x[0].shape[0], D)).astype(np.float32)).cuda() for _ in range(2)]
    return lg, (x, y, sw), s0s


def test_auto_keeps_the_building_blocks_for_a_composite_stack():
    got = {}
    for js in ('auto', 'blocks'):
        lg, data, s0s = _composite_stack('parallel', js)
        logs = lg.train_step(data, state0=s0s, apply=False)
        assert lg.last_joint_route == 'blocks'
        got[js] = [float(logs['loss'])] + [g.detach().cpu().numpy().copy() for tp in lg._last_tapes for g_ in list(tp.gs) + [tp.go] for g in g_.gradients()]
    assert len(got['auto']) == len(got['blocks']) > 1
    for u, v in zip(got['auto'], got['blocks']): assert np.array_equal(u, v)
    lg, data, s0s = _composite_stack('parallel', 'library')
    with pytest.raises(NotImplementedError, match='composite'):
        lg.train_step(data, state0=s0s, apply=False)


# ---- 5. a failed backward launch moves nothing ------------------------------------------------------------------------------------------------
def _all_weights(lg):
    return [np.array(w) for g in lg.gnns for w in g.net_state.get_weights() + g.net_output.get_weights()]


@pytest.mark.parametrize('opt_cls', [Adam, SGD])
def test_a_failed_backward_launch_moves_no_layer(mutag_graphs, opt_cls, monkeypatch):
    """GNN_DEBUG_FAIL_BWD=1 lets every barrier wait of the persistent backward launch expire (layer 0 of this stack runs it; the layers
    above, with their wider label matrices, run the general kernels and succeed): layer 0's validity word stays 0, the gate word over all
    layers is 0 and no variable of ANY layer moves.  The next step learns of it at its first synchronisation, takes the counted update
    back and is the step a fresh model would have made."""
    (x, y, sw), rng = batch(mutag_graphs, 'g')
    s0s = [torch.from_numpy(rng.normal(0, 0.1, (x[0].shape[0], 8)).astype(np.float32)).cuda() for _ in range(3)]
    def model():
        lg = lgnn_stack('g', 8, 3, True, True, False)
        lg.compile(optimizer=opt_cls(0.01), loss='categorical_crossentropy', training_mode='parallel', joint_step='library')
        return lg
    lg, fresh = model(), model()
    w0 = _all_weights(lg)
    monkeypatch.setenv('GNN_DEBUG_FAIL_BWD', '1')
    lg.train_step((x, y, sw), state0=s0s)
    monkeypatch.delenv('GNN_DEBUG_FAIL_BWD')
    words = [int(tp.grads_ok_view.item()) for tp in lg._last_tapes]
    assert words[0] == 0 and int(lg._joint_gate.item()) == 0, words
    for a, b in zip(_all_weights(lg), w0): assert np.array_equal(a, b)
    with pytest.warns(RuntimeWarning, match='discarded on the device'):
        lg.train_step((x, y, sw), state0=s0s)
    fresh.train_step((x, y, sw), state0=s0s)
    assert lg._optimizer_obj().iterations == fresh._optimizer_obj().iterations == 1
    assert [int(tp.grads_ok_view.item()) for tp in lg._last_tapes] == [1, 1, 1] and int(lg._joint_gate.item()) == 1
    moved = False
    for a, b, c in zip(_all_weights(lg), _all_weights(fresh), w0):
        assert np.allclose(a, b, rtol=1e-5, atol=1e-6), float(np.max(np.abs(a - b)))
        moved = moved or not np.array_equal(a, c)
    assert moved


def test_moving_statistics_are_gated_per_layer(mutag_graphs, monkeypatch):
    """BatchNormalization on: layer 0 (persistent kernels) fails under GNN_DEBUG_FAIL_BWD=1 and keeps its moving statistics; the layers above
    (general kernels) completed their own launches and move theirs; no trainable variable of any layer moves.  `resolve_joint_pending()`
    - what `fit()` calls behind its last step - reports the discarded step and takes the counted update back."""
    (x, y, sw), rng = batch(mutag_graphs, 'g')
    s0s = [torch.from_numpy(rng.normal(0, 0.1, (x[0].shape[0], 8)).astype(np.float32)).cuda() for _ in range(3)]
    lg = lgnn_stack('g', 8, 3, True, True, True)
    lg.compile(optimizer=Adam(0.01), loss='categorical_crossentropy', training_mode='parallel', joint_step='library')
    nets = [n for g in lg.gnns for n in (g.net_state, g.net_output)]
    before = [[np.array(w) for w in n.get_weights()] for n in nets]
    monkeypatch.setenv('GNN_DEBUG_FAIL_BWD', '1')
    lg.train_step((x, y, sw), state0=s0s)
    monkeypatch.delenv('GNN_DEBUG_FAIL_BWD')
    assert [int(tp.grads_ok_view.item()) for tp in lg._last_tapes] == [0, 1, 1]
    for i, (n, b) in enumerate(zip(nets, before)):
        now = [np.array(w) for w in n.get_weights()]         # Keras order: gamma, beta, moving_mean, moving_variance, kernels / biases
        for j, (u, v) in enumerate(zip(now, b)):
            if j in (2, 3) and i >= 2: assert not np.array_equal(u, v), (i, j)      # layers 1, 2: their own word is 1
            else: assert np.array_equal(u, v), (i, j)
    assert lg._optimizer_obj().iterations == 1
    with pytest.warns(RuntimeWarning, match='discarded on the device'):
        lg.resolve_joint_pending()
    assert lg._optimizer_obj().iterations == 0
