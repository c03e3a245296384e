"""The joint CompositeLGNN step inside the library (docs/joint_lgnn_step.md, "Composite stacks"): `gnn_train_step_composite_ex` phases 1
and 2 per layer, upstream gradients in, d loss / d nodes out (`k_label_grads_types`) - against the float64 autograd oracle
(oracle/torch_train.py) with the per-tensor bars of tests/test_gpu_training.py, against the whole step and against the building-block
route.  All networks use tanh (softmax heads): no activation kinks.

Batch A: the batch of test_composite_lgnn_joint_training_gradients (2 graphs of 50 + 40 nodes, 3 types, label widths (4, 2, 3), A = 2,
T = 2).  Batch B: 3 graphs, 88 nodes - 70 of type 0 (two 64-node tiles of the persistent kernels, 16-row tiles of the label-gradient
kernel with a remainder of 6), 17 of type 1 (16 + 1), 1 of type 2; variants without any type-2 node and with label widths (4, 0, 3)."""
import numpy as np
import pytest
import torch

from gnnkeras_amd import CompositeGraphObject
from gnnkeras_amd import _native as nat
from gnnkeras_amd.Models.MLP import MLP, get_inout_dims
from gnnkeras_amd.Models.LGNN import LGNN
from gnnkeras_amd.Models.CompositeGNN import CompositeGNNnodeBased, CompositeGNNarcBased, CompositeGNNgraphBased
from gnnkeras_amd.Models.CompositeLGNN import CompositeLGNN
from gnnkeras_amd.Models.training import SGD, LoopTrainer
from gnnkeras_amd.Sequencers.GraphSequencers import CompositeMultiGraphSequencer
from oracle import torch_train
from oracle.harness import _np, _triple
from test_gpu_training import BARS, check_network_grads, split_by_network

pytestmark = pytest.mark.gpu
LABEL_BAR = 2e-5                 # label gradients: the bar of the parameter gradients, relative to the tensor's largest entry
CC = {'n': CompositeGNNnodeBased, 'a': CompositeGNNarcBased, 'g': CompositeGNNgraphBased}
A, T = 2, 2


# ---- the batches ------------------------------------------------------------------------------------------------------------------------------
def _graph(rng, n, e, focus, dims, types=None):
    """One graph, drawn in the order of test_composite_lgnn_joint_training_gradients; `types`: the node types instead of a draw."""
    pairs = set()
    while len(pairs) < e:
        a, b = rng.integers(0, n, 2)
        if a != b: pairs.add((int(a), int(b)))
    ids = np.array(sorted(pairs), dtype=float)
    if types is None:
        types = rng.integers(0, 3, n); types[:3] = [0, 1, 2]
    tm = np.zeros((n, 3), bool); tm[np.arange(n), types] = True
    rows = e if focus == 'a' else n
    om = rng.random(rows) < 0.8 if focus != 'g' else np.ones(n, bool)
    tg = np.zeros((int(om.sum()) if focus != 'g' else 1, T)); tg[np.arange(len(tg)), rng.integers(0, T, len(tg))] = 1
    return CompositeGraphObject(nodes=rng.normal(size=(n, 4)), arcs=np.concatenate([ids, rng.normal(size=(e, A))], 1), targets=tg, type_mask=tm,
                                dim_node_label=dims, focus=focus, aggregation_mode='composite_average', **(dict(output_mask=om) if focus != 'g' else {}))


_BATCHES = {}


def batch(name, focus, dims=(4, 2, 3)):
    """(x, y, sw) of one merged batch, built once per (name, focus, dims) and shared."""
    key = (name, focus, tuple(dims))
    if key not in _BATCHES:
        rng = np.random.default_rng(41)
        if name == 'A':
            graphs = [_graph(rng, 50, 160, focus, dims), _graph(rng, 40, 120, focus, dims)]
        else:       # B: 70 / 17 / 1 nodes of types 0 / 1 / 2 over three graphs ('B-2': the type-2 node left out)
            t2 = [2] if name == 'B' else []
            parts = [[0] * 30 + [1] * 9 + t2, [0] * 25 + [1] * 5, [0] * 15 + [1] * 3]
            graphs = [_graph(rng, len(ty), 3 * len(ty), focus, dims, types=rng.permutation(np.array(ty))) for ty in parts]
        _BATCHES[key] = CompositeMultiGraphSequencer(graphs, focus, 'composite_average', len(graphs), shuffle=False)[0]
    return _BATCHES[key]


# ---- the models -------------------------------------------------------------------------------------------------------------------------------
def layer(focus, D, bn, dims=(4, 2, 3), hidden=None, max_it=3, thr=0.0):
    """One composite layer over labels of max(dims) columns; `hidden`: per-type hidden widths (the general kernels)."""
    S = D if D > 0 else max(dims)
    ns = []
    for t, dt in enumerate(dims):
        units = ([hidden[t]] if hidden else []) + [S]
        n = MLP((dt + 2 * S + sum(dims) + A,), units, 'tanh', 'lecun_normal', 'lecun_normal', rng=60 + t, batch_normalization=bn)
        n.set_weights([a * 0.5 if a.ndim == 2 else a for a in n.get_weights()])
        ns.append(n)
    no = MLP((2 * S + A if focus == 'a' else S,), [T], 'softmax', 'glorot_normal', 'glorot_normal', rng=80)
    m = CC[focus](ns, no, D, max_it, thr)
    m.compile(optimizer=SGD(0.0), loss='categorical_crossentropy')
    return m


def composite_stack(focus, D, n_layers, dims=(4, 2, 3), hidden_above=None, get_state=True, get_output=True, seed=0):
    """`n_layers` layers sized by `get_inout_dims`, BatchNormalization on; `hidden_above`: hidden widths of the layers above the first."""
    gnns = []
    for i in range(n_layers):
        hid = hidden_above if i > 0 else None
        inp, lay = get_inout_dims('state', dims, A, T, focus, D, hidden_units=hid, layer=i, get_state=get_state, get_output=get_output)
        ns = [MLP(k, lay, 'tanh', 'lecun_normal', 'lecun_normal', rng=60 + seed + t + 10 * i, batch_normalization=True) for t, k in enumerate(inp)]
        for n in ns: n.set_weights([a * 0.5 if a.ndim == 2 else a for a in n.get_weights()])
        inp, lay = get_inout_dims('output', dims, A, T, focus, D, layer=i, get_state=get_state, get_output=get_output)
        no = MLP(inp[0], lay, 'softmax', 'glorot_normal', 'glorot_normal', rng=80 + seed + i)
        gnns.append(CC[focus](ns, no, D, 3, 0.0))
    return CompositeLGNN(gnns, get_state, get_output)


def _close(name, got, ref, bar):
    got = got.detach().cpu().numpy()
    err = float(np.max(np.abs(got - ref))) / max(float(np.max(np.abs(ref))), 1e-30)
    print(name, 'error relative to the largest entry', err, 'bar', bar)
    assert got.shape == ref.shape and err <= bar, (name, err)


# ---- 1. phase 1 + phase 2 against the whole step ----------------------------------------------------------------------------------------------
def _everything(m, res, gs, go):
    out = [res['loss'].reshape(1), res['y_pred'], res['state']] + [g for g_ in gs for g in g_.gradients()] + list(go.gradients())
    out = [t.detach().cpu().numpy().copy() for t in out]
    return out + [np.array(w) for n in list(m.net_state) + [m.net_output] for w in n.get_weights()]      # (moving statistics included)


@pytest.mark.parametrize('path', ['small', 'general'])
def test_composite_phase_split_equals_the_whole_step(path, monkeypatch):
    """Phase 1 followed by phase 2 issues the launches of the whole step in the same order: where two whole steps agree bit for bit, the
    split must agree bit for bit with them as well; where they do not (float atomics of the scatter-add behind the output network), the
    per-tensor bars apply.  Loss, prediction, state, every gradient of every type's network and the moving statistics."""
    if path == 'general': monkeypatch.setenv('GNN_TRAIN_SMALL', '0')
    x, y, sw = batch('A', 'n')
    s0 = torch.from_numpy(np.random.default_rng(3).normal(0, 0.1, (x[0].shape[0], 6)).astype(np.float32)).cuda()
    runs = []
    for split in (False, False, True):
        m = layer('n', 6, True)
        tr = LoopTrainer(m)
        if not split:
            res = tr._train_step_native(x, y, sw, s0, None, False)
            gs, go = tr.gs, tr.go
        else:
            h = tr.forward_phase(x, state0=s0, composite_phases=True)
            assert (b'persistent' if path == 'small' else b'general kernels') in nat.lib().gnn_last_kernel_name()
            tr.backward_phase(h, y, sw)
            tr.finish(h, apply=False)
            res, gs, go = dict(loss=h.loss[0], y_pred=h.y_pred, state=h.state), h.gs, h.go
        torch.cuda.synchronize()
        assert (h.k if split else res['k']) == 3
        runs.append(_everything(m, res, gs, go))
    a, b, c = runs
    bitwise = all(np.array_equal(u, v) for u, v in zip(a, b))
    print(f'{path}: two whole steps agree bit for bit: {bitwise}')
    assert len(a) == len(c)
    for u, v in zip(a, c):
        assert u.shape == v.shape
        if bitwise: assert np.array_equal(u, v), float(np.max(np.abs(u - v)))
        else: assert float(np.max(np.abs(u - v))) <= BARS['kernel'] * max(float(np.max(np.abs(u))), 1e-30)


# ---- 2. the label gradients themselves --------------------------------------------------------------------------------------------------------
def _label_oracle(m, x, y, sw, s0, dS, dO, focus, d):
    """d loss / d nodes of one composite layer by float64 autograd: `torch_train._composite_forward` with the labels a leaf."""
    dt = torch.float64
    nodes, arcs, dnl, tmask, sm, om, cas, adj, an, ng = x
    mask = torch.from_numpy(np.logical_and(_np(sm).reshape(-1), _np(om).reshape(-1)))
    X = torch.tensor(_np(nodes), dtype=dt, requires_grad=True)
    lab = torch.tensor(_np(arcs)[:, 2:], dtype=dt)
    At, ANt = torch_train._sp(_triple(adj), dt), torch_train._sp(_triple(an), dt)
    CAts = [torch_train._sp(_triple(c), dt) for c in cas]
    NGt = torch_train._sp(_triple(ng), dt) if focus == 'g' else None
    tm = torch.from_numpy(np.asarray(_np(tmask)).reshape(len(cas), -1).astype(bool))
    dims = [int(v) for v in _np(dnl).reshape(-1)]
    nss, no = [torch_train.Net(*n.spec(), dtype=dt) for n in m.net_state], torch_train.Net(*m.net_output.spec(), dtype=dt)
    k, state, out, task = torch_train._composite_forward(nss, no, X, lab, dims, tm, At, ANt, CAts, d, m.max_iteration, float(m.state_threshold),
                                                         None if d == 0 else torch.tensor(s0, dtype=dt), mask, focus, _triple(adj), NGt)
    yt = torch.tensor(_np(y), dtype=dt)
    L = torch_train.keras_loss('categorical_crossentropy', yt, task, torch.ones(yt.shape[0], dtype=dt) if sw is None else torch.tensor(_np(sw), dtype=dt))
    L = L + (state * torch.tensor(dS, dtype=dt)).sum() + (out * torch.tensor(dO, dtype=dt)).sum()
    gX, = torch.autograd.grad(L, [X], allow_unused=True)
    return k, (torch.zeros_like(X) if gX is None else gX).numpy()


LABEL_CASES = [('A', 'n', 6, True, 'small', None, (4, 2, 3), 0.0), ('B', 'n', 6, True, 'small', None, (4, 2, 3), 0.0),
               ('B-2', 'n', 6, True, 'small', None, (4, 2, 3), 0.0), ('B', 'n', 6, True, 'small', None, (4, 0, 3), 0.0),
               ('A', 'g', 5, True, 'small', None, (4, 2, 3), 0.0), ('A', 'n', 0, False, 'small', None, (4, 2, 3), 0.0),
               ('A', 'n', 0, True, 'small', None, (4, 2, 3), 0.0), ('A', 'g', 6, True, 'general', None, (4, 2, 3), 0.0),
               ('B', 'n', 6, True, 'small', (12, 7, 9), (4, 2, 3), 0.0), ('A', 'n', 0, False, 'general', None, (4, 2, 3), 0.0),
               ('A', 'n', 6, True, 'small', None, (4, 2, 3), 1e9), ('A', 'n', 0, False, 'small', None, (4, 2, 3), 1e9)]


@pytest.mark.parametrize('name,focus,d,bn,path,hidden,dims,thr', LABEL_CASES)
def test_composite_label_gradients_against_autograd_and_the_building_blocks(name, focus, d, bn, path, hidden, dims, thr, monkeypatch):
    """One layer, random upstream gradients on the final state and on the output rows: d loss / d nodes of the library against float64
    autograd (bar: 2e-5 of the tensor's largest entry) and against `LoopTrainer.backward(want_label_grads=True)`: two float32 results that
    each keep the bar differ by at most twice the bar.  `path` 'general': GNN_TRAIN_SMALL=0; `hidden`: per-type hidden layers, which take
    the general kernels by themselves (widths 12 / 7 / 9: a 16-byte piece, and scalar tails of 3 and 1).  A threshold of 1e9 stops the loop
    at k = 0: d loss / d nodes is all zeros at d = 6 and the output network's state gradient (plus the upstream one) at d = 0."""
    if path == 'general': monkeypatch.setenv('GNN_TRAIN_SMALL', '0')
    x, y, sw = batch(name, focus, dims)
    m = layer(focus, d, bn, dims=dims, hidden=hidden, thr=thr)
    rng = np.random.default_rng(7)
    N, S = x[0].shape[0], d if d else 4
    s0 = rng.normal(0, 0.1, (N, d)).astype(np.float32) if d else None
    s0d = None if s0 is None else torch.from_numpy(s0).cuda()
    tr = LoopTrainer(m)
    h = tr.forward_phase(x, state0=s0d, composite_phases=True)
    assert (b'persistent' if path == 'small' and not hidden else b'general kernels') in nat.lib().gnn_last_kernel_name()
    dS = rng.normal(0, 0.01, (N, S)).astype(np.float32)
    dO = rng.normal(0, 0.01, (h.M, h.T)).astype(np.float32)
    tr.backward_phase(h, y, sw, d_state_extra=torch.from_numpy(dS).cuda(), d_out_extra=torch.from_numpy(dO).cuda(), want_label_grads=True)
    k, gX = _label_oracle(m, x, y, sw, s0, dS, dO, focus, d)
    assert h.k == k == (0 if thr > 0 else 3)
    assert tuple(h.d_nodes.shape) == (N, 4)
    if thr > 0 and d > 0: assert not np.any(gX) and not bool(torch.any(h.d_nodes != 0))
    if thr > 0 and d == 0: assert float(np.max(np.abs(gX))) > 0
    _close('d_nodes', h.d_nodes, gX, LABEL_BAR)
    # the building blocks on the same inputs
    tb = LoopTrainer(m)
    tp = tb.forward(x, state0=s0d, node_level=focus == 'g')
    y_pred = LGNN._pool(x[-1], tp.out_nodes) if focus == 'g' else tp.y_pred
    _, dpred = tb.loss_and_grad(tp, y_pred, y, sw)
    G = (tb.pool_backward(tp, dpred) if focus == 'g' else dpred.clone()) + torch.from_numpy(dO).cuda()
    d_nodes = tb.backward(tp, G.contiguous(), d_state_extra=torch.from_numpy(dS).cuda(), want_label_grads=True)
    _close('d_nodes vs blocks', h.d_nodes, d_nodes.detach().cpu().numpy(), 2 * LABEL_BAR)


# ---- 3. the joint step against the oracle -----------------------------------------------------------------------------------------------------
def joint_step_against_oracle(lg, data, focus, D, mode, avg, dims=(4, 2, 3)):
    x, y, sw = data
    lg.compile(optimizer=SGD(0.0), loss='categorical_crossentropy', training_mode=mode, average_st_grads=avg, composite_joint_step='library')
    rng = np.random.default_rng(11)
    N = x[0].shape[0]
    s0s = [rng.normal(0, 0.1, (N, D)).astype(np.float32) for _ in lg.gnns]
    nodes, arcs, dnl, tmask, sm, om_, cas, adj, an, ng = x
    mask = np.logical_and(_np(sm).reshape(-1), _np(om_).reshape(-1))
    layers = [dict(net_state=[n.spec() for n in g.net_state], net_output=g.net_output.spec(), state_vect_dim=D, max_iteration=g.max_iteration,
                   state_threshold=0.0) for g in lg.gnns]
    want = torch_train.composite_lgnn_train_step(
        _np(nodes), _np(arcs), _np(dnl).reshape(-1), _np(tmask).reshape(len(dims), -1), [_triple(c) for c in cas], _triple(adj),
        _triple(an), _triple(ng), mask, layers=layers, get_state=True, get_output=True, focus=focus, state0s=s0s, y=_np(y),
        sample_weight=_np(sw), loss='categorical_crossentropy', training_mode=mode, average_st_grads=avg)
    logs = lg.train_step((x, y, sw), state0=[torch.from_numpy(s).cuda() for s in s0s], apply=False)
    assert lg.last_joint_route == 'library'
    assert logs['k'] == want['k']
    rel = abs(float(logs['loss']) - want['loss']) / max(1.0, abs(want['loss']))
    print('loss', float(logs['loss']), want['loss'], 'rel', rel)
    assert rel <= 1e-5
    rows_t = _np(tmask).reshape(len(dims), -1).sum(1)
    nets_ = []
    for li, tp in enumerate(lg._last_tapes):
        per_type = split_by_network(tp.gs, want['grads'][li][0])
        nets_ += [(f'layer{li}.state{t}', g_, per_type[t], None, int(rows_t[t])) for t, g_ in enumerate(tp.gs)]
        nets_ += [(f'layer{li}.output', tp.go, want['grads'][li][1], None, N)]
    rows = check_network_grads('', nets_)
    print('worst gradient error: relative to the tensor', max(r['err_own'] for r in rows), 'relative to the network', max(r['err_scale'] for r in rows))
    return logs, [torch.from_numpy(s).cuda() for s in s0s]


@pytest.mark.parametrize('avg', [True, False])
@pytest.mark.parametrize('name', ['A', 'B'])
@pytest.mark.parametrize('focus,D', [('n', 6), ('g', 5)])
@pytest.mark.parametrize('mode', ['parallel', 'residual'])
def test_composite_joint_step_library_route_matches_the_oracle(mode, focus, D, name, avg):
    """The cases of test_composite_lgnn_joint_training_gradients on the library route, on both batches, `average_st_grads` on and off."""
    joint_step_against_oracle(composite_stack(focus, D, 2), batch(name, focus), focus, D, mode, avg)


def test_composite_joint_step_three_layers_upper_layers_on_the_general_path():
    """Three layers; the two upper ones carry a hidden layer in every state network and run the general kernels (per-type `dz_acc`), the
    first one the persistent kernels.  Label widths (4, 4, 4): the third layer of a composite stack reads ALL label columns of every type."""
    dims = (4, 4, 4)
    lg, data = composite_stack('n', 6, 3, dims=dims, hidden_above=[10]), batch('A', 'n', dims)
    logs, s0s = joint_step_against_oracle(lg, data, 'n', 6, 'parallel', True, dims=dims)
    # the building blocks take the third layer's label widths (above the column count: `prepare_operands` clamps them) to the same step
    lg.compile(optimizer=SGD(0.0), loss='categorical_crossentropy', training_mode='parallel', average_st_grads=True, composite_joint_step='blocks')
    blocks = lg.train_step(data, state0=s0s, apply=False)
    assert lg.last_joint_route == 'blocks' and blocks['k'] == logs['k']
    assert abs(float(blocks['loss']) - float(logs['loss'])) <= 2e-5 * max(1.0, abs(float(logs['loss'])))


# ---- 4. the keyword ---------------------------------------------------------------------------------------------------------------------------
def _weights(lg):
    return [[np.array(w) for w in n.get_weights()] for g in lg.gnns for n in list(g.net_state) + [g.net_output]]


def test_composite_joint_step_keyword():
    data = batch('A', 'n')
    s0s = [torch.from_numpy(np.random.default_rng(5).normal(0, 0.1, (data[0][0].shape[0], 6)).astype(np.float32)).cuda() for _ in range(2)]
    lg = composite_stack('n', 6, 2)
    with pytest.raises(ValueError, match='composite_joint_step'):
        lg.compile(optimizer=SGD(0.0), loss='categorical_crossentropy', composite_joint_step='nonsense')
    lg.compile(optimizer=SGD(0.0), loss='categorical_crossentropy')
    assert lg.composite_joint_step == 'blocks' and lg.last_joint_route is None
    lg.train_step(data, state0=s0s, apply=False)
    assert lg.last_joint_route == 'blocks'
    lg.compile(optimizer=SGD(0.0), loss='categorical_crossentropy', composite_joint_step='auto')
    lg.train_step(data, state0=s0s, apply=False)
    assert lg.last_joint_route == 'library'
    # an arc-focused stack with get_output hands its outputs on through the arc labels: no composite arc-label gradient, the building blocks
    arc = batch('A', 'a')
    s0a = [torch.from_numpy(np.random.default_rng(5).normal(0, 0.1, (arc[0][0].shape[0], 6)).astype(np.float32)).cuda() for _ in range(2)]
    la = composite_stack('a', 6, 2)
    la.compile(optimizer=SGD(0.0), loss='categorical_crossentropy', composite_joint_step='auto')
    la.train_step(arc, state0=s0a, apply=False)
    assert la.last_joint_route == 'blocks'
    la.compile(optimizer=SGD(0.0), loss='categorical_crossentropy', composite_joint_step='library')
    with pytest.raises(NotImplementedError, match='arc-label gradient'):
        la.train_step(arc, state0=s0a, apply=False)


def test_one_applied_step_moves_every_layer_like_the_building_blocks():
    """SGD(0.1), one applied step on each route from identically seeded models: every layer's kernels move, and the two steps differ by at
    most twice the kernel bar (two float32 results that each keep it), relative to the larger of the tensor's and the network's largest step."""
    data = batch('A', 'n')
    s0s = [torch.from_numpy(np.random.default_rng(5).normal(0, 0.1, (data[0][0].shape[0], 6)).astype(np.float32)).cuda() for _ in range(2)]
    steps = {}
    for route in ('library', 'blocks'):
        lg = composite_stack('n', 6, 2)
        lg.compile(optimizer=SGD(0.1), loss='categorical_crossentropy', training_mode='parallel', composite_joint_step=route)
        w0 = _weights(lg)
        lg.train_step(data, state0=s0s)
        lg.resolve_joint_pending()
        assert lg.last_joint_route == route
        steps[route] = [[a - b for a, b in zip(net1, net0)] for net1, net0 in zip(_weights(lg), w0)]
    for net_l, net_b in zip(steps['library'], steps['blocks']):
        trainable = [(u, v) for j, (u, v) in enumerate(zip(net_l, net_b)) if not (len(net_b) > 4 and j in (2, 3))]      # (Keras order: moving statistics at 2, 3)
        scale = max(float(np.max(np.abs(v))) for _, v in trainable)
        assert scale > 0
        for u, v in trainable:
            if v.ndim == 2: assert float(np.max(np.abs(u))) > 0
            assert float(np.max(np.abs(u - v))) <= 2 * BARS['kernel'] * max(float(np.max(np.abs(v))), scale)
