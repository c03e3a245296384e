"""The constants line of a large batch is built once and kept with the batch (include/gnnloop.h: gnn_loop_args_t::xc; sparse.py:
`SparseMatrix.constants_line`): every check here is BIT identity (`torch.equal`) - the line against the aggregates of the existing C
entry, forwards and training steps with the kept line against the same calls with reuse switched off, a stale line never surviving
an edit of what it was computed from, and the models that do not take the line ignoring it."""
import numpy as np
import pytest
import torch

from gnnkeras_amd import _native as nat
from gnnkeras_amd import ops
from gnnkeras_amd.sparse import SparseMatrix
from gnnkeras_amd.synth import er_device_batch
from gnnkeras_amd.Models.MLP import MLP, get_inout_dims
from gnnkeras_amd.Models.GNN import GNNnodeBased

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SIZES = [(200_000, 2_000_000), (1_000_000, 10_000_000)]
MODES = ['average', 'sum']


def _model(d=64, K=5, seed=0, L=14, A=3):
    inp, lay = get_inout_dims('state', L, A, 2, 'n', d)
    ns = MLP(inp[0], lay, 'selu', 'lecun_normal', 'lecun_normal', rng=seed, device=DEV)
    inp, lay = get_inout_dims('output', L, A, 2, 'n', d)
    no = MLP(inp[0], lay, 'softmax', 'glorot_normal', 'glorot_normal', rng=seed + 1, device=DEV)
    return GNNnodeBased(ns, no, d, K, 0.0)


_batches = {}


def _batch(N, E, mode):
    """One ER batch per (size, aggregation), labels drawn from a normal distribution (sums of one-hot rows would be exact in any order)."""
    if (N, E, mode) not in _batches:
        _batches.clear()                                        # (one at a time: a 1 M-node batch holds ~0.5 GB)
        x = er_device_batch(N, E, DEV, aggregation_mode=mode, seed=7)
        gen = torch.Generator(device=DEV); gen.manual_seed(11)
        x[0] = torch.randn(x[0].shape, generator=gen, device=DEV)
        x[1][:, 2:] = torch.randn((E, x[1].shape[1] - 2), generator=gen, device=DEV)
        _batches[(N, E, mode)] = x
    return _batches[(N, E, mode)]


def _fresh(x):
    """The same batch as new objects: nothing cached on them."""
    adj, arcn = x[5], x[6]
    d = adj.device_csr(DEV)
    mk = lambda m: SparseMatrix.device_only(m.dense_shape, {k: v for k, v in m.device_csr(DEV).items() if k not in ('light', 'heavy')}, DEV)
    assert d['heavy'] is None
    return [x[0], x[1], x[2], x[3], x[4], mk(adj), mk(arcn), x[7]]


def _state0(N, d=64):
    gen = torch.Generator(device=DEV); gen.manual_seed(3)
    return torch.randn((N, d), generator=gen, device=DEV) * 0.1


def _expected_line(x):
    nodes, arcs, adj, arcn = x[0], x[1], x[5], x[6]
    L, A = nodes.shape[1], arcs.shape[1] - 2
    line = torch.zeros((nodes.shape[0], 32), device=DEV)
    line[:, :L] = nodes
    line[:, L:2 * L] = ops.aggregate(adj.device_csr(DEV), nodes.contiguous())                      # gnn_aggregate, the existing C entry
    line[:, 2 * L:2 * L + A] = ops.aggregate(arcn.device_csr(DEV), arcs[:, 2:].contiguous())
    line[:, 2 * L + A] = 1.0
    return line


def _loop(gnn, x, s0):
    k, state, out = gnn.Loop(*gnn.process_inputs(x), state0=s0)
    torch.cuda.synchronize()
    return k, state, out


def _same(a, b):
    return all(torch.equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('N,E', SIZES)
def test_line_equals_the_aggregates_of_the_c_entry(N, E, mode):
    x = _fresh(_batch(N, E, mode))
    gnn = _model()
    _loop(gnn, x, _state0(N))
    e = x[5].__dict__.get('_xc')
    assert e is not None and e['valid'], 'the forward of a large homogeneous graph keeps its line'
    assert nat.lib().gnn_last_kernel_name().decode().startswith('k_state_fused4<64')
    want = _expected_line(x)
    assert torch.equal(e['line'], want)


def _skewed_batch(N=40_000, mode='average'):
    """Empty rows, rows above 16 and above 32 in-arcs (an ER graph of mean in-degree 10 has next to none of the last kind)."""
    gen = torch.Generator(device=DEV); gen.manual_seed(5)
    E0 = 8 * N
    src = torch.randint(0, N, (E0,), generator=gen, device=DEV)
    dst = torch.randint(200, N, (E0,), generator=gen, device=DEV)                 # nodes 0 .. 199 get no random arc
    hub = [(torch.randint(0, N, (n,), generator=gen, device=DEV), torch.full((n,), j, device=DEV))
           for j, n in ((0, 70), (1, 40), (2, 33), (3, 32), (4, 20), (5, 17), (6, 16), (7, 1))]   # 8 .. 199 stay empty
    src = torch.cat([src] + [h[0] for h in hub]); dst = torch.cat([dst] + [h[1] for h in hub])
    keys = torch.unique(src * N + dst)
    keys = keys[(keys // N) != (keys % N)]
    src, dst = keys // N, keys % N
    E = int(keys.numel())
    order = torch.sort(dst, stable=True).indices
    counts = torch.bincount(dst, minlength=N)
    assert int(counts[0]) > 32 and int(counts[4]) > 16 and int((counts == 0).sum()) >= 150
    rowptr = torch.zeros(N + 1, dtype=torch.int64, device=DEV); rowptr[1:] = torch.cumsum(counts, 0)
    rowptr = rowptr.to(torch.int32)
    scale = torch.where(counts > 0, 1.0 / counts.clamp(min=1).to(torch.float32), torch.ones((), device=DEV)) if mode == 'average' else None
    op = lambda ids, n_src: SparseMatrix.device_only((n_src, N), dict(rowptr=rowptr, src=ids, w=None, row_scale=scale, n_src=int(n_src), n_dst=N,
                                                                       nnz=E, max_degree=int(counts.max())), DEV)
    nodes = torch.randn((N, 14), generator=gen, device=DEV)
    arcs = torch.randn((E, 5), generator=gen, device=DEV)
    arcs[:, 0], arcs[:, 1] = src.to(torch.float32), dst.to(torch.float32)
    ones = torch.ones(N, dtype=torch.bool, device=DEV)
    ng = SparseMatrix(np.zeros((0, 2), np.int64), np.zeros(0, np.float32), (N, 1))
    return [nodes, arcs, torch.tensor([[14]], dtype=torch.int32), ones, ones.clone(), op(src[order].to(torch.int32), N), op(order.to(torch.int32), E), ng]


@pytest.mark.parametrize('mode', MODES)
def test_line_on_empty_and_long_rows(mode, monkeypatch):
    monkeypatch.setenv('GNN_XC_MIN_NODES', '0')                # (the XC form from 32 768 nodes on: a graph small enough to build by hand)
    x = _skewed_batch(mode=mode)
    gnn = _model()
    got = _loop(gnn, x, _state0(x[0].shape[0]))
    e = x[5].__dict__.get('_xc')
    assert e is not None and e['valid']
    assert torch.equal(e['line'], _expected_line(x))
    assert _same(_loop(gnn, x, _state0(x[0].shape[0])), got)
    monkeypatch.setenv('GNN_XC_REUSE', '0')
    assert _same(_loop(gnn, _fresh(x), _state0(x[0].shape[0])), got)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('N,E', SIZES)
def test_three_loops_on_one_batch_equal_a_loop_without_reuse(N, E, mode, monkeypatch):
    x = _fresh(_batch(N, E, mode))
    gnn, s0 = _model(), _state0(N)
    first = _loop(gnn, x, s0)
    line = x[5]._xc['line']
    assert x[5]._xc['valid']
    for _ in range(2):
        again = _loop(gnn, x, s0)
        assert _same(again, first)
        assert x[5]._xc['line'] is line and x[5]._xc['valid']
    assert float(first[0]) == 5.0
    monkeypatch.setenv('GNN_XC_REUSE', '0')
    y = _fresh(x)
    plain = _loop(gnn, y, s0)
    assert '_xc' not in y[5].__dict__
    assert _same(plain, first)
    # another model on the same batch reads the same line (it depends on no weight)
    monkeypatch.delenv('GNN_XC_REUSE')
    other = _model(seed=40)
    assert _same(_loop(other, x, s0), _loop(other, y, s0)) and x[5]._xc['line'] is line


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('N,E', SIZES)
def test_a_stale_line_does_not_survive_an_edit(N, E, mode):
    src = _batch(N, E, mode)
    x = _fresh(src)
    x[0], x[1] = src[0].clone(), src[1].clone()
    gnn, s0 = _model(), _state0(N)
    before = _loop(gnn, x, s0)
    x[0].mul_(2)                                               # in place: the same object, another version
    edited = _loop(gnn, x, s0)
    assert x[5]._xc['valid']
    fresh = _fresh(x)                                          # a fresh model's call on the edited labels, nothing cached
    want = _loop(_model(), fresh, s0)
    assert _same(edited, want) and not torch.equal(edited[1], before[1])
    assert torch.equal(x[5]._xc['line'], _expected_line(x))
    # another `arcs` tensor (same shape, other arc labels)
    x[1] = x[1].clone(); x[1][:, 2:] *= -0.5
    swapped = _loop(gnn, x, s0)
    fresh = _fresh(x)
    assert _same(swapped, _loop(_model(), fresh, s0)) and not torch.equal(swapped[1], edited[1])
    assert torch.equal(x[5]._xc['line'], _expected_line(x))


def _train(x, steps, reuse, monkeypatch, seed=0):
    from gnnkeras_amd.Models.training import Adam
    if reuse: monkeypatch.delenv('GNN_XC_REUSE', raising=False)
    else: monkeypatch.setenv('GNN_XC_REUSE', '0')
    gnn = _model(K=4, seed=seed)
    gnn.compile(optimizer=Adam(0.001), loss='categorical_crossentropy', metrics=['accuracy'])
    N = x[0].shape[0]
    gen = torch.Generator(device=DEV); gen.manual_seed(9)
    y = torch.nn.functional.one_hot(torch.randint(0, 2, (N,), generator=gen, device=DEV), 2).to(torch.float32)
    from gnnkeras_amd.Models.training import LoopTrainer
    tr = gnn._trainer = LoopTrainer(gnn)
    assert tr._native_step_applies(y)
    res = []
    for _ in range(steps):
        r = tr.train_step(x, y, None, state0=_state0(N), seed=0)          # (what GNNnodeBased.train_step runs; it keeps y_pred and the state)
        torch.cuda.synchronize()
        res.append([r['loss'].clone(), r['y_pred'].clone(), r['state'].clone(), torch.tensor(float(r['k']))] +
                   [g.clone() for h in (tr.gs, tr.go) for g in list(h.dW) + list(h.db)] +
                   [w.clone() for w in list(gnn.net_state.weights) + list(gnn.net_output.weights)])      # (moving statistics and updated weights included)
    return gnn, res


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('N,E', SIZES)
def test_train_steps_equal_with_and_without_reuse(N, E, mode, monkeypatch):
    src = _batch(N, E, mode)
    x = _fresh(src)
    x[0] = src[0].clone()
    assert nat.lib() is not None
    gnn, kept = _train(x, 3, True, monkeypatch)
    assert x[5]._xc['valid'] and 'row-streaming' in nat.lib().gnn_last_kernel_name().decode()
    assert torch.equal(x[5]._xc['line'], _expected_line(x))
    y = _fresh(x)
    _, plain = _train(y, 3, False, monkeypatch)
    assert '_xc' not in y[5].__dict__
    for a, b in zip(kept, plain): assert _same(a, b)
    # the training step and the forward share the line; an in-place edit between two steps refills it
    monkeypatch.delenv('GNN_XC_REUSE', raising=False)
    line = x[5]._xc['line']
    fwd = _loop(gnn, x, _state0(N))
    assert x[5]._xc['line'] is line
    monkeypatch.setenv('GNN_XC_REUSE', '0')
    assert _same(fwd, _loop(gnn, y, _state0(N)))
    x[0].mul_(2)
    _, kept = _train(x, 2, True, monkeypatch, seed=20)
    _, plain = _train(_fresh(x), 2, False, monkeypatch, seed=20)
    for a, b in zip(kept, plain): assert _same(a, b)


def _with_sentinel_line(monkeypatch, N):
    """Every `ops.loop_forward` gets a line it must not touch where the call does not take the XC form."""
    line = torch.full((N, 32), -7.0, device=DEV)
    real = ops.loop_forward

    def forward(*args, **kw):
        kw['xc'], kw['xc_valid'] = line, False
        return real(*args, **kw)
    monkeypatch.setattr(ops, 'loop_forward', forward)
    return line


def test_per_arc_weights_ignore_the_line(monkeypatch):
    N, E = SIZES[0]
    x = _fresh(_batch(N, E, 'average'))
    d = dict(x[5].device_csr(DEV))
    gen = torch.Generator(device=DEV); gen.manual_seed(2)
    d['w'], d['row_scale'] = torch.rand(E, generator=gen, device=DEV) + 0.5, None
    x[5] = SparseMatrix.device_only(x[5].dense_shape, {k: v for k, v in d.items() if k not in ('light', 'heavy')}, DEV)
    gnn, s0 = _model(), _state0(N)
    want = _loop(gnn, x, s0)
    assert '_xc' not in x[5].__dict__, 'no line is kept where the library would not read it'
    line = _with_sentinel_line(monkeypatch, N)
    assert _same(_loop(gnn, x, s0), want)
    assert bool((line == -7.0).all())


def test_composite_model_ignores_the_line(monkeypatch):
    from gnnkeras_amd.synth import er_composite_graph
    from gnnkeras_amd.Models.CompositeGNN import CompositeGNNnodeBased
    from gnnkeras_amd.Sequencers.GraphSequencers import CompositeMultiGraphSequencer
    N, E, dims, d = 200_000, 2_000_000, (14, 8, 4), 64
    inp, lay = get_inout_dims('state', dims, 3, 2, 'n', d)
    nets = [MLP(i, lay, 'selu', 'lecun_normal', 'lecun_normal', rng=t, device=DEV) for t, i in enumerate(inp)]
    inp, lay = get_inout_dims('output', dims, 3, 2, 'n', d)
    no = MLP(inp[0], lay, 'softmax', 'glorot_normal', 'glorot_normal', rng=9, device=DEV)
    gnn = CompositeGNNnodeBased(nets, no, d, 5, 0.0)
    graph = er_composite_graph(N, E, dim_node_label=dims, aggregation_mode='average', seed=4)
    x = CompositeMultiGraphSequencer([graph], 'n', 'average', 1, shuffle=False, device=DEV)[0][0]
    s0 = _state0(N)
    want = _loop(gnn, x, s0)
    line = _with_sentinel_line(monkeypatch, N)
    assert _same(_loop(gnn, x, s0), want)
    assert bool((line == -7.0).all())
