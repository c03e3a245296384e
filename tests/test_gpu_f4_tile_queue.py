"""The tile queue of the wave-specialised iteration kernel (gnnkeras_amd/csrc/kernel_state_fused4.hpp): which workgroup computes a
row does not enter the row's arithmetic, so a forward with the queue (the default) and one with GNN_F4_TILE_QUEUE=0 (every tile dealt
statically; the switch is read at every call) must agree bit for bit in k, state and output.  gnn_debug_f4_last_tickets says whether the
launches of the last forward really drew from the queue.

Only the instantiations that carry the queue's words without spilling registers run it - padded width 64, one Dense layer, no per-arc
weights, C or XC constants (docs/rounds/f4_tile_queue_resources.md).  Padded widths 16 / 32, per-arc weights and a second Dense keep the
static form: their cases below hold the switch to "no difference" and the read-out to 0."""
import pytest
import torch

from gnnkeras_amd import _native as nat
from gnnkeras_amd.Models.GNN import GNNnodeBased
from gnnkeras_amd.Models.MLP import MLP, get_inout_dims
from gnnkeras_amd.sparse import SparseMatrix
from gnnkeras_amd.synth import er_device_batch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _model(d=64, K=3, thr=0.0, hidden=None, scale=None, L=14, A=3):
    inp, lay = get_inout_dims('state', L, A, 2, 'n', d, hidden)
    ns = MLP(inp[0], lay, 'selu', 'lecun_normal', 'lecun_normal', rng=0, device=DEV)
    if scale is not None: ns.set_weights([w * scale if w.ndim == 2 else w for w in ns.get_weights()])
    inp, lay = get_inout_dims('output', L, A, 2, 'n', d)
    no = MLP(inp[0], lay, 'softmax', 'glorot_normal', 'glorot_normal', rng=1, device=DEV)
    gnn = GNNnodeBased(ns, no, d, K, thr)
    gnn.native_flags = nat.FLAG_FUSED_GEN4
    return gnn


_batches = {}


def _batch(N):
    """One ER batch (10 arcs per node, 'average') per size, built once and never changed."""
    if N not in _batches:
        _batches.clear()
        _batches[N] = er_device_batch(N, 10 * N, DEV, aggregation_mode='average', seed=7)
    return list(_batches[N])


def _state0(N, d):
    gen = torch.Generator(device=DEV); gen.manual_seed(3)
    return torch.randn((N, d), generator=gen, device=DEV) * 0.1


def _loop(gnn, x, s0):
    k, state, out = gnn.Loop(*gnn.process_inputs(x), state0=s0)
    torch.cuda.synchronize()
    return k.clone(), state.clone(), out.clone(), int(nat.lib().gnn_debug_f4_last_tickets())


def _both(monkeypatch, gnn, x, s0):
    """The same forward with the queue and without it, in one process: (results with, tickets with)."""
    monkeypatch.setenv('GNN_F4_TILE_QUEUE', '0')
    *want, t_off = _loop(gnn, x, s0)
    assert t_off == 0, t_off
    monkeypatch.delenv('GNN_F4_TILE_QUEUE')
    *got, t_on = _loop(gnn, x, s0)
    assert nat.lib().gnn_last_kernel_name().decode().startswith('k_state_fused4<'), nat.lib().gnn_last_kernel_name()
    assert float(want[0]) >= 0
    for u, v in zip(got, want): assert torch.equal(u, v)
    return got, t_on


def test_xc_form(monkeypatch):                                                       # (a)
    N = 200_000
    got, tickets = _both(monkeypatch, _model(), _batch(N), _state0(N, 64))
    assert float(got[0]) == 3.0 and tickets > 0, (float(got[0]), tickets)


def test_pad_rows_uneven_ranges_partial_last_chunk(monkeypatch):                     # (b) 12 501 tiles: 7 x 1 563 + 1 560, three rows in the last tile
    N = 200_003
    got, tickets = _both(monkeypatch, _model(), _batch(N), _state0(N, 64))
    assert float(got[0]) == 3.0 and tickets > 0, (float(got[0]), tickets)


@pytest.mark.parametrize('d,xc,queued', [(32, '1', False), (20, '1', False), (64, '0', True)])   # (c) padded width 32 (static: see above); the C form
def test_other_widths_and_the_c_form(monkeypatch, d, xc, queued):
    N = 200_000
    monkeypatch.setenv('GNN_XC', xc)
    got, tickets = _both(monkeypatch, _model(d=d), _batch(N), _state0(N, d))
    assert float(got[0]) == 3.0 and (tickets > 0) == queued, (float(got[0]), tickets)


@pytest.mark.parametrize('form', ['per-arc weights', 'two layers'])                  # (d) HAS_W; the second Dense (hidden 48): both static (see above)
def test_arc_weights_and_second_dense(monkeypatch, form):
    N = 200_000
    x = _batch(N)
    if form == 'per-arc weights':
        d = dict(x[5].device_csr(DEV))
        gen = torch.Generator(device=DEV); gen.manual_seed(2)
        d['w'], d['row_scale'] = torch.rand(10 * N, generator=gen, device=DEV) + 0.5, None
        x[5] = SparseMatrix.device_only(x[5].dense_shape, {k: v for k, v in d.items() if k not in ('light', 'heavy')}, DEV)
    got, tickets = _both(monkeypatch, _model(hidden=48 if form == 'two layers' else None, scale=0.5), x, _state0(N, 64))
    assert float(got[0]) == 3.0 and tickets == 0, (float(got[0]), tickets)


def _draws_per_launch_at_most(N, sp=64):
    """Upper bound of the tickets one launch can draw: every chunk of every pool, and at most one ticket past the pool per workgroup."""
    lib = nat.lib()
    out = (nat.C.c_int32 * 56)()
    lib.gnn_debug_f4_tile_plan((N + 15) // 16, 512, lib.gnn_debug_f4_tile_queue_const(1, sp), out)
    return sum(out[7 * xcd + 6] + out[7 * xcd + 2] for xcd in range(8))


def test_early_exit_gated_launches_draw_nothing(monkeypatch):                        # (e)
    N, K = 200_000, 50
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    got, tickets = _both(monkeypatch, _model(K=K, thr=0.01, scale=0.25), _batch(N), _state0(N, 64))
    k = int(float(got[0]))
    assert 0 < k < K, k
    assert tickets > 0
    if cus == 256:                                                                   # (the bound is worked out for 2 x 256 workgroups)
        assert tickets <= k * _draws_per_launch_at_most(N), (tickets, k, _draws_per_launch_at_most(N))


def test_counters_are_zeroed_every_forward():                                        # (f) the switch stays on
    N = 200_000
    x, s0 = _batch(N), _state0(N, 64)
    gnn = _model(K=3)
    first, second = _loop(gnn, x, s0), _loop(gnn, x, s0)
    assert first[3] > 0 and second[3] > 0
    for u, v in zip(first[:3], second[:3]): assert torch.equal(u, v)
    longer = _model(K=5)
    a, b = _loop(longer, x, s0), _loop(longer, x, s0)
    assert float(a[0]) == 5.0 and a[3] > first[3] and b[3] > first[3], (float(a[0]), a[3], b[3], first[3])
    for u, v in zip(a[:3], b[:3]): assert torch.equal(u, v)
    assert not torch.equal(a[1], first[1])                                           # (two more iterations really ran)


def test_small_graph_stays_static(monkeypatch):                                      # (g) 2 500 tiles: 5 per workgroup
    N = 40_000
    got, tickets = _both(monkeypatch, _model(), _batch(N), _state0(N, 64))
    assert float(got[0]) == 3.0 and tickets == 0, (float(got[0]), tickets)
