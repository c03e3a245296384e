"""Host side of the phased training step of heterogeneous models (`gnn_train_step_composite_ex`, additive to C ABI 10) - no GPU: struct
layout and exports through `_native`, `gnn_train_composite_phases_supported` on covered / uncovered dims, what the pinned entry points
keep answering for the same composite arguments, an all-zero block against the plain call, and every refusal the library decides
before its first launch (host data alone: dims, network descriptions, NULLs; the device addresses below are fake and never read)."""
import ctypes as C
import os

import pytest

from gnnkeras_amd import _native as nat


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(nat.LIB_PATH):
        nat.build()
    return nat.lib()


@pytest.fixture(autouse=True)
def _default_thresholds(monkeypatch):
    monkeypatch.delenv('GNN_TRAIN_BIG_MIN_NODES', raising=False)
    monkeypatch.delenv('GNN_TRAIN_SMALL', raising=False)


DIMS = (4, 2, 3)


def _composite_args(d=6, dims=DIMS, A=2, T=2, counts=(40, 30, 20), n_arcs=280, focus='n', state_units=None, composite=1):
    """Three node types; `state_units`: hidden widths in front of every type's last Dense."""
    ta = nat.TrainArgs()
    a = ta.loop
    N, L = sum(counts), max(dims)
    a.abi_version, a.composite, a.n_types = nat.GNN_ABI_VERSION, composite, len(dims)
    a.n_nodes, a.n_arcs, a.dim_node_label, a.dim_arc_label = N, n_arcs, L, A
    a.nodes, a.ld_nodes, a.type_nodes, a.arc_labels, a.ld_arcs = 4096, L, 4096, 4096, A + 2
    a.state_dim, a.max_iteration, a.state_threshold = d, 4, 0.01
    S = d if d > 0 else L
    first = 0
    for t, (dt, n) in enumerate(zip(dims, counts)):
        a.type_dim_label[t] = dt
        first += n
        a.type_offsets[t + 1] = first
        units = list(state_units or []) + [S]
        m = a.net_state[t]
        m.in_dim, m.n_layers = dt + 2 * S + sum(dims) + A, len(units)
        for i, u in enumerate(units): m.units[i], m.activation[i], m.kernel[i], m.bias[i] = u, 3, 4096, 4096      # (fake device addresses)
    o = a.net_output
    o.in_dim, o.n_layers = (2 * S + A if focus == 'a' else S), 1
    o.units[0], o.activation[0], o.kernel[0], o.bias[0] = T, 7, 4096, 4096
    a.focus, a.n_out = nat.FOCUS[focus], (n_arcs if focus == 'a' else N)
    if focus == 'g': a.nodegraph.n_dst, a.nodegraph.n_src = 3, N
    ta.tape, ta.tape_bytes = 256, 1 << 40                      # never dereferenced: every call below is refused on host data
    return ta


def _scratch(lib, ta):
    cx = nat.TrainCompositePhaseArgs()
    cx.scratch, cx.scratch_bytes = 4096 * 256, lib.gnn_train_composite_phase_scratch_bytes(C.byref(ta))
    return cx


def test_layout_exports_and_version(lib):
    assert nat.GNN_ABI_VERSION == 10 and lib.gnn_abi_version() == 10
    assert C.sizeof(nat.TrainCompositePhaseArgs) == lib.gnn_struct_size(10) > 0
    assert C.sizeof(nat.TrainPhaseArgs) == lib.gnn_struct_size(8)                 # (the homogeneous block did not grow)
    for name in ('gnn_train_step_composite_ex', 'gnn_train_composite_phases_supported', 'gnn_train_composite_phase_scratch_bytes'):
        assert name in nat.EXPORTS and getattr(lib, name) is not None
    assert [f[0] for f in nat.TrainCompositePhaseArgs._fields_] == ['composite_adjacency_by_source', 'scratch', 'scratch_bytes']


def test_composite_phases_supported_reads_dims_only(lib, monkeypatch):
    ok = lambda **kw: lib.gnn_train_composite_phases_supported(C.byref(_composite_args(**kw)))
    for focus in 'nga':
        for d in (6, 5, 0, 16, 40):
            assert ok(d=d, focus=focus) == 0, (focus, d)          # the persistent small-graph path's dims
    assert ok(state_units=[12]) == 0                               # a hidden layer: the general path
    monkeypatch.setenv('GNN_TRAIN_SMALL', '0')
    assert ok() == 0                                               # ... and the general path by the switch
    monkeypatch.delenv('GNN_TRAIN_SMALL')
    assert ok(counts=(70, 0, 20)) == 0                             # a type with zero rows
    assert lib.gnn_train_composite_phase_scratch_bytes(C.byref(_composite_args())) > 0
    # not covered: homogeneous arguments, convergence groups, the forward alone, the row-streaming path, a very wide first state layer
    assert ok(composite=0) == -1
    ta = _composite_args(); ta.n_groups = 2
    assert lib.gnn_train_composite_phases_supported(C.byref(ta)) == -1
    ta = _composite_args(); ta.forward_only = 1
    assert lib.gnn_train_composite_phases_supported(C.byref(ta)) == -1
    assert ok(d=32, counts=(16384, 8192, 8191), n_arcs=70000) == 0     # 32 767 nodes: below the row-streaming threshold
    assert ok(d=32, counts=(16384, 8192, 8192), n_arcs=70000) == -1    # 32 768 nodes
    assert ok(state_units=[961]) == -1 and ok(state_units=[960]) == 0
    ta = _composite_args(); ta.loop.net_state[1].in_dim += 1        # dims that do not fit the graph: not covered either
    assert lib.gnn_train_composite_phases_supported(C.byref(ta)) == -1
    assert lib.gnn_train_composite_phases_supported(None) == -1
    for ta in (_composite_args(composite=0), _composite_args(d=32, counts=(16384, 8192, 8192), n_arcs=70000)):
        assert lib.gnn_train_composite_phase_scratch_bytes(C.byref(ta)) == 0
        assert lib.gnn_last_status() == nat.STATUS_NOT_COVERED and lib.gnn_last_error()


def test_the_pinned_entry_points_answer_as_before(lib):
    """`gnn_train_phases_supported`, `gnn_train_workspace_bytes` and `gnn_train_step_ex` on composite arguments: still -1, the tape of
    the plain step (the scratch is a buffer of its own), and the refusal that names homogeneous models."""
    ta = _composite_args()
    assert lib.gnn_train_phases_supported(C.byref(ta)) == -1
    nbytes = lib.gnn_train_workspace_bytes(C.byref(ta))
    assert nbytes > 0 and nbytes % 256 == 0
    ps = nat.TrainPhaseState()
    px = nat.TrainPhaseArgs(); px.phase, px.phase_state = nat.TRAIN_PHASE_FORWARD, C.pointer(ps)
    before = bytes(ta)
    assert lib.gnn_train_step_ex(C.byref(ta), C.byref(px)) != 0
    assert b'homogeneous' in lib.gnn_last_error() and lib.gnn_last_status() == nat.STATUS_NOT_COVERED
    assert bytes(ta) == before and ps.magic == 0
    assert lib.gnn_train_workspace_bytes(C.byref(ta)) == nbytes


def test_an_all_zero_block_is_the_plain_call(lib):
    def message(call):
        assert call() != 0
        return lib.gnn_last_status(), lib.gnn_last_error()
    cases = [_composite_args(), _composite_args(focus='a'), _composite_args(d=0), _composite_args(focus='g'), _composite_args(state_units=[12])]
    bad_dims = _composite_args(); bad_dims.loop.net_state[2].in_dim += 1
    bad_abi = _composite_args(); bad_abi.loop.abi_version = 9
    no_tape = _composite_args(); no_tape.tape = 0
    no_loss = _composite_args(); no_loss.loss_kind = nat.LOSS_NONE
    for ta in cases + [bad_dims, bad_abi, no_tape, no_loss]:
        plain = message(lambda: lib.gnn_train_step(C.byref(ta)))
        assert plain[1]
        assert message(lambda: lib.gnn_train_step_composite_ex(C.byref(ta), None, None)) == plain
        assert message(lambda: lib.gnn_train_step_composite_ex(C.byref(ta), C.byref(nat.TrainPhaseArgs()), None)) == plain
    assert b'in_dim' in message(lambda: lib.gnn_train_step_composite_ex(C.byref(bad_dims), None, None))[1]
    assert b'abi_version' in message(lambda: lib.gnn_train_step_composite_ex(C.byref(bad_abi), None, None))[1]


def _refused(lib, ta, px, cx, text, status):
    before = bytes(ta)
    assert lib.gnn_train_step_composite_ex(C.byref(ta), C.byref(px), None if cx is None else C.byref(cx)) != 0
    err = lib.gnn_last_error()
    assert text in err, err
    assert lib.gnn_last_status() == status, (lib.gnn_last_status(), err)
    assert bytes(ta) == before                                       # (nothing written back into the arguments)


def test_refused_calls_fail_with_a_status_before_any_launch(lib):
    """Every refusal is decided in front of the operand checks (the CSR arrays here are NULL: a call that got past them would complain
    about `adjacency`) and in front of the first launch."""
    NC, ERR = nat.STATUS_NOT_COVERED, nat.STATUS_ERROR
    ps = nat.TrainPhaseState()
    def fwd():
        px = nat.TrainPhaseArgs(); px.phase, px.phase_state = nat.TRAIN_PHASE_FORWARD, C.pointer(ps)
        return px
    ta = _composite_args()
    cx = _scratch(lib, ta)
    # ---- NOT_COVERED
    _refused(lib, _composite_args(composite=0), fwd(), cx, b'homogeneous models have gnn_train_step_ex', NC)
    t = _composite_args(); t.n_groups = 2
    _refused(lib, t, fwd(), cx, b'whole steps only', NC)
    t = _composite_args(); t.forward_only = 1
    _refused(lib, t, fwd(), cx, b'whole steps only', NC)
    _refused(lib, _composite_args(d=32, counts=(16384, 8192, 8192), n_arcs=70000), fwd(), cx, b'row-streaming', NC)
    _refused(lib, _composite_args(state_units=[961]), fwd(), cx, b'961 units', NC)
    px = nat.TrainPhaseArgs(); px.d_arc_labels = 4096
    _refused(lib, _composite_args(focus='a'), px, cx, b'arc-label gradient', NC)
    t = _composite_args(); t.drop_state[1].n, t.drop_state[1].pos[0], t.drop_state[1].rate[0] = 1, 0, 0.5
    _refused(lib, t, fwd(), cx, b'position 0', NC)
    # ---- ERROR
    _refused(lib, ta, fwd(), None, b'need cx->scratch', ERR)                       # phases without a scratch
    none = nat.TrainCompositePhaseArgs()
    _refused(lib, ta, fwd(), none, b'need cx->scratch', ERR)
    small = _scratch(lib, ta); small.scratch_bytes -= 1
    _refused(lib, ta, fwd(), small, b'scratch too small', ERR)
    px = nat.TrainPhaseArgs(); px.d_nodes = 4096                                   # label gradients of a whole step, no scratch
    _refused(lib, ta, px, None, b'need cx->scratch', ERR)
    _refused(lib, ta, px, cx, b'composite_adjacency_by_source[0]', ERR)            # ... a scratch, the by-source matrices missing
    two = _scratch(lib, ta)
    for q in (0, 1):
        c = two.composite_adjacency_by_source[q]
        c.n_dst, c.n_src, c.rowptr, c.src, c.nnz = 90, 90, 4096, 4096, 10
    _refused(lib, ta, px, two, b'composite_adjacency_by_source[2]', ERR)
    px = nat.TrainPhaseArgs(); px.phase = nat.TRAIN_PHASE_BACKWARD
    _refused(lib, ta, px, cx, b'needs phase_state', ERR)
    px = nat.TrainPhaseArgs(); px.phase, px.phase_state = nat.TRAIN_PHASE_BACKWARD, C.pointer(ps)
    _refused(lib, ta, px, cx, b'not filled by a phase-1 call', ERR)                # phase 2 without a phase-1 phase_state
    px = nat.TrainPhaseArgs(); px.d_nodes, px.ld_d_nodes = 4096, 3
    _refused(lib, ta, px, cx, b'ld_d_nodes', ERR)
    px = nat.TrainPhaseArgs(); px.phase = 3
    _refused(lib, ta, px, cx, b'unknown phase', ERR)
    t = _composite_args(); t.loss_kind = nat.LOSS_NONE
    px = nat.TrainPhaseArgs(); px.loss_scale = 0.5
    _refused(lib, t, px, cx, b'GNN_LOSS_NONE', ERR)
    assert ps.magic == 0 and ps.k == 0
    # a covered call gets past all of it: the operand checks speak next (still no launch: `adjacency` is NULL)
    before = bytes(ta)
    assert lib.gnn_train_step_composite_ex(C.byref(ta), C.byref(fwd()), C.byref(cx)) != 0
    assert b'adjacency' in lib.gnn_last_error() and bytes(ta) == before
