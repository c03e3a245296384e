"""Host side of the phased training step (`gnn_train_step_ex`, additive to C ABI 10) - no GPU: struct layouts and exports through
`_native`, `gnn_train_phases_supported` on covered / uncovered dims, an all-zero second argument block against the plain call, and the
calls the library refuses before its first launch (every refusal below is decided from host data: dims, network descriptions, NULLs)."""
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


def _train_args(d=8, L=14, A=3, T=2, n_nodes=200, n_arcs=420, n_out=200, focus='n', state_units=None, composite=0):
    ta = nat.TrainArgs()
    a = ta.loop
    a.abi_version, a.n_types, a.composite = nat.GNN_ABI_VERSION, 1, composite
    a.n_nodes, a.n_arcs, a.dim_node_label, a.dim_arc_label = n_nodes, n_arcs, L, A
    a.state_dim, a.max_iteration, a.state_threshold = d, 4, 0.01
    S = d if d > 0 else L
    units = list(state_units or []) + [S]
    m = a.net_state[0]
    m.in_dim, m.n_layers = (2 * S + 2 * L + A if d > 0 else 2 * S + A), len(units)
    for i, u in enumerate(units): m.units[i], m.activation[i], m.kernel[i], m.bias[i] = u, 3, 4096, 4096      # (fake device addresses)
    o = a.net_output
    node_part = S + L if d > 0 else S
    o.in_dim, o.n_layers = (2 * node_part + A if focus == 'a' else node_part), 1
    o.units[0], o.activation[0], o.kernel[0], o.bias[0] = T, 7, 4096, 4096
    a.focus, a.n_out = nat.FOCUS[focus], n_out
    if focus == 'g': a.nodegraph.n_dst, a.nodegraph.n_src = 12, n_out
    ta.tape, ta.tape_bytes = 256, 1 << 40                      # never dereferenced: every call below is refused on host data
    return ta


def test_layouts_exports_and_version(lib):
    assert nat.GNN_ABI_VERSION == 10 and lib.gnn_abi_version() == 10
    assert C.sizeof(nat.TrainArgs) == lib.gnn_struct_size(4)
    assert C.sizeof(nat.TrainPhaseArgs) == lib.gnn_struct_size(8)
    assert C.sizeof(nat.TrainPhaseState) == lib.gnn_struct_size(9)
    for name in ('gnn_train_step_ex', 'gnn_train_phases_supported', 'gnn_gate_all'):
        assert name in nat.EXPORTS and getattr(lib, name) is not None
    assert (nat.TRAIN_PHASE_FORWARD, nat.TRAIN_PHASE_BACKWARD, nat.LOSS_NONE) == (1, 2, -1)
    names = [f[0] for f in nat.TrainPhaseArgs._fields_]
    assert names == ['phase', 'loss_scale', 'phase_state', 'node_out', 'd_pred_extra', 'd_out_extra', 'd_state_extra', 'd_nodes', 'ld_d_nodes',
                     'd_arc_labels', 'arcnode_by_source']


def test_an_all_zero_block_is_the_plain_call(lib):
    """The same argument checks, in the same order, with the same messages: no block, an all-zero block, and `gnn_train_step`."""
    def message(call):
        assert call() != 0
        return lib.gnn_last_error()
    cases = [_train_args(), _train_args(focus='a', n_out=300), _train_args(d=0), _train_args(focus='g')]
    bad_dims = _train_args(); bad_dims.loop.net_state[0].in_dim += 1
    bad_abi = _train_args(); bad_abi.loop.abi_version = 9
    no_tape = _train_args(); no_tape.tape = 0
    for ta in cases + [bad_dims, bad_abi, no_tape]:
        plain = message(lambda: lib.gnn_train_step(C.byref(ta)))
        assert plain
        assert message(lambda: lib.gnn_train_step_ex(C.byref(ta), None)) == plain
        assert message(lambda: lib.gnn_train_step_ex(C.byref(ta), C.byref(nat.TrainPhaseArgs()))) == plain
    assert b'in_dim' in message(lambda: lib.gnn_train_step(C.byref(bad_dims)))
    assert b'abi_version' in message(lambda: lib.gnn_train_step(C.byref(bad_abi)))


def test_phases_supported_reads_dims_only(lib):
    ok = lambda **kw: lib.gnn_train_phases_supported(C.byref(_train_args(**kw)))
    # the MUTAG shapes of the joint-step tests: 12 graphs, about 200 nodes; layer 0 and the wider label matrices of the layers above it
    for focus in 'nag':
        for d, L, A in ((8, 14, 3), (8, 24, 3), (8, 22, 3), (0, 14, 3), (0, 30, 3), (0, 46, 3), (6, 20, 3), (6, 14, 7), (16, 14, 3), (40, 14, 3)):
            assert ok(d=d, L=L, A=A, focus=focus, n_out=420 if focus == 'a' else 200) == 0, (focus, d, L, A)
    assert ok(state_units=[12]) == 0                                # a two-layer state network: the general kernels
    assert ok(n_nodes=32767, n_arcs=70000, n_out=32767, d=16) == 0  # below the row-streaming threshold
    # not covered: composite models, convergence groups, the forward alone, the row-streaming path, a very wide first state layer
    assert ok(composite=1) == -1
    assert ok(n_nodes=32768, n_arcs=70000, n_out=32768, d=16) == -1
    assert ok(n_nodes=131072, n_arcs=300000, n_out=131072, d=32) == -1
    assert ok(state_units=[961]) == -1 and ok(state_units=[960]) == 0
    ta = _train_args(); ta.forward_only = 1
    assert lib.gnn_train_phases_supported(C.byref(ta)) == -1
    ta = _train_args(); ta.n_groups = 2
    assert lib.gnn_train_phases_supported(C.byref(ta)) == -1
    ta = _train_args(); ta.loop.net_state[0].in_dim += 1              # dims that do not fit the graph: not covered either
    assert lib.gnn_train_phases_supported(C.byref(ta)) == -1
    assert lib.gnn_train_phases_supported(None) == -1


def _refused(lib, ta, px, text):
    before = bytes(ta)
    assert lib.gnn_train_step_ex(C.byref(ta), C.byref(px)) != 0
    err = lib.gnn_last_error()
    assert text in err, err
    assert bytes(ta) == before                                       # (nothing written back into the arguments)
    return err


def test_refused_calls_fail_with_a_message_before_any_launch(lib):
    """Each refusal comes from `check_phase_args`, which runs in front of the operand checks (the CSR arrays here are NULL: a call that got
    past it would complain about `adjacency`) and in front of the first launch."""
    k = C.c_int32(-7)
    ps = nat.TrainPhaseState()
    # phase 2 without phase_state
    px = nat.TrainPhaseArgs(); px.phase = nat.TRAIN_PHASE_BACKWARD
    _refused(lib, _train_args(), px, b'needs phase_state')
    px = nat.TrainPhaseArgs(); px.phase = nat.TRAIN_PHASE_FORWARD
    _refused(lib, _train_args(), px, b'needs phase_state')
    # ... or with one no phase-1 call has filled
    px = nat.TrainPhaseArgs(); px.phase, px.phase_state = nat.TRAIN_PHASE_BACKWARD, C.pointer(ps)
    _refused(lib, _train_args(), px, b'not filled by a phase-1 call')
    # GNN_LOSS_NONE in a whole step
    ta = _train_args(); ta.loss_kind = nat.LOSS_NONE
    _refused(lib, ta, nat.TrainPhaseArgs(), b'GNN_LOSS_NONE')
    ta = _train_args(); ta.loss_kind = nat.LOSS_NONE
    assert lib.gnn_train_step(C.byref(ta)) != 0 and b'GNN_LOSS_NONE' in lib.gnn_last_error()
    # d_arc_labels without arcnode_by_source
    px = nat.TrainPhaseArgs(); px.d_arc_labels = 4096
    _refused(lib, _train_args(focus='a', n_out=300), px, b'arcnode_by_source')
    # an unknown phase; a leading dimension below the label width; phases on what they do not cover
    px = nat.TrainPhaseArgs(); px.phase = 3
    _refused(lib, _train_args(), px, b'unknown phase')
    px = nat.TrainPhaseArgs(); px.d_nodes, px.ld_d_nodes = 4096, 13
    _refused(lib, _train_args(), px, b'ld_d_nodes')
    px = nat.TrainPhaseArgs(); px.phase, px.phase_state = nat.TRAIN_PHASE_FORWARD, C.pointer(ps)
    _refused(lib, _train_args(composite=1), px, b'homogeneous')
    ta = _train_args(); ta.forward_only = 1
    _refused(lib, ta, px, b'homogeneous')
    _refused(lib, _train_args(n_nodes=32768, n_arcs=70000, n_out=32768, d=16), px, b'row-streaming')
    assert k.value == -7 and ps.magic == 0 and ps.k == 0
