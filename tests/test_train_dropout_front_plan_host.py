"""The rule of Dropout in FRONT of a first Dense inside `gnn_train_step` (gnnkeras_amd/csrc/train_loop.hpp `check_dropout`,
`dropout_front_asked`, `homogeneous_train_path`; opt-in: GNN_FLAG_TRAIN_DROPOUT_FRONT in gnn_train_args_t::loop.flags) - no GPU:
`gnn_train_workspace_bytes` / `gnn_train_xc_applies` / `gnn_train_phases_supported` with fake device addresses, nothing launched.

With the flag a homogeneous model with ONE layer at position 0 of its state and / or output network plans the general kernels, with the
normalised, dropped-out input X0 [rows x in_dim] of every such network in the workspace, and has no phases.  Without the flag position 0
stays refused (tests/test_train_dropout_plan_host.py::test_position_0_is_still_refused), and a model without such a layer never sees the
flag."""
import contextlib
import ctypes as C
import os

import pytest

from gnnkeras_amd import _native as nat
from test_train_plan_host import fill_grads, fill_mlp, make_args
from test_train_dropout_plan_host import answers, drop_args

TANH = nat.ACTIVATIONS['tanh']
FRONT = nat.FLAG_TRAIN_DROPOUT_FRONT
SMALL = nat.FLAG_TRAIN_DROPOUT_SMALL | nat.FLAG_TRAIN_HIDDEN_SMALL
L, A = 14, 3


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(nat.LIB_PATH):
        nat.build()
    return nat.lib()


def front_args(d, n, flags, units=None, pos=(0,), state=True, output=False, out_units=None, **kw):
    """`drop_args` (rate 0.5, state network Dense(units[0]) - .. tanh) with the layers of the state network at `pos` (`state`), one layer
    at position 0 of the output network (`output`), the output network replaced by Dense(out_units[0]) - .. (`out_units`)."""
    ta, keep = drop_args(d, n, flags, units=units, pos=pos, state_drop=state, **kw)
    a = ta.loop
    if out_units is not None:
        m = a.net_output
        in_dim, bn = m.in_dim, bool(m.has_bn)
        C.memset(C.byref(m), 0, C.sizeof(m))
        fill_mlp(m, in_dim, list(out_units), [TANH] * len(out_units), bn)
        fill_grads(ta.grad_output, m)
    if output:
        do = ta.drop_output
        do.n, do.net_id, do.pos[0], do.index[0], do.rate[0] = 1, 1000, 0, 0, 0.5
    return ta, keep


@contextlib.contextmanager
def general_only():
    """GNN_TRAIN_SMALL=0 and an unreachable GNN_TRAIN_BIG_MIN_NODES: every plan takes the general kernels."""
    knobs = {'GNN_TRAIN_SMALL': '0', 'GNN_TRAIN_BIG_MIN_NODES': str(1 << 30)}
    old = {k: os.environ.get(k) for k in knobs}
    os.environ.update(knobs)
    try: yield
    finally:
        for k, v in old.items():
            if v is None: del os.environ[k]
            else: os.environ[k] = v


def in_dims(d):
    S = d if d > 0 else L
    return (2 * S + 2 * L + A if d > 0 else 2 * S + A), (S + L if d > 0 else S)      # state network, output network (node focus)


def test_the_flag_is_one_additive_bit():
    assert FRONT == 1 << 12
    others = (nat.FLAG_UNFUSED | nat.FLAG_NO_EARLY_EXIT | nat.FLAG_FUSED_GEN_MASK | nat.FLAG_TRAIN_HIDDEN_SMALL | nat.FLAG_LDS_HIDDEN |
              nat.FLAG_TRAIN_GROUPS_HIDDEN | nat.FLAG_TRAIN_DROPOUT_SMALL)
    assert FRONT & others == 0
    assert nat.GNN_ABI_VERSION == 10


def test_train_flags_let_the_bit_through():
    from gnnkeras_amd.Models.training import _train_flags

    class M: native_flags = FRONT | nat.FLAG_UNFUSED | nat.FLAG_LDS_HIDDEN | nat.FLAG_FUSED_GEN7
    assert _train_flags(M) == FRONT
    M.native_flags |= SMALL | nat.FLAG_TRAIN_GROUPS_HIDDEN
    assert _train_flags(M) == FRONT | SMALL | nat.FLAG_TRAIN_GROUPS_HIDDEN


@pytest.mark.parametrize('where', ('state', 'output', 'both'))
@pytest.mark.parametrize('units,pos', ((None, (0,)), ([16, 16], (0,)), ([16, 16], (0, 1))))
@pytest.mark.parametrize('bn', (False, True))
@pytest.mark.parametrize('n', (64, 16384, 32768))
def test_position_0_plans_the_general_path(lib, where, units, pos, bn, n):
    """(workspace > 0, no constants line, no phases); the workspace exceeds that of the same networks without the layer(s) at position 0
    by X0 of every network that has one - at least N x in_dim floats each; the persistent kernels' flags change nothing."""
    d = 16
    state, output = where in ('state', 'both'), where in ('output', 'both')
    kw = dict(units=units, bn=bn, output=output)
    pos_s = pos if state else tuple(q for q in pos if q != 0)
    got = answers(lib, front_args(d, n, FRONT, pos=pos_s, state=bool(pos_s), **kw)[0])
    assert got[0] > 0 and got[1] == 0 and got[2] == -1, got
    assert answers(lib, front_args(d, n, FRONT | SMALL, pos=pos_s, state=bool(pos_s), **kw)[0]) == got      # never the persistent path
    # the same networks without the layers at position 0, kept on the general kernels by the knobs of the two fast paths (read at every
    # call) - which the position-0 plan does not see at all
    rest = tuple(q for q in pos_s if q != 0)
    with general_only():
        assert answers(lib, front_args(d, n, FRONT, pos=pos_s, state=bool(pos_s), **kw)[0]) == got
        plain = answers(lib, front_args(d, n, FRONT, units=units, bn=bn, pos=rest or (1,), state=bool(rest), output=False)[0])
    in_s, in_o = in_dims(d)
    extra = 4 * n * ((in_s if state else 0) + (in_o if output else 0))
    assert plain[0] > 0 and got[0] - plain[0] >= extra, (got[0], plain[0], extra)


@pytest.mark.parametrize('name,d,n,kw', [
    ('two layers at position 0 (state)', 16, 64, dict(pos=(0, 0))),
    ('two layers at position 0 (state, hidden)', 16, 64, dict(units=[16, 16], pos=(0, 0, 1))),
    ('composite', 16, 64, dict(composite=True)),
])
def test_beyond_the_rule_stays_not_covered(lib, name, d, n, kw):
    ta, keep = front_args(d, n, FRONT, **kw)
    if kw.get('composite'):
        for t in range(ta.loop.n_types): ta.drop_state[t].n, ta.drop_state[t].pos[0], ta.drop_state[t].rate[0] = 1, 0, 0.5
        assert lib.gnn_train_workspace_bytes(C.byref(ta)) == 0, name
    else:
        assert answers(lib, ta) == (0, 0, -1), name
        assert lib.gnn_train_workspace_bytes(C.byref(ta)) == 0
    assert lib.gnn_last_status() == nat.STATUS_NOT_COVERED and b'position 0' in lib.gnn_last_error(), name


def test_two_layers_at_position_0_of_the_output_network(lib):
    ta, keep = front_args(16, 64, FRONT, state=False, output=True)
    do = ta.drop_output
    do.n, do.pos[1], do.index[1], do.rate[1] = 2, 0, 1, 0.5
    assert lib.gnn_train_workspace_bytes(C.byref(ta)) == 0
    assert lib.gnn_last_status() == nat.STATUS_NOT_COVERED and b'position 0' in lib.gnn_last_error()


def test_convergence_groups_stay_not_covered(lib):
    """A grouped training-mode forward (n_groups > 0) refuses position 0 with the flag as without it."""
    for flags in (0, FRONT):
        ta, keep = front_args(16, 64, flags)
        gb, ob = (C.c_int32 * 3)(0, 32, 64), (C.c_int32 * 3)(0, 32, 64)
        ta.forward_only, ta.n_groups = 1, 2
        ta.group_node_begin, ta.group_out_begin = C.addressof(gb), C.addressof(ob)
        assert lib.gnn_train_workspace_bytes(C.byref(ta)) == 0, flags
        assert lib.gnn_last_status() == nat.STATUS_NOT_COVERED, flags
        assert lib.gnn_train_phases_supported(C.byref(ta)) == -1


def test_a_phase_block_is_refused_before_anything_runs(lib):
    """`gnn_train_step_ex` with a phase block on a covered position-0 model: "not covered" on host data (fake addresses: a launch would fault)."""
    ta, keep = front_args(16, 64, FRONT)
    ps, px = nat.TrainPhaseState(), nat.TrainPhaseArgs()
    px.phase, px.phase_state = nat.TRAIN_PHASE_FORWARD, C.pointer(ps)
    assert lib.gnn_train_step_ex(C.byref(ta), C.byref(px)) != 0
    assert lib.gnn_last_status() == nat.STATUS_NOT_COVERED and b'GNN_FLAG_TRAIN_DROPOUT_FRONT' in lib.gnn_last_error()


def test_models_without_a_layer_at_position_0_do_not_see_the_flag(lib):
    for d in (0, 16, 64):
        for n in (64, 16384, 32768):
            for kw in (dict(state=False), dict(pos=(1,)), dict(units=[16, d or 14], pos=(1,)), dict(units=[16, d or 14], pos=(1, 2), bn=True),
                       dict(state=False, drop_output=True)):
                for base in (0, SMALL):
                    on, off = answers(lib, front_args(d, n, base | FRONT, **kw)[0]), answers(lib, front_args(d, n, base, **kw)[0])
                    assert on == off and on[0] > 0, (d, n, kw, base)
