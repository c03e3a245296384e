"""The rule of the Dropout form of the persistent small-graph training kernels (gnnkeras_amd/csrc/train_loop.hpp `dropout_small_form`,
`homogeneous_train_path`; opt-in: GNN_FLAG_TRAIN_DROPOUT_SMALL in gnn_train_args_t::loop.flags, independent of
GNN_FLAG_TRAIN_HIDDEN_SMALL) - no GPU: `gnn_train_workspace_bytes` / `gnn_train_xc_applies` / `gnn_train_phases_supported` with fake
device addresses, nothing launched.

The persistent path carves buffers of its own (padded tape rows, per-workgroup gradient shares, the un-dropped output of a Dropout layer
behind the last Dense), so the tape's size tells the plans apart: on a covered shape the flag moves it, on every shape beyond the rule the
flag changes nothing.  Without the flag nothing moves at all: tests/test_train_plan_host.py, tests/test_train_hidden_plan_host.py."""
import ctypes as C
import os

import pytest

from gnnkeras_amd import _native as nat
from test_train_plan_host import fill_grads, fill_mlp, make_args

TANH = nat.ACTIVATIONS['tanh']
DROP, HIDDEN = nat.FLAG_TRAIN_DROPOUT_SMALL, nat.FLAG_TRAIN_HIDDEN_SMALL
NODES = (1, 64, 16384)                            # one tile .. 256 tiles of 64 nodes (one per CU)


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(nat.LIB_PATH):
        nat.build()
    return nat.lib()


def drop_args(d, n, flags, units=None, pos=(1,), state_drop=True, **kw):
    """`make_args` of the plan table (one Dropout layer of rate 0.5 at position 1 of the state network) with flags `flags`; `units`: the state
    network replaced by Dense(units[0]) - .. - Dense(units[-1]) (tanh); `pos`: the positions of its Dropout layers, in list order."""
    ta, keep = make_args(d, n, drop_state=state_drop, **kw)
    a = ta.loop
    if units is not None and not a.composite:
        m = a.net_state[0]
        in_dim, bn = m.in_dim, bool(m.has_bn)
        C.memset(C.byref(m), 0, C.sizeof(m))
        fill_mlp(m, in_dim, list(units), [TANH] * len(units), bn)
        fill_grads(ta.grad_state, m)
    if state_drop and not a.composite:
        ds = ta.drop_state[0]
        ds.n = len(pos)
        for i, q in enumerate(pos): ds.pos[i], ds.index[i], ds.rate[i] = q, i, 0.5
    a.flags = flags
    return ta, keep


def answers(lib, ta):
    return (lib.gnn_train_workspace_bytes(C.byref(ta)), lib.gnn_train_xc_applies(C.byref(ta)), lib.gnn_train_phases_supported(C.byref(ta)))


def both(lib, d, n, flags=DROP, **kw):
    """(with `flags`, with `flags` less the Dropout bit)"""
    on, off = drop_args(d, n, flags, **kw), drop_args(d, n, flags & ~DROP, **kw)
    return answers(lib, on[0]), answers(lib, off[0])


def test_the_flag_is_one_additive_bit():
    assert DROP == 1 << 11
    others = (nat.FLAG_UNFUSED | nat.FLAG_NO_EARLY_EXIT | nat.FLAG_FUSED_GEN_MASK | nat.FLAG_TRAIN_HIDDEN_SMALL | nat.FLAG_LDS_HIDDEN |
              nat.FLAG_TRAIN_GROUPS_HIDDEN)
    assert DROP & others == 0
    assert nat.GNN_ABI_VERSION == 10


def test_train_flags_let_the_bit_through():
    from gnnkeras_amd.Models.training import _train_flags

    class M: native_flags = DROP | nat.FLAG_UNFUSED | nat.FLAG_LDS_HIDDEN | nat.FLAG_FUSED_GEN7
    assert _train_flags(M) == DROP
    M.native_flags |= HIDDEN
    assert _train_flags(M) == DROP | HIDDEN                       # (independent of each other)


@pytest.mark.parametrize('d', (16, 32, 0, 20))                    # 0: the 14 label columns padded to 16; 20: padded to 32
@pytest.mark.parametrize('n', NODES)
@pytest.mark.parametrize('bn', (False, True))
def test_one_layer_with_dropout_behind_it_plans_the_persistent_kernels(lib, d, n, bn):
    on, off = both(lib, d, n, bn=bn)
    assert on[0] > 0 and off[0] > 0
    assert on[0] != off[0], (d, n)
    assert on[1] == off[1] == 0                   # (no constants line: that is the row-streaming path's)
    assert on[2] == off[2] == 0                   # the phases stay available


def test_covered_shapes_with_tiles(lib):
    on, off = both(lib, 32, 16384, tiles=256)
    assert on[0] != off[0] and on[2] == 0
    on, off = both(lib, 32, 16384, flags=DROP | HIDDEN, units=[20, 32], pos=(1, 2), tiles=256)
    assert on[0] != off[0] and on[2] == 0


@pytest.mark.parametrize('d,H', ((16, 16), (32, 20)))
@pytest.mark.parametrize('pos', ((1,), (2,), (1, 2)))
@pytest.mark.parametrize('n', NODES)
def test_hidden_networks_with_both_flags(lib, d, H, pos, n):
    """Both flags: Dropout between the two Dense layers, behind the second, or both.  The HIDDEN flag alone keeps such a network on the
    general kernels (its own test pins that), so the flag-off answer here IS the general plan's."""
    on, off = both(lib, d, n, flags=DROP | HIDDEN, units=[H, d], pos=pos)
    assert on[0] > 0 and off[0] > 0 and on[0] != off[0], (d, H, pos, n)
    assert off == answers(lib, drop_args(d, n, 0, units=[H, d], pos=pos)[0])
    assert on[1] == 0 and on[2] == 0


def test_a_layer_behind_the_last_dense_tapes_its_input(lib):
    """The un-dropped output is one more [K][N][ldS] array, carved only when a layer sits behind the last Dense."""
    mid = answers(lib, drop_args(32, 64, DROP | HIDDEN, units=[32, 32], pos=(1,))[0])[0]
    last = answers(lib, drop_args(32, 64, DROP | HIDDEN, units=[32, 32], pos=(2,))[0])[0]
    assert last > mid > 0
    assert abs((last - mid) - 4 * 64 * 32 * 4) <= 256    # K = 4 iterations x 64 nodes x 32 floats (the Dropout buffers of the general plan are the same size at either position)


@pytest.mark.parametrize('name,d,n,kw', [
    ('padded width 64 (d = 64)', 64, 64, {}),
    ('padded width 64 (d = 40)', 40, 64, {}),
    ('two Dropout layers at one position', 16, 64, dict(pos=(1, 1))),
    ('two Dropout layers at one position (hidden, both flags)', 16, 64, dict(flags=DROP | HIDDEN, units=[16, 16], pos=(1, 2, 2))),
    ('a hidden network without the HIDDEN flag', 16, 64, dict(units=[16, 16], pos=(1,))),
    ('a hidden network without the HIDDEN flag (position 2)', 32, 64, dict(units=[20, 32], pos=(2,))),
    ('a hidden layer wider than the padded width (both flags)', 16, 64, dict(flags=DROP | HIDDEN, units=[17, 16], pos=(1,))),
    ('three layers (both flags)', 16, 64, dict(flags=DROP | HIDDEN, units=[16, 16, 16], pos=(1,))),
    ('33 constant columns', 16, 64, dict(L=15)),
    ('257 tiles', 16, 16385, dict(tiles=257)),
    ('N = 32768', 16, 32768, {}),
    ('max_iteration = 0', 16, 64, dict(K=0)),
    ('composite', 16, 64, dict(composite=True)),
])
def test_shapes_beyond_the_rule_plan_as_without_the_flag(lib, name, d, n, kw):
    on, off = both(lib, d, n, **kw)
    assert off[0] > 0, name
    assert on == off, name


def test_position_0_is_still_refused(lib):
    for flags in (0, DROP, DROP | HIDDEN):
        ta, keep = drop_args(16, 64, flags, pos=(0,))
        assert answers(lib, ta) == (0, 0, -1), flags
        assert lib.gnn_last_status() == nat.STATUS_NOT_COVERED and b'position 0' in lib.gnn_last_error(), flags
        ta, keep = drop_args(16, 64, flags, units=[16, 16], pos=(0, 1))
        assert answers(lib, ta) == (0, 0, -1), flags


def test_models_without_state_dropout_do_not_see_the_flag(lib):
    for d in (0, 16, 64):
        for n in (64, 16384, 32768):
            on, off = both(lib, d, n, state_drop=False)
            assert on == off and on[0] > 0, (d, n)
            on, off = both(lib, d, n, flags=DROP | HIDDEN, units=[16, d or 14], state_drop=False)
            assert on == off and on[0] > 0, (d, n)
            on, off = both(lib, d, n, state_drop=False, drop_output=True)
            assert on == off and on[0] > 0, (d, n)


def test_the_knobs_of_the_persistent_path_hold_for_the_dropout_form(lib):
    """GNN_TRAIN_SMALL=0 and a node count at GNN_TRAIN_BIG_MIN_NODES keep the general kernels (both are read at every call)."""
    def with_env(name, value, fn):
        old = os.environ.get(name)
        os.environ[name] = value
        try: return fn()
        finally:
            if old is None: del os.environ[name]
            else: os.environ[name] = old
    for kw in ({}, dict(flags=DROP | HIDDEN, units=[16, 16], pos=(1, 2))):
        on, off = with_env('GNN_TRAIN_SMALL', '0', lambda: both(lib, 16, 64, **kw))
        assert on == off
        on, off = with_env('GNN_TRAIN_BIG_MIN_NODES', '64', lambda: both(lib, 16, 64, **kw))
        assert on == off
        on, off = both(lib, 16, 64, **kw)
        assert on[0] != off[0]
