"""The rule of the hidden-layer form of the persistent small-graph training kernels (gnnkeras_amd/csrc/train_loop.hpp
`hidden_dense_of_state_width`, `homogeneous_train_path`; opt-in: GNN_FLAG_TRAIN_HIDDEN_SMALL in gnn_train_args_t::loop.flags) - no GPU:
`gnn_train_workspace_bytes` / `gnn_train_xc_applies` / `gnn_train_phases_supported` with fake device addresses, nothing launched.

The persistent path carves buffers of its own (padded tape rows, the hidden rows of every iteration, per-workgroup gradient shares), so
the tape's size tells the plans apart: on a covered shape the flag moves it, on every shape beyond the rule the flag changes nothing.
Without the flag nothing moves at all: that is tests/test_train_plan_host.py and its committed table."""
import ctypes as C
import os

import pytest

from gnnkeras_amd import _native as nat
from test_train_plan_host import FAKE, fill_grads, fill_mlp, make_args

TANH, SOFTMAX = nat.ACTIVATIONS['tanh'], nat.ACTIVATIONS['softmax']
COVERED = ((16, 16), (32, 20))                    # (state_dim, hidden units); the hidden form ships for the padded state widths 16 / 32
NODES = (1, 64, 16384)                            # one tile .. 256 tiles of 64 nodes (one per CU)


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(nat.LIB_PATH):
        nat.build()
    return nat.lib()


def hidden_args(d, units, n, flag, act=None, **kw):
    """`make_args` of the plan table with the state network replaced by Dense(units[0]) - .. - Dense(units[-1]) (tanh unless `act`)."""
    ta, keep = make_args(d, n, **kw)
    a = ta.loop
    if not a.composite:
        m = a.net_state[0]
        in_dim, bn = m.in_dim, bool(m.has_bn)
        C.memset(C.byref(m), 0, C.sizeof(m))
        fill_mlp(m, in_dim, list(units), list(act or [TANH] * len(units)), bn)
        fill_grads(ta.grad_state, m)
    a.flags = nat.FLAG_TRAIN_HIDDEN_SMALL if flag else 0
    return ta, keep


def answers(lib, ta):
    return (lib.gnn_train_workspace_bytes(C.byref(ta)), lib.gnn_train_xc_applies(C.byref(ta)), lib.gnn_train_phases_supported(C.byref(ta)))


def both(lib, d, units, n, **kw):
    on, off = hidden_args(d, units, n, True, **kw), hidden_args(d, units, n, False, **kw)
    return answers(lib, on[0]), answers(lib, off[0])


def test_the_flag_is_one_additive_bit():
    assert nat.FLAG_TRAIN_HIDDEN_SMALL == 1 << 8
    assert nat.FLAG_TRAIN_HIDDEN_SMALL & (nat.FLAG_UNFUSED | nat.FLAG_NO_EARLY_EXIT | nat.FLAG_FUSED_GEN_MASK) == 0
    assert nat.GNN_ABI_VERSION == 10


@pytest.mark.parametrize('d,H', COVERED)
@pytest.mark.parametrize('n', NODES)
@pytest.mark.parametrize('bn', (False, True))
def test_covered_shapes_plan_the_persistent_kernels(lib, d, H, n, bn):
    on, off = both(lib, d, [H, d], n, bn=bn)
    assert on[0] > 0 and off[0] > 0
    assert on[0] != off[0], (d, H, n)
    assert on[1] == off[1] == 0                   # (no constants line: that is the row-streaming path's)
    assert on[2] == off[2] == 0                   # the phases stay available


def test_covered_shapes_with_the_label_state_and_tiles(lib):
    """The starter shape (state_dim 0: 14 label columns padded to 16) with a hidden layer of 9 and of 14 units; a merged batch in tiles."""
    for H in (9, 14, 16):
        on, off = both(lib, 0, [H, 14], 200)
        assert on[0] != off[0] and on[2] == 0, H
    on, off = both(lib, 32, [20, 32], 16384, tiles=256)
    assert on[0] != off[0]


@pytest.mark.parametrize('name,d,units,n,kw', [
    ('H = SPs + 1 (d = 16)', 16, [17, 16], 64, {}),
    ('H = SPs + 1 (d = 32)', 32, [33, 32], 64, {}),
    ('padded width 64 (d = 64)', 64, [64, 64], 64, {}),
    ('padded width 64 (d = 40)', 40, [32, 40], 64, {}),
    ('H = SPs + 1 (label state, 14 -> 16)', 0, [17, 14], 64, {}),
    ('three layers', 16, [16, 16, 16], 64, {}),
    ('softmax on the hidden layer', 16, [16, 16], 64, dict(act=[SOFTMAX, TANH])),
    ('softmax on the state layer', 16, [16, 16], 64, dict(act=[TANH, SOFTMAX])),
    ('state dropout', 16, [16, 16], 64, dict(drop_state=True)),
    ('33 constant columns', 16, [16, 16], 64, dict(L=15)),
    ('257 tiles', 16, [16, 16], 16385, dict(tiles=257)),
    ('N = 32768', 16, [16, 16], 32768, {}),
    ('max_iteration = 0', 16, [16, 16], 64, dict(K=0)),
    ('composite', 16, [16, 16], 64, dict(composite=True, layers=2)),
])
def test_shapes_beyond_the_rule_plan_as_without_the_flag(lib, name, d, units, n, kw):
    on, off = both(lib, d, units, n, **kw)
    assert off[0] > 0, name
    assert on == off, name


def test_one_layer_models_do_not_see_the_flag(lib):
    for d in (0, 16, 64):
        for n in (64, 16384, 32768):
            on, off = both(lib, d, [d or 14], n)
            assert on == off and on[0] > 0, (d, n)


def test_the_knobs_of_the_persistent_path_hold_for_the_hidden_form(lib):
    """GNN_TRAIN_SMALL=0 and a node count at GNN_TRAIN_BIG_MIN_NODES keep the general kernels (both are read at every call)."""
    def with_env(name, value, fn):
        old = os.environ.get(name)
        os.environ[name] = value
        try: return fn()
        finally:
            if old is None: del os.environ[name]
            else: os.environ[name] = old
    on, off = with_env('GNN_TRAIN_SMALL', '0', lambda: both(lib, 16, [16, 16], 64))
    assert on == off
    on, off = with_env('GNN_TRAIN_BIG_MIN_NODES', '64', lambda: both(lib, 16, [16, 16], 64))
    assert on == off
    on, off = both(lib, 16, [16, 16], 64)
    assert on[0] != off[0]
