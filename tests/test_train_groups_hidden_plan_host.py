"""What the grouped training-mode forward answers for state networks with a hidden layer (gnnkeras_amd/csrc/train_group.hpp
`train_groups_hidden_net`; opt-in: GNN_FLAG_TRAIN_GROUPS_HIDDEN in gnn_train_args_t::loop.flags) - no GPU: `gnn_train_groups_supported`,
`gnn_train_workspace_bytes` and the refusals of `gnn_train_step` over widths, hidden widths, foci, BatchNormalization and both model
kinds, with the fake device addresses of tests/test_train_plan_host.py and nothing launched (`gnn_train_step` is only called on shapes the
rule refuses on host data).  The answers are pinned in tests/golden/train_group_hidden_plans.json.

    python tests/test_train_groups_hidden_plan_host.py FILE      writes the table of the library GNNKERAS_AMD_LIB names (default: the built one)

The rule: Dense(H) - Dense(S), 1 <= H <= the padded state width, padded width 16 or 32, no softmax, no Dropout, and every other condition
of the one-layer rule; a composite model's types all two-layered.  Without the flag - and with it on any other shape - nothing differs."""
import ctypes as C
import json
import os
import sys

import pytest

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gnnkeras_amd import _native as nat
from test_train_plan_host import DIMS, FAKE, dump, fill_grads, fill_mlp, make_args
from test_train_group_plan_host import TABLES, grouped_args, sections as one_layer_sections
import test_train_group_plan_host as one_layer

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'train_group_hidden_plans.json')
TANH, SIGMOID, SOFTMAX = nat.ACTIVATIONS['tanh'], nat.ACTIVATIONS['sigmoid'], nat.ACTIVATIONS['softmax']
OK, UNCOVERED = 0, nat.TRAIN_GROUPS_UNCOVERED
WIDTHS = (0, 8, 16, 17, 32)               # state_dim; 0: the state is the 14 label columns
KINDS = ('homogeneous', 'composite')


def padded(S): return 16 if S <= 16 else 32 if S <= 32 else 64


def hidden_args(d, kind, units=None, acts=None, flag=True, bn=False, focus='n', node_begin=TABLES['many groups'], L=14, drop=False, flags=0):
    """A grouped forward (tests/test_train_group_plan_host.py) whose state network(s) are Dense(units[0]) - .. - Dense(units[-1]).
    `units` / `acts`: one list for every type, or one list per type of a composite model (None: that type keeps its one Dense layer).
    A state of width 0 is the label matrix: `L` columns in both model kinds."""
    comp = kind == 'composite'
    n = node_begin[-1]
    ta, keep = make_args(d, n, composite=comp, bn=(bn, bn) if comp else bn, focus=focus, L=L)
    ta.forward_only, ta.k_groups = 1, FAKE
    out_begin = [(2 if focus == 'a' else 1) * v for v in node_begin]
    nb, ob = (C.c_int32 * len(node_begin))(*node_begin), (C.c_int32 * len(out_begin))(*out_begin)
    ta.group_node_begin, ta.group_out_begin, ta.n_groups = C.cast(nb, C.c_void_p), C.cast(ob, C.c_void_p), len(node_begin) - 1
    keep += [nb, ob]
    per_type = units is not None and len(units) > 0 and (units[0] is None or isinstance(units[0], (list, tuple)))
    for t in range(ta.loop.n_types):
        u = units[t] if per_type else units
        if u is None: continue
        a_ = (acts[t] if per_type else acts) if acts is not None else [TANH] * len(u)
        m = ta.loop.net_state[t]
        fill_mlp(m, m.in_dim, list(u), list(a_), bool(m.has_bn))
        fill_grads(ta.grad_state_types[t] if comp else ta.grad_state, m)
        if drop: ta.drop_state[t].n, ta.drop_state[t].pos[0], ta.drop_state[t].rate[0] = 1, 1, 0.5
    ta.loop.flags = flags | (nat.FLAG_TRAIN_GROUPS_HIDDEN if flag else 0)
    return ta, keep


def supported(lib, made): return lib.gnn_train_groups_supported(C.byref(made[0]))
def workspace(lib, made): return lib.gnn_train_workspace_bytes(C.byref(made[0]))


def refusal(lib, made):
    rc = lib.gnn_train_step(C.byref(made[0]))
    return [rc, lib.gnn_last_error().decode()]


def covered_cases():
    """{name: hidden_args keywords} - every one inside the rule."""
    out = {}
    for kind in KINDS:
        for d in WIDTHS:
            S = d or 14
            for H in sorted({1, S, padded(S)}):
                for focus in 'na':
                    for bn in (False, True):
                        out[f'{kind}: d={d} H={H}{" bn" if bn else ""} focus={focus}'] = dict(d=d, kind=kind, units=[H, S], bn=bn, focus=focus)
    # composite: H and both activations per type
    out['composite: d=16 H=(5, 16) activations per type'] = dict(d=16, kind='composite', units=[[5, 16], [16, 16]], acts=[[SIGMOID, TANH], [1, 0]])
    return out


def uncovered_cases():
    """{name: hidden_args keywords} - the flag is set, the rule says no."""
    out = {}
    for kind in KINDS:
        def case(name, **kw): out[f'{kind}: {name}'] = dict(dict(d=16, kind=kind, units=[16, 16]), **kw)
        case('H = padded width + 1 (d = 16)', units=[17, 16])
        case('H = padded width + 1 (d = 32)', d=32, units=[33, 32])
        case('H = padded width + 1 (label state, 14 -> 16)', d=0, units=[17, 14])
        case('softmax on the hidden layer', acts=[SOFTMAX, TANH])
        case('softmax on the last layer', acts=[TANH, SOFTMAX])
        case('three layers', units=[16, 16, 16])
        case('S = 33', d=33, units=[32, 33])
        case('S = 40 (padded width 64)', d=40, units=[32, 40])
        case('S = 64', d=64, units=[64, 64])
        case('state-network Dropout', drop=True)
        case('graph focus', focus='g')
    out['homogeneous: Kc = 33 (L = 15)'] = dict(d=16, kind='homogeneous', units=[16, 16], L=15)
    out['composite: one one-layer and one two-layer type'] = dict(d=16, kind='composite', units=[None, [16, 16]])
    out['composite: one two-layer and one one-layer type'] = dict(d=16, kind='composite', units=[[16, 16], None])
    out['composite: one type beyond the rule (H = 17)'] = dict(d=16, kind='composite', units=[[16, 16], [17, 16]])
    out['composite: softmax in one type'] = dict(d=16, kind='composite', units=[[16, 16], [16, 16]], acts=[[TANH, TANH], [SOFTMAX, TANH]])
    return out


def full_table(lib):
    """Covered: "bytes supported" with the flag | the same without.  Uncovered: the answer and gnn_train_step's refusal, with the flag."""
    table = {'covered': {}, 'uncovered': {}, 'without the flag': {}}
    for name, kw in covered_cases().items():
        on, off = hidden_args(**kw), hidden_args(**dict(kw, flag=False))
        table['covered'][name] = f'{workspace(lib, on)} {supported(lib, on)} | {workspace(lib, off)} {supported(lib, off)}'
    for name, kw in uncovered_cases().items():
        made = hidden_args(**kw)
        table['uncovered'][name] = [supported(lib, made)] + refusal(lib, made)
    for kind in KINDS:
        made = hidden_args(16, kind, [16, 16], flag=False)
        table['without the flag'][f'{kind}: d=16 H=16'] = [supported(lib, made)] + refusal(lib, made)
    return table


if __name__ == '__main__':
    if len(sys.argv) != 2: sys.exit('usage: python tests/test_train_groups_hidden_plan_host.py FILE')
    with open(sys.argv[1], 'w') as fh: fh.write(dump(full_table(nat.lib())))
    sys.exit(0)


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(nat.LIB_PATH):
        nat.build()
    return nat.lib()


def test_the_flag_is_a_bit_of_its_own():
    assert nat.FLAG_TRAIN_GROUPS_HIDDEN == 1 << 10
    others = nat.FLAG_UNFUSED | nat.FLAG_NO_EARLY_EXIT | nat.FLAG_FUSED_GEN_MASK | nat.FLAG_TRAIN_HIDDEN_SMALL | nat.FLAG_LDS_HIDDEN
    assert nat.FLAG_TRAIN_GROUPS_HIDDEN & others == 0


def test_train_flags_let_the_bit_through():
    from gnnkeras_amd.Models.training import _train_flags

    class M: native_flags = nat.FLAG_TRAIN_GROUPS_HIDDEN | nat.FLAG_UNFUSED | nat.FLAG_LDS_HIDDEN | nat.FLAG_FUSED_GEN7
    assert _train_flags(M) == nat.FLAG_TRAIN_GROUPS_HIDDEN
    M.native_flags |= nat.FLAG_TRAIN_HIDDEN_SMALL
    assert _train_flags(M) == nat.FLAG_TRAIN_GROUPS_HIDDEN | nat.FLAG_TRAIN_HIDDEN_SMALL        # (independent of each other)


@pytest.mark.parametrize('name', list(covered_cases()))
def test_covered_with_the_flag(lib, name):
    assert lib.gnn_abi_version() == 10                    # (additive: the ABI version does not move)
    assert supported(lib, hidden_args(**covered_cases()[name])) == OK, name


@pytest.mark.parametrize('name', list(covered_cases()))
def test_not_covered_without_the_flag(lib, name):
    """(passes before the flag existed)"""
    kw = covered_cases()[name]
    assert supported(lib, hidden_args(**dict(kw, flag=False))) == UNCOVERED, name
    assert supported(lib, hidden_args(**dict(kw, flag=False, flags=nat.FLAG_TRAIN_HIDDEN_SMALL | nat.FLAG_LDS_HIDDEN))) == UNCOVERED, name


@pytest.mark.parametrize('name', list(uncovered_cases()))
def test_still_uncovered_with_the_flag(lib, name):
    kw = uncovered_cases()[name]
    on, off = hidden_args(**kw), hidden_args(**dict(kw, flag=False))
    assert supported(lib, on) == supported(lib, off) == UNCOVERED, name
    assert workspace(lib, on) == workspace(lib, off), name
    got, want = refusal(lib, on), refusal(lib, off)
    assert got == want and got[0] == 1 and 'do not cover' in got[1], (name, got, want)
    assert lib.gnn_last_status() == nat.STATUS_NOT_COVERED, name


@pytest.mark.parametrize('kind', KINDS)
def test_a_group_of_257_nodes_still_answers_1(lib, kind):
    for d, H in ((16, 16), (0, 5), (32, 32)):
        S = d or 14
        assert supported(lib, hidden_args(d, kind, [H, S], node_begin=TABLES['a group of 257'])) == 1
        assert supported(lib, hidden_args(d, kind, [H, S], node_begin=TABLES['a group of 256'])) == OK
        assert supported(lib, hidden_args(d, kind, [H, S], node_begin=[0, 20, 300])) == 2


@pytest.mark.parametrize('kind', KINDS)
def test_the_workspace_is_that_of_the_one_layer_case(lib, kind):
    """Workspace bytes depend on the dims alone: Cc is [N][padded width] and H is at most that; h never leaves registers; no tape."""
    for d in WIDTHS:
        S = d or 14
        for focus in 'na':
            for bn in (False, True):
                for name, nb in TABLES.items():
                    one = workspace(lib, hidden_args(d, kind, None, bn=bn, focus=focus, node_begin=nb))
                    assert one > 0
                    for H in sorted({1, S, padded(S)}):
                        assert workspace(lib, hidden_args(d, kind, [H, S], bn=bn, focus=focus, node_begin=nb)) == one, (d, H, focus, bn, name)
                        assert workspace(lib, hidden_args(d, kind, [H, S], bn=bn, focus=focus, node_begin=nb, flag=False)) == one


def test_the_committed_one_layer_table_does_not_see_the_flag(lib):
    """Every case of tests/golden/train_group_plans.json recomputed with the flag OR-ed in equals the committed answer."""
    with open(one_layer.TABLE) as fh: want = json.loads(fh.read())
    n = 0
    for s, lines in one_layer_sections().items():
        for key, row in lines.items():
            for name, kw in row.items():
                ta, keep = grouped_args(**kw)
                ta.loop.flags |= nat.FLAG_TRAIN_GROUPS_HIDDEN
                assert one_layer.answers(lib, ta) == want[s][key][name], (s, key, name)
                n += 1
    for key, (ta, keep) in one_layer.malformed().items():
        ta.loop.flags |= nat.FLAG_TRAIN_GROUPS_HIDDEN
        assert one_layer.refusal(lib, ta) == want['malformed'][key], key
        n += 1
    assert n > 300


def test_the_answers_equal_the_committed_table(lib):
    with open(TABLE) as fh: golden = fh.read()
    table, want = full_table(lib), json.loads(golden)
    moved = [(s, k, want.get(s, {}).get(k), v) for s, lines in table.items() for k, v in lines.items() if want.get(s, {}).get(k) != v]
    assert not moved, f'{len(moved)} cases differ from the table (section, case, table, library); the first: {moved[:10]}'
    assert dump(table) == golden          # the file is what the generator writes: no stale line, no other order
    for name, row in table['covered'].items():
        on, off = row.split(' | ')
        assert on.split(' ')[1] == str(OK) and off.split(' ')[1] == str(UNCOVERED) and on.split(' ')[0] == off.split(' ')[0], (name, row)
