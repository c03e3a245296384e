"""The rule of the hidden-layer form of the one-CU-per-group kernels (gnnkeras_amd/csrc/loop_route.hpp `lds_hidden_asked`, `lds_covers`,
`lds_types_covers`; opt-in: GNN_FLAG_LDS_HIDDEN in gnn_loop_args_t::flags) - no GPU: `gnn_loop_route_name` / `gnn_loop_groups_supported` /
`gnn_loop_group_max_nodes` / the refusal of `gnn_loop_forward` with fake device addresses, nothing launched.

With the flag a state network Dense(H) - Dense(state width) on convergence groups answers 2 and names the hidden form; every shape
beyond the rule, and every shape without the flag, answers what it answered before: that half is tests/test_loop_route_host.py's
committed table, read here with the flag OR-ed into every one-layer case."""
import ctypes as C
import json
import os

import pytest

from gnnkeras_amd import _native as nat
from test_loop_route_host import A, FAKE, FLAGS, GROUPS, TABLE, decode, make_args, route_name, sections

TANH, SOFTMAX = nat.ACTIVATIONS['tanh'], nat.ACTIVATIONS['softmax']
HIDDEN, HIDDEN_TYPES = 'k_state_lds<.., hidden>', 'k_state_lds_types<.., hidden>'
COMPOSITE_REFUSAL = 'refused: convergence groups of a composite graph need the one-CU-per-group kernel (gnn_loop_groups_supported() != 2 for these args)'
FIT = GROUPS['fit'][0]                            # 3 groups of 100 / 80 / 120 nodes


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(nat.LIB_PATH):
        nat.build()
    lib = nat.lib()
    lib.gnn_loop_group_max_nodes.restype, lib.gnn_loop_group_max_nodes.argtypes = C.c_int, [C.POINTER(nat.LoopArgs)]
    return lib


def set_net(m, in_dim, units, acts):
    m.in_dim, m.n_layers = in_dim, len(units)
    for i in range(nat.GNN_MAX_LAYERS):
        m.units[i], m.activation[i], m.kernel[i], m.bias[i] = 0, 0, None, None
    for i, (u, act) in enumerate(zip(units, acts)): m.units[i], m.activation[i], m.kernel[i], m.bias[i] = u, act, FAKE, FAKE


def group_table(a, keep, node_begin, set_begin=None):
    keep.append((C.c_int32 * len(node_begin))(*node_begin))
    a.group_node_begin, a.n_groups = C.cast(keep[-1], C.c_void_p), len(node_begin) - 1
    a.n_nodes = a.adjacency.n_dst = a.adjacency.n_src = a.arcnode.n_dst = node_begin[-1]
    a.n_arcs = a.adjacency.nnz = a.arcnode.nnz = a.arcnode.n_src = 4 * a.n_nodes
    a.n_out = a.n_nodes
    if set_begin:
        keep.append((C.c_int32 * len(set_begin))(*set_begin))
        a.group_set_begin, a.n_group_sets = C.cast(keep[-1], C.c_void_p), len(set_begin) - 1


def homogeneous(d, units, flag, acts=None, labels=3, flags=0, node_begin=FIT, sets=None):
    """A homogeneous model with state network Dense(units[0]) - .. on a group table; d = 0: the state is the `labels` label columns."""
    a, keep = make_args(d or 16, node_begin[-1], flags=flags | (nat.FLAG_LDS_HIDDEN if flag else 0))
    S = d or labels
    a.state_dim, a.dim_node_label, a.ld_nodes = d, labels, labels
    set_net(a.net_state[0], 2 * S + 2 * labels + A if d else 2 * S + A, list(units), list(acts or [TANH] * len(units)))
    a.net_output.in_dim = S + labels if d else S
    group_table(a, keep, node_begin, sets)
    return a, keep


def composite(d, hidden, flag, acts=None, flags=0, node_begin=FIT, depth=None):
    """A composite model of len(hidden) node types, type t's state network Dense(hidden[t]) - Dense(d) (`depth`: layers per type)."""
    T, dims = len(hidden), [3] * len(hidden)
    a, keep = make_args(d, node_begin[-1], composite=True, flags=flags | (nat.FLAG_LDS_HIDDEN if flag else 0))
    a.n_types = T
    n = node_begin[-1]
    for t in range(T):
        layers = depth[t] if depth else 2
        units = [hidden[t]] * (layers - 1) + [d]
        set_net(a.net_state[t], dims[t] + 2 * d + sum(dims) + A, units, list(acts[t]) if acts else [TANH] * layers)
        a.type_dim_label[t], a.type_offsets[t + 1] = dims[t], n if t == T - 1 else (t + 1) * (n // T)
        a.composite_adjacency[t] = nat.CSR(n, n, 4 * n, FAKE, FAKE, None, None)
    group_table(a, keep, node_begin)
    return a, keep


def answers(lib, made):
    a, keep = made
    name, sup = route_name(lib, a), lib.gnn_loop_groups_supported(C.byref(a))
    status = None
    if name.startswith('refused: '):              # refused before the first launch: nothing touches a device
        assert lib.gnn_loop_forward(C.byref(a)) == 1 and lib.gnn_last_error().decode() == name[len('refused: '):]
        status = lib.gnn_last_status()
    return name, sup, status


def test_the_flag_is_one_additive_bit():
    assert nat.FLAG_LDS_HIDDEN == 1 << 9
    others = nat.FLAG_UNFUSED | nat.FLAG_NO_EARLY_EXIT | nat.FLAG_FUSED_GEN_MASK | nat.FLAG_TRAIN_HIDDEN_SMALL
    assert nat.FLAG_LDS_HIDDEN & others == 0
    assert nat.GNN_ABI_VERSION == 10


def test_the_library_knows_the_flag(lib):
    assert lib.gnn_abi_version() == 10
    assert answers(lib, homogeneous(16, [16, 16], True))[0] != answers(lib, homogeneous(16, [16, 16], False))[0]


HOMOGENEOUS = [(16, 16, 3), (6, 16, 3), (32, 20, 3), (32, 1, 3), (0, 9, 14)]       # (d, H, label columns)
COMPOSITE = [(5,), (5, 16, 9), (5, 16, 9, 5, 16, 9, 5, 16)]                        # H per type: 1, 3 and 8 types


@pytest.mark.parametrize('d,H,labels', HOMOGENEOUS)
def test_two_layer_groups_route_to_the_hidden_form_with_the_flag(lib, d, H, labels):
    S = d or labels
    assert answers(lib, homogeneous(d, [H, S], True, labels=labels)) == (HIDDEN, 2, None)
    assert answers(lib, homogeneous(d, [H, S], True, labels=labels, sets=[0, 3])) == (HIDDEN, 2, None)           # group sets too
    assert answers(lib, homogeneous(d, [H, S], True, labels=labels, flags=nat.FLAG_FUSED_GEN7)) == (HIDDEN, 2, None)


@pytest.mark.parametrize('d,H,labels', HOMOGENEOUS)
def test_two_layer_groups_without_the_flag_answer_as_before(lib, d, H, labels):
    """(passes before the flag existed: the spread form, answer 1 - and group sets refused)"""
    S = d or labels
    assert answers(lib, homogeneous(d, [H, S], False, labels=labels)) == ('k_state_small(setup_small)', 1, None)
    name, sup, status = answers(lib, homogeneous(d, [H, S], False, labels=labels, sets=[0, 3]))
    assert name.startswith('refused: convergence group sets need the one-CU-per-group form') and sup == 1 and status == 1


@pytest.mark.parametrize('hidden', COMPOSITE)
@pytest.mark.parametrize('d', (16, 32, 6))
def test_composite_two_layer_groups_route_to_the_hidden_form_with_the_flag(lib, d, hidden):
    hidden = [min(h, 16 if d <= 16 else 32) for h in hidden]
    assert answers(lib, composite(d, hidden, True)) == (HIDDEN_TYPES, 2, None)
    acts = [[nat.ACTIVATIONS[n] for n in pair] for pair in (('sigmoid', 'tanh'), ('relu', 'linear'), ('softplus', 'selu'))]
    assert answers(lib, composite(d, hidden, True, acts=[acts[t % 3] for t in range(len(hidden))])) == (HIDDEN_TYPES, 2, None)


@pytest.mark.parametrize('hidden', COMPOSITE)
def test_composite_two_layer_groups_without_the_flag_are_refused_as_before(lib, hidden):
    """(passes before the flag existed)"""
    assert answers(lib, composite(16, hidden, False)) == (COMPOSITE_REFUSAL, 0, nat.STATUS_NOT_COVERED)


def cap(lib, made):
    return lib.gnn_loop_group_max_nodes(C.byref(made[0]))


def beyond_the_rule():
    """name -> maker(flag): shapes the hidden form does not cover."""
    hom, comp = homogeneous, composite
    over = lambda make, **kw: (lambda flag: make(flag=flag, **kw))
    cases = {
        'H = SP + 1 (d = 16)': over(hom, d=16, units=[17, 16]),
        'H = SP + 1 (d = 32)': over(hom, d=32, units=[33, 32]),
        'H = SP + 1 (label state, 14 -> 16)': over(hom, d=0, units=[17, 14], labels=14),
        'padded width 64 (d = 64)': over(hom, d=64, units=[64, 64]),
        'padded width 64 (d = 40)': over(hom, d=40, units=[32, 40]),
        'softmax on the hidden layer': over(hom, d=16, units=[16, 16], acts=[SOFTMAX, TANH]),
        'softmax on the last layer': over(hom, d=16, units=[16, 16], acts=[TANH, SOFTMAX]),
        'three layers': over(hom, d=16, units=[16, 16, 16]),
        'one layer': over(hom, d=16, units=[16]),
        'GNN_FLAG_UNFUSED': over(hom, d=16, units=[16, 16], flags=nat.FLAG_UNFUSED),
        'composite: H = SP + 1': over(comp, d=16, hidden=[5, 17, 9]),
        'composite: padded width 64': over(comp, d=64, hidden=[5, 16, 9]),
        'composite: hidden softmax in one type': over(comp, d=16, hidden=[5, 16, 9], acts=[[TANH, TANH], [SOFTMAX, TANH], [TANH, TANH]]),
        'composite: last softmax in one type': over(comp, d=16, hidden=[5, 16, 9], acts=[[TANH, TANH], [TANH, TANH], [TANH, SOFTMAX]]),
        'composite: three layers': over(comp, d=16, hidden=[5, 16, 9], depth=[3, 3, 3]),
        'composite: mixed depth': over(comp, d=16, hidden=[16, 16, 16], depth=[2, 1, 2]),
        'composite: one layer': over(comp, d=16, hidden=[16, 16, 16], depth=[1, 1, 1]),
        'composite: GNN_FLAG_UNFUSED': over(comp, d=16, hidden=[5, 16, 9], flags=nat.FLAG_UNFUSED),
    }
    for gen in ('GEN2', 'GEN4', 'GEN5', 'GEN6'):
        cases[f'pinned to {gen}'] = over(hom, d=16, units=[16, 16], flags=FLAGS[gen])
        cases[f'composite: pinned to {gen}'] = over(comp, d=16, hidden=[5, 16, 9], flags=FLAGS[gen])
    return cases


@pytest.mark.parametrize('name', list(beyond_the_rule()))
def test_shapes_beyond_the_rule_answer_as_without_the_flag(lib, name):
    make = beyond_the_rule()[name]
    on, off = answers(lib, make(True)), answers(lib, make(False))
    assert on == off, name
    assert on[0] not in (HIDDEN, HIDDEN_TYPES) and on[0], name
    assert cap(lib, make(True)) == cap(lib, make(False)), name


def test_a_group_one_node_above_the_limit_answers_as_without_the_flag(lib):
    """The hidden form keeps W2 / b2 in the group's LDS: gnn_loop_group_max_nodes answers for the smaller budget when the flag is set on
    a two-layer model, a group of exactly that size takes the hidden form, one node more routes as without the flag."""
    for d, H in ((16, 16), (32, 20), (32, 1)):
        on, off = cap(lib, homogeneous(d, [H, d], True)), cap(lib, homogeneous(d, [H, d], False))
        assert 0 < on < off, (d, H)
        assert off - on <= -(-(d * d + d) * 4 // (4 * d + 16)) + 1, (d, H, on, off)      # W2 [d x d] + b2, in rows of a node's bytes
        at = [0, 100, 100 + on]
        assert answers(lib, homogeneous(d, [H, d], True, node_begin=at)) == (HIDDEN, 2, None)
        above = [0, 100, 101 + on]
        got, want = answers(lib, homogeneous(d, [H, d], True, node_begin=above)), answers(lib, homogeneous(d, [H, d], False, node_begin=above))
        assert got == want and got[0] != HIDDEN, (d, H, got, want)
    for d in (16, 32):
        for hidden in COMPOSITE:
            on, off = cap(lib, composite(d, hidden, True)), cap(lib, composite(d, hidden, False))
            assert 0 < on < off, (d, hidden)
            assert answers(lib, composite(d, hidden, True, node_begin=[0, 100, 100 + on])) == (HIDDEN_TYPES, 2, None)
            above = [0, 100, 101 + on]
            got, want = answers(lib, composite(d, hidden, True, node_begin=above)), answers(lib, composite(d, hidden, False, node_begin=above))
            assert got == want == (COMPOSITE_REFUSAL, 0, want[2]), (d, hidden, got, want)


def test_one_layer_cases_of_the_committed_table_do_not_see_the_flag(lib):
    """Every one-layer case of tests/golden/loop_routes.json with the flag OR-ed in gives the committed name (the reduced grid: the widths,
    node counts, flags and group tables on either side of every condition; the full cross is test_loop_route_host.py's, without the flag)."""
    with open(TABLE) as fh: want = decode(json.loads(fh.read()))
    full = sections()
    n = 0
    for s, lines in sections(reduced=True).items():
        for key, cases in lines.items():
            if ' net=1 ' not in key + ' ': continue
            assert key in full[s], (s, key)                                      # (the reduced grid is a part of the full one)
            for v, kw in cases:
                a, keep = make_args(**dict(kw, flags=kw['flags'] | nat.FLAG_LDS_HIDDEN))
                assert route_name(lib, a) == want[(s, key, str(v))], (s, key, v)
                n += 1
    for s in ('groups', 'composite groups'):                                     # ... and every one-layer group case of the full grid
        for key, cases in full[s].items():
            if ' net=1 ' not in key + ' ': continue
            for v, kw in cases:
                a, keep = make_args(**dict(kw, flags=kw['flags'] | nat.FLAG_LDS_HIDDEN))
                assert route_name(lib, a) == want[(s, key, str(v))], (s, key, v)
                n += 1
    assert n > 1000


def test_two_layer_cases_of_the_committed_table_move_only_to_the_hidden_form(lib):
    """The table's own two-layer group cases (H = d; 2w: H above the padded width; 3 layers) with the flag: a case either keeps the
    committed name, or the committed name was the spread form / a refusal for want of the one-CU-per-group kernel and it is now the hidden form."""
    with open(TABLE) as fh: want = decode(json.loads(fh.read()))
    moved = 0
    for s, hidden_name in (('groups', HIDDEN), ('composite groups', HIDDEN_TYPES)):
        for key, cases in sections()[s].items():
            if ' net=1 ' in key + ' ': continue
            for v, kw in cases:
                a, keep = make_args(**dict(kw, flags=kw['flags'] | nat.FLAG_LDS_HIDDEN))
                name, before = route_name(lib, a), want[(s, key, str(v))]
                if name == before: continue
                assert name == hidden_name and kw['net'] == '2' and not kw['soft'] and kw['d'] <= 32, (s, key, v, name)
                assert kw['flags'] in (0, nat.FLAG_FUSED_GEN7, nat.FLAG_NO_EARLY_EXIT) and 'heavy' not in kw['other'], (s, key, v)
                assert before == 'k_state_small(setup_small)' or before.startswith('refused: '), (s, key, v, before)
                assert lib.gnn_loop_groups_supported(C.byref(a)) == 2
                moved += 1
    assert moved > 0
