"""What the grouped training-mode forward (`gnn_train_step(forward_only)` with convergence groups; gnnkeras_amd/csrc/train_group.hpp) plans
and refuses for both model kinds - no GPU: `gnn_train_workspace_bytes` and `gnn_train_groups_supported` over state widths, BatchNormalization,
foci and group tables, with fake device addresses and nothing launched, against the committed table tests/golden/train_group_plans.json.
Both kinds carve their own workspace and share their checks: the malformed calls record the return code and the message of
`gnn_train_step`, every one refused on host data before a launch, and the cases with two faults at once pin the order of refusal.

    python tests/test_train_group_plan_host.py FILE      writes the table of the library GNNKERAS_AMD_LIB names (default: the built one)

A line of a section is one case but for the group table: "d=16 bn focus=a: {"one group": "bytes supported", ..}"."""
import ctypes as C
import json
import os
import sys

import pytest

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gnnkeras_amd import _native as nat
from test_train_plan_host import DIMS, FAKE, WIDTHS, dump, make_args

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'train_group_plans.json')

N = 300
# group_node_begin (the last entry is the node count): the group size (256, GNN_TRAIN_GROUP_MAX_NODES) and one more
TABLES = {'one group': [0, 200], 'many groups': list(range(0, 301, 20)), 'a group of 256': [0, 256, 300], 'a group of 257': [0, 257, 300]}


def grouped_args(d, kind, bn=False, focus='n', node_begin=TABLES['many groups'], out_begin=None, n_groups=None, n=N):
    """`make_args` (tests/test_train_plan_host.py) as a grouped forward: every output row of group g sits in
    [out_begin[g], out_begin[g + 1]); arc focus has two arcs per node.  A composite state of width 0 is the label matrix: 3 columns."""
    comp = kind == 'composite'
    ta, keep = make_args(d, n, composite=comp, bn=(bn, bn) if comp else bn, focus=focus, **(dict(L=max(DIMS)) if comp and d == 0 else {}))
    ta.forward_only, ta.k_groups = 1, FAKE
    if node_begin is not None:
        out_begin = [(2 if focus == 'a' else 1) * v for v in node_begin] if out_begin is None else out_begin
        nb, ob = (C.c_int32 * len(node_begin))(*node_begin), (C.c_int32 * len(out_begin))(*out_begin)
        ta.group_node_begin, ta.group_out_begin = C.cast(nb, C.c_void_p), C.cast(ob, C.c_void_p)
        keep += [nb, ob]
    ta.n_groups = len(node_begin) - 1 if n_groups is None else n_groups
    return ta, keep


def sections():
    return {kind: {f'd={d}{" bn" if bn else ""} focus={f}': {name: dict(d=d, kind=kind, bn=bn, focus=f, node_begin=nb, n=nb[-1]) for name, nb in TABLES.items()}
                   for d in WIDTHS for bn in (False, True) for f in 'nag'} for kind in ('homogeneous', 'composite')}


def malformed():
    """Calls `gnn_train_step` refuses on host data, for both model kinds: {name: (args, keep-alive)}."""
    out = {}
    for kind in ('homogeneous', 'composite'):
        def case(name, change=None, **kw):
            ta, keep = grouped_args(16, kind, **kw)
            if change: keep.append(change(ta))
            out[f'{kind}: {name}'] = (ta, keep)
        null = lambda *path: lambda ta: [setattr(ta.loop if p.startswith('loop.') else ta, p.split('.')[-1], None) for p in path]
        case('NULL tables', node_begin=None, n_groups=2)
        case('NULL group_out_begin', null('group_out_begin'))
        case('group_node_begin does not start at 0', node_begin=[1, 100, 300], out_begin=[0, 100, 300])
        case('group_node_begin ends short', node_begin=[0, 100, 299], out_begin=[0, 100, 300])
        case('group_out_begin ends short', node_begin=[0, 100, 300], out_begin=[0, 100, 299])
        case('an empty group', node_begin=[0, 100, 100, 300], out_begin=[0, 100, 100, 300])
        case('descending group_node_begin', node_begin=[0, 200, 100, 300], out_begin=[0, 1, 2, 300])
        case('descending group_out_begin', node_begin=[0, 100, 200, 300], out_begin=[0, 200, 100, 300])
        case('a group of 257', node_begin=TABLES['a group of 257'])
        case('the second group has 280', node_begin=[0, 20, 300])
        case('forward_only = 0', lambda ta: setattr(ta, 'forward_only', 0))
        def prev(ta):
            p = C.c_int32(-7)
            ta.prev_grads_ok_host = C.pointer(p)
            return p
        case('prev_grads_ok_host', prev)
        case('n_groups < 0', n_groups=-1)
        case('tape too small', lambda ta: setattr(ta, 'tape_bytes', 4096))
        case('NULL tape', null('tape'))
        def no_rowptr(which):
            def change(ta):
                c = getattr(ta.loop, which)
                c.rowptr = None
            return change
        case('adjacency without rowptr', no_rowptr('adjacency'))
        case('arcnode without rowptr', no_rowptr('arcnode'))
        def arcnode_shape(ta): ta.loop.arcnode.n_src = 7
        case('arcnode of another shape', arcnode_shape)
        case('NULL nodes', null('loop.nodes'))
        case('NULL arc_labels', null('loop.arc_labels'))
        case('NULL state0', null('loop.state0'))
        case('NULL out_index', null('loop.out_index'))
        case('NULL arc_src (arc focus)', null('loop.arc_src'), focus='a')
        case('NULL arc_dst (arc focus)', null('loop.arc_dst'), focus='a')
        case('NULL y_pred', null('y_pred'))
        case('NULL state', null('state'))
        case('NULL k_groups', null('k_groups'))
        def no_kernel(ta): ta.loop.net_state[0].kernel[0] = None
        case('state network without kernel', no_kernel)
        def no_out_bias(ta): ta.loop.net_output.bias[0] = None
        case('output network without bias', no_out_bias)
        if kind == 'composite':
            case('NULL type_nodes', null('loop.type_nodes'))
            def comp_adj(ta): ta.loop.composite_adjacency[1].rowptr = None
            case('composite_adjacency without rowptr', comp_adj)
        # two faults at once: which one is reported is the order of the checks
        case('forward_only = 0 and NULL tables', lambda ta: setattr(ta, 'forward_only', 0), node_begin=None, n_groups=2)
        case('not covered (pooled output) and tables that do not span', focus='g', node_begin=[0, 100, 299], out_begin=[0, 100, 300])
        case('tables that do not span and a tape too small', lambda ta: setattr(ta, 'tape_bytes', 4096), node_begin=[0, 100, 299], out_begin=[0, 100, 300])
        case('a group of 257 and a tape too small', lambda ta: setattr(ta, 'tape_bytes', 4096), node_begin=TABLES['a group of 257'])
        case('a tape too small and NULL nodes', lambda ta: [setattr(ta, 'tape_bytes', 4096), setattr(ta.loop, 'nodes', None)])
        case('adjacency without rowptr and NULL nodes', lambda ta: [no_rowptr('adjacency')(ta), setattr(ta.loop, 'nodes', None)])
        case('NULL nodes and NULL state0', null('loop.nodes', 'loop.state0'))
        case('NULL state0 and NULL out_index', null('loop.state0', 'loop.out_index'))
        case('NULL out_index and NULL arc_src (arc focus)', null('loop.out_index', 'loop.arc_src'), focus='a')
        case('NULL arc_src (arc focus) and NULL state', null('loop.arc_src', 'state'), focus='a')
        case('NULL k_groups and an output network without bias', lambda ta: [setattr(ta, 'k_groups', None), no_out_bias(ta)])
    return out


def answers(lib, ta):
    return f'{lib.gnn_train_workspace_bytes(C.byref(ta))} {lib.gnn_train_groups_supported(C.byref(ta))}'


def refusal(lib, ta):
    rc = lib.gnn_train_step(C.byref(ta))
    return [rc, lib.gnn_last_error().decode()]


def full_table(lib):
    table = {s: {key: {name: answers(lib, grouped_args(**kw)[0]) for name, kw in row.items()} for key, row in lines.items()}
             for s, lines in sections().items()}
    table['malformed'] = {key: refusal(lib, ta) for key, (ta, keep) in malformed().items()}
    return table


if __name__ == '__main__':
    if len(sys.argv) != 2: sys.exit('usage: python tests/test_train_group_plan_host.py FILE')
    with open(sys.argv[1], 'w') as fh: fh.write(dump(full_table(nat.lib())))
    sys.exit(0)


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(nat.LIB_PATH):
        nat.build()
    return nat.lib()


@pytest.fixture(scope='module')
def golden():
    with open(TABLE) as fh: return fh.read()


@pytest.fixture(scope='module')
def table(lib):
    return full_table(lib)


def test_group_plans_equal_the_committed_table(table, golden):
    """Case by case, then the file byte for byte."""
    want = json.loads(golden)
    moved = [(s, key, name, want.get(s, {}).get(key, {}).get(name), got) for s, lines in table.items() if s != 'malformed'
             for key, row in lines.items() for name, got in row.items() if want.get(s, {}).get(key, {}).get(name) != got]
    assert not moved, f'{len(moved)} cases differ from the table (section, case, groups, table, library); the first: {moved[:10]}'
    refused = [(key, want['malformed'].get(key), got) for key, got in table['malformed'].items() if want['malformed'].get(key) != got]
    assert not refused, refused
    assert dump(table) == golden          # the file is what the generator writes: no stale line, no other order


def test_the_cases_sit_on_both_sides_of_the_rules(table):
    """The answers tell covered from uncovered from oversized, and the two kinds carve different workspaces."""
    for kind in ('homogeneous', 'composite'):
        sec = table[kind]
        ans = lambda key, name: sec[key][name].split(' ')
        for d in (0, 8, 16, 17, 32, 64):
            for bn in ('', ' bn'):
                for f in 'na':
                    key = f'd={d}{bn} focus={f}'
                    assert [ans(key, name)[1] for name in TABLES] == ['0', '0', '0', '1'], (kind, key, sec[key])
                    assert all(int(ans(key, name)[0]) > 0 for name in TABLES), (kind, key)
                assert {ans(f'd={d}{bn} focus=g', name)[1] for name in TABLES} == {str(nat.TRAIN_GROUPS_UNCOVERED)}, (kind, d, bn)
        assert {ans(f'd=65 focus={f}', name)[1] for name in TABLES for f in 'nag'} == {str(nat.TRAIN_GROUPS_UNCOVERED)}
        assert ans('d=16 focus=n', 'one group')[0] != ans('d=16 focus=n', 'many groups')[0]       # (tables and statistics slots per group)
        assert ans('d=16 focus=n', 'one group')[0] != ans('d=17 focus=n', 'one group')[0]         # (rows padded to 16 / 32 / 64 floats)
    assert table['homogeneous']['d=16 focus=n'] != table['composite']['d=16 focus=n']
    for key, (rc, text) in table['malformed'].items(): assert rc == 1 and text, key
    texts = {key: text for key, (rc, text) in table['malformed'].items()}
    for kind in ('homogeneous', 'composite'):
        assert 'forward_only' in texts[f'{kind}: forward_only = 0 and NULL tables']
        assert 'do not cover' in texts[f'{kind}: not covered (pooled output) and tables that do not span']
        assert 'span' in texts[f'{kind}: tables that do not span and a tape too small']
        assert 'at most 256' in texts[f'{kind}: a group of 257 and a tape too small']
        assert 'tape too small' in texts[f'{kind}: a tape too small and NULL nodes']


def test_malformed_calls_write_nothing_back(lib):
    for key, (ta, keep) in malformed().items():
        before = bytes(ta)
        assert lib.gnn_train_step(C.byref(ta)) == 1, key
        assert bytes(ta) == before and keep[0].value == -7, key
