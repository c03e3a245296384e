"""What `gnn_train_step` plans for every shape on either side of every condition of its two path rules (gnnkeras_amd/csrc/train_loop.hpp
`homogeneous_train_path`, train_composite.hpp `composite_train_path`) - no GPU: `gnn_train_workspace_bytes`, `gnn_train_xc_applies` and
`gnn_train_phases_supported` over a grid of arguments with fake device addresses, nothing launched, against the committed table
tests/golden/train_plans.json.  The tape's size moves with the path (each path carves its own buffers) and with the thin output head,
so a change of either rule or of the tape layout has to change the table in the same commit, where a reader sees what moved.  The
malformed calls record the return code and the message of `gnn_train_step`: every one of them is refused on host data, before a launch.

    python tests/test_train_plan_host.py FILE      writes the table of the library GNNKERAS_AMD_LIB names (default: the built one)

A line of a section is one case but for the node count: "d=16 bn: {"64": "bytes xc phases", ..}"."""
import ctypes as C
import json
import os
import sys

import pytest

if __name__ == '__main__': sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnnkeras_amd import _native as nat

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'train_plans.json')

# the boundaries of the rules: one tile, 256 tiles of 64 nodes (one per CU) and one more, GNN_TRAIN_BIG_MIN_NODES (32768)
NODES = (1, 64, 16384, 16385, 32767, 32768)
WIDTHS = (0, 8, 16, 17, 32, 64, 65)       # state_dim; 0: the state is the 14 label columns (padded to 16 on the persistent path)
FAKE = 0x7f0000001000                     # "device addresses": never read by the calls below (256-byte aligned)
K = 4
# what a homogeneous case changes against the base (one SELU layer of the state's width, no BatchNormalization, node focus, 2 classes,
# L = 14 and A = 3: 31 constant columns)
VARIANTS = {'base': {}, 'two state layers': dict(layers=2), 'bn': dict(bn=True), 'softmax state': dict(soft=True),
            'state dropout': dict(drop_state=True), 'output dropout': dict(drop_output=True), 'L=15 (33 constant columns)': dict(L=15),
            'focus=a': dict(focus='a'), 'focus=g': dict(focus='g'), 'focus=g bn': dict(focus='g', bn=True), '5 outputs': dict(T=5),
            '5 outputs bn': dict(T=5, bn=True), 'n_out=n_nodes-1': dict(fewer_out=True), 'max_iteration=0': dict(K=0),
            '256 tiles': dict(tiles=256), '257 tiles': dict(tiles=257)}
COMPOSITE = {'base': {}, 'second type empty': dict(empty=True), 'bn on the first type': dict(bn=(True, False)), 'bn': dict(bn=(True, True)),
             'two state layers': dict(layers=2), 'softmax state': dict(soft=True), 'state dropout': dict(drop_state=True),
             'focus=a': dict(focus='a'), 'focus=g': dict(focus='g'), '5 outputs': dict(T=5), 'n_out=n_nodes-1': dict(fewer_out=True)}
DIMS = (3, 2)                             # label columns of the two node types of the composite model
KNOBS = ('GNN_TRAIN_BIG_MIN_NODES=1000', 'GNN_TRAIN_SMALL=0')      # read at every call: switched inside this process


def csr(n_dst, n_src, nnz):
    return nat.CSR(n_dst, n_src, nnz, FAKE, FAKE, None, None)


def fill_mlp(m, in_dim, units, act, bn):
    m.in_dim, m.n_layers = in_dim, len(units)
    for i, u in enumerate(units): m.units[i], m.activation[i], m.kernel[i], m.bias[i] = u, act[i], FAKE, FAKE
    if bn: m.has_bn, m.bn_eps, m.bn_gamma, m.bn_beta, m.bn_mean, m.bn_var = 1, 1e-3, FAKE, FAKE, FAKE, FAKE


def fill_grads(g, m):
    g.dgamma, g.dbeta = FAKE, FAKE
    for i in range(m.n_layers): g.dkernel[i], g.dbias[i] = FAKE, FAKE


def make_args(d, n, composite=False, layers=1, bn=False, soft=False, drop_state=False, drop_output=False, L=14, A=3, focus='n', T=2,
              fewer_out=False, K=K, tiles=0, empty=False):
    """Training arguments from dims alone.  Every pointer an argument check wants is FAKE; returns (args, keep-alive)."""
    ta = nat.TrainArgs()
    a = ta.loop
    keep = []
    E = 2 * n
    S = d if d > 0 else L
    a.abi_version, a.composite, a.n_types = nat.GNN_ABI_VERSION, int(composite), len(DIMS) if composite else 1
    a.n_nodes, a.n_arcs, a.dim_node_label, a.dim_arc_label = n, E, L, A
    a.state_dim, a.max_iteration, a.state_threshold = d, K, 0.01
    a.nodes, a.ld_nodes, a.arc_labels, a.ld_arcs, a.state0 = FAKE, L, FAKE, A, FAKE
    a.adjacency, a.arcnode, ta.adjacency_by_source = csr(n, n, E), csr(n, E, E), csr(n, n, E)
    units, act = [S] * layers, [3] * (layers - 1) + [7 if soft else 3]
    for t in range(a.n_types):
        bn_t = bn[t] if isinstance(bn, tuple) else bn
        in_dim = DIMS[t] + 2 * S + sum(DIMS) + A if composite else (2 * S + 2 * L + A if d > 0 else 2 * S + A)
        fill_mlp(a.net_state[t], in_dim, units, act, bn_t)
        if drop_state: ta.drop_state[t].n, ta.drop_state[t].pos[0], ta.drop_state[t].rate[0] = 1, 1, 0.5
        if composite:
            a.type_dim_label[t], a.composite_adjacency[t] = DIMS[t], csr(n, n, E)
            a.type_offsets[t + 1] = n if (t == a.n_types - 1 or empty) else (t + 1) * (n // a.n_types)
            fill_grads(ta.grad_state_types[t], a.net_state[t])
    if composite: a.type_nodes = FAKE
    fill_grads(ta.grad_state, a.net_state[0])
    M = (E if focus == 'a' else n) - (1 if fewer_out and focus != 'g' else 0)
    node_part = S if composite or d == 0 else S + L
    fill_mlp(a.net_output, 2 * node_part + A if focus == 'a' else node_part, [T], [7], bn if isinstance(bn, bool) else False)
    fill_grads(ta.grad_output, a.net_output)
    if drop_output: ta.drop_output.n, ta.drop_output.pos[0], ta.drop_output.rate[0] = 1, 1, 0.5
    a.focus, a.n_out, a.out_index, a.arc_src, a.arc_dst = nat.FOCUS[focus], M, FAKE, FAKE, FAKE
    if focus == 'g':
        G = max(1, n // 18)
        a.nodegraph, ta.nodegraph_by_source = csr(G, M, M), csr(M, G, M)
    if tiles: ta.tile_node_begin, ta.n_tiles = FAKE, tiles
    ta.targets, ta.y_pred, ta.state, ta.loss = FAKE, FAKE, FAKE, FAKE
    keep.append(C.c_int32(-7))
    ta.k_host = C.pointer(keep[-1])
    ta.bn_momentum = 0.99
    ta.tape, ta.tape_bytes = FAKE, 1 << 60
    return ta, keep


def malformed():
    """Calls `gnn_train_step` refuses on host data, for both model kinds."""
    out = {}
    for kind, comp in (('homogeneous', False), ('composite', True)):
        def case(name, change):
            ta, keep = make_args(16, 200, composite=comp)
            keep.append(change(ta))
            out[f'{kind}: {name}'] = (ta, keep)
        case('abi_version 9', lambda ta: setattr(ta.loop, 'abi_version', 9))
        case('net_state in_dim + 1', lambda ta: setattr(ta.loop.net_state[0], 'in_dim', ta.loop.net_state[0].in_dim + 1))
        case('net_output in_dim + 1', lambda ta: setattr(ta.loop.net_output, 'in_dim', ta.loop.net_output.in_dim + 1))
        case('NULL tape', lambda ta: setattr(ta, 'tape', None))
        case('unaligned tape', lambda ta: setattr(ta, 'tape', FAKE + 16))
        case('tape too small', lambda ta: setattr(ta, 'tape_bytes', 4096))
        case('missing targets', lambda ta: setattr(ta, 'targets', None))
        case('unknown loss kind', lambda ta: setattr(ta, 'loss_kind', 7))
        def fwd_prev(ta):
            prev = C.c_int32(-7)
            ta.forward_only, ta.prev_grads_ok_host = 1, C.pointer(prev)
            return prev
        case('forward_only with prev_grads_ok_host', fwd_prev)
    return out


def sections(reduced=False):
    """{section: {line key: [(node count, make_args keywords)]}}.  `reduced`: the grid of the environment knobs."""
    if reduced:
        nodes = (64, 999, 1000, 32768)
        return {'homogeneous': {f'd={d} {v}': [(n, dict(VARIANTS[v], d=d, n=n)) for n in nodes] for d in (8, 16, 64, 65) for v in ('base', 'bn')},
                'composite': {f'd={d} {v}': [(n, dict(COMPOSITE[v], d=d, n=n, composite=True)) for n in nodes] for d in (16, 64, 65) for v in ('base', 'bn')}}
    hom = {f'd={d} base': [(n, dict(d=d, n=n)) for n in NODES] for d in WIDTHS}
    for v, kw in VARIANTS.items():
        if v == 'base': continue
        for d in (0, 16, 64) if v.startswith('L=15') or 'outputs' in v or 'focus' in v else (16, 64):
            hom[f'd={d} {v}'] = [(n, dict(kw, d=d, n=n)) for n in NODES]
    comp = {f'd={d} {v}': [(n, dict(kw, d=d, n=n, composite=True)) for n in (2, 64, 16384, 16385, 32767, 32768)]
            for v, kw in COMPOSITE.items() for d in (16, 64, 65)}
    return {'homogeneous': hom, 'composite': comp}


def answers(lib, ta):
    return f'{lib.gnn_train_workspace_bytes(C.byref(ta))} {lib.gnn_train_xc_applies(C.byref(ta))} {lib.gnn_train_phases_supported(C.byref(ta))}'


def compute(lib, reduced=False):
    return {s: {key: {str(n): answers(lib, make_args(**kw)[0]) for n, kw in cases} for key, cases in lines.items()}
            for s, lines in sections(reduced).items()}


def refusal(lib, ta):
    rc = lib.gnn_train_step(C.byref(ta))
    return [rc, lib.gnn_last_error().decode()]


def with_knob(setting, fn):
    name, value = setting.split('=')
    old = os.environ.get(name)
    os.environ[name] = value
    try: return fn()
    finally:
        if old is None: del os.environ[name]
        else: os.environ[name] = old


def full_table(lib):
    for name in ('GNN_TRAIN_BIG_MIN_NODES', 'GNN_TRAIN_SMALL', 'GNN_TRAIN_TAPE_MB'): assert name not in os.environ, name
    table = compute(lib)
    for setting in KNOBS:
        for s, lines in with_knob(setting, lambda: compute(lib, reduced=True)).items(): table[f'{setting}: {s}'] = lines
    table['malformed'] = {key: refusal(lib, ta) for key, (ta, keep) in malformed().items()}
    return table


def dump(table, indent='  '):
    """One line per group of cases."""
    body = []
    for s, lines in table.items():
        rows = [f'{indent * 2}{json.dumps(k)}: {json.dumps(v)}' for k, v in lines.items()]
        body.append(f'{indent}{json.dumps(s)}: {{\n' + ',\n'.join(rows) + f'\n{indent}}}')
    return '{\n' + ',\n'.join(body) + '\n}\n'


if __name__ == '__main__':
    if len(sys.argv) != 2: sys.exit('usage: python tests/test_train_plan_host.py FILE')
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


def test_plans_equal_the_committed_table(table, golden):
    """Case by case, then the file byte for byte."""
    want = json.loads(golden)
    moved = [(s, key, n, want.get(s, {}).get(key, {}).get(n), got) for s, lines in table.items() if s != 'malformed'
             for key, row in lines.items() for n, got in row.items() if want.get(s, {}).get(key, {}).get(n) != got]
    assert not moved, f'{len(moved)} cases differ from the table (section, case, nodes, table, library); the first: {moved[:10]}'
    refused = [(key, want['malformed'].get(key), got) for key, got in table['malformed'].items() if want['malformed'].get(key) != got]
    assert not refused, refused
    assert dump(table) == golden          # the file is what the generator writes: no stale line, no other order


def test_the_cases_sit_on_both_sides_of_the_rules(table):
    """The answers tell the paths apart: only the row-streaming path has no phases, only it adopts a constants line, and the tape of the
    persistent path (rows padded to 16 / 32 / 64 floats, buffers of its own) differs from the general path's at the same dims."""
    hom = table['homogeneous']
    ans = lambda key, n, s=hom: s[key][str(n)].split(' ')
    assert ans('d=16 base', 32767)[1:] == ['0', '0'] and ans('d=16 base', 32768)[1:] == ['1', '-1']
    assert ans('d=17 base', 32768)[1:] == ['0', '0'] and ans('d=65 base', 32768)[1:] == ['0', '0']
    for v in ('two state layers', 'softmax state', 'state dropout', 'L=15 (33 constant columns)', 'max_iteration=0'):
        assert ans(f'd=16 {v}', 32768)[1:] == ['0', '0'], v
    assert ans('d=16 256 tiles', 16385)[0] != ans('d=16 257 tiles', 16385)[0] == ans('d=16 base', 16385)[0]
    assert ans('d=16 5 outputs', 32768)[0] != ans('d=16 base', 32768)[0]          # (the thin head's partials are part of the tape)
    big = table['GNN_TRAIN_BIG_MIN_NODES=1000: homogeneous']
    assert ans('d=16 base', 999, big)[1:] == ['0', '0'] and ans('d=16 base', 1000, big)[1:] == ['1', '-1']
    off = table['GNN_TRAIN_SMALL=0: homogeneous']
    assert ans('d=8 base', 64, off)[0] != ans('d=8 base', 64)[0]                   # (8 columns padded to 16 on the persistent path alone)
    for key, (rc, text) in table['malformed'].items(): assert rc == 1 and text, key


def test_malformed_calls_write_nothing_back(lib):
    for key, (ta, keep) in malformed().items():
        before = bytes(ta)
        assert lib.gnn_train_step(C.byref(ta)) == 1, key
        assert bytes(ta) == before and keep[0].value == -7, key
        if 'abi' in key or 'in_dim' in key: assert lib.gnn_train_workspace_bytes(C.byref(ta)) == 0, key
