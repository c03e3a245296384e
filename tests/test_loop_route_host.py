"""Which kernels `gnn_loop_forward` runs, for every shape on either side of every condition of the rule (gnnkeras_amd/csrc/loop_route.hpp) -
no GPU: `gnn_loop_route_name` over a grid of arguments with fake device addresses, nothing launched, against the committed table
tests/golden/loop_routes.json.  The table is the library's own recorded answer: a kernel change that moves a route has to change the
table in the same commit, where a reader sees what moved.

    python tests/test_loop_route_host.py FILE      writes the table of the library GNNKERAS_AMD_LIB names (default: the built one)

The rule has few distinct answers, so the file is written factored (encode()): a "pattern" is the list of names along the last axis of a
section - the node count (homogeneous / composite) or the state width (groups) - with equal neighbours joined,
"64,130: k_state_small(setup_small)"; a line of a section is every case that shares the rest of its key ("net=1 flags=0", several joined
with " | " where they answer alike, "*" for every case of the section that no other line names) and says which pattern each value of the first axis (state width, or kind of group table) has:
"d=4,16:P3 17,32:P1 ..".  Every case of the grid is in the file: the full cross of state width, nodes, state network (with and without a
softmax), flags, the other inputs, model and group table.  The test expands the file to one name per case (decode()) and names the
first cases that differ."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

if __name__ == '__main__': sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnnkeras_amd import _native as nat

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'loop_routes.json')

# the boundaries of the rule: padded widths 16 / 32 / 64 / 128 / wider, 256 CUs of one 64-node tile each, the size from which the
# wave-specialised kernel runs (32768), GNN_MID_MAX_NODES (36000), GNN_XC_MIN_NODES (196608)
WIDTHS = (4, 16, 17, 32, 64, 65, 128, 129, 200, 256, 257)
NODES = (0, 64, 130, 16384, 16448, 32767, 32768, 36000, 36001, 196607, 196608)
NETS = ('1', '2', '2w', '3')              # layers of the state network; 2w: a hidden layer wider than the padded state width
FLAGS = {'0': 0, 'UNFUSED': nat.FLAG_UNFUSED, 'GEN2': nat.FLAG_FUSED_GEN2, 'GEN4': nat.FLAG_FUSED_GEN4, 'GEN5': nat.FLAG_FUSED_GEN5,
         'GEN6': nat.FLAG_FUSED_GEN6, 'GEN7': nat.FLAG_FUSED_GEN7, 'NO_EARLY_EXIT': nat.FLAG_NO_EARLY_EXIT}
OTHERS = ('', 'w', 'heavy', 'src', 'w+heavy', 'w+src', 'heavy+src', 'w+heavy+src')      # adjacency.w, n_heavy_segments = 2, nodes_src
GROUPS = {'fit': ([0, 100, 180, 300], None),               # 3 groups, each within one CU's LDS at padded widths 16 / 32
          'one_large': ([0, 100, 180, 3180], None),        # ... the third is not (3000 nodes): 51 tiles spread over the CUs
          '33': (list(range(0, 331, 10)), None),           # more than GNN_MAX_GROUPS
          'set': ([0, 100, 180, 300], [0, 3])}             # 3 groups that leave the loop together
L, A, DIMS = 3, 2, (3, 2)                 # label / arc label columns; label columns of the 2 node types of the composite model
FAKE = 0x7f0000001000                     # "device addresses": never read by the calls below (256-byte aligned)


def padded(S):
    p = 16
    while p < S: p *= 2
    return p if S <= 128 else (S + 3) // 4 * 4


def make_args(d, n, net='1', soft=False, flags=0, other='', composite=False, groups=None, workspace=True):
    """Loop arguments from dims alone (state_dim = d > 0).  Every pointer the argument check wants is FAKE; returns (args, keep-alive)."""
    a = nat.LoopArgs()
    keep = []
    a.abi_version, a.composite, a.n_types = nat.GNN_ABI_VERSION, int(composite), len(DIMS) if composite else 1
    a.n_nodes, a.n_arcs, a.dim_node_label, a.dim_arc_label = n, 4 * n, L, A
    a.state_dim, a.max_iteration, a.state_threshold, a.flags = d, 5, 0.01, flags
    a.nodes, a.ld_nodes, a.arc_labels, a.ld_arcs, a.state0 = FAKE, L, FAKE, A, FAKE
    csr = lambda n_src, w: nat.CSR(n, n_src, 4 * n, FAKE, FAKE, FAKE if w else None, None)
    a.adjacency, a.arcnode = csr(n, 'w' in other), nat.CSR(n, 4 * n, 4 * n, FAKE, FAKE, None, None)
    if 'heavy' in other:
        a.n_heavy_segments, a.heavy_seg_beg, a.heavy_seg_end, a.adjacency_light = 2, FAKE, FAKE, csr(n + 2, 'w' in other)
    if 'src' in other: a.nodes_src, a.ld_nodes_src = FAKE, L
    units = {'1': [d], '2': [d, d], '2w': [padded(d) + 4, d], '3': [d, d, d]}[net]
    for t in range(a.n_types):
        m = a.net_state[t]
        m.in_dim = DIMS[t] + 2 * d + sum(DIMS) + A if composite else 2 * d + 2 * L + A
        m.n_layers = len(units)
        for i, u in enumerate(units): m.units[i], m.activation[i], m.kernel[i], m.bias[i] = u, 3, FAKE, FAKE
        if soft: m.activation[len(units) - 1] = 7
        if composite:
            a.type_dim_label[t], a.type_offsets[t + 1] = DIMS[t], n if t == a.n_types - 1 else (t + 1) * (n // a.n_types)
            a.composite_adjacency[t] = csr(n, False)
    if composite: a.type_nodes = FAKE
    o = a.net_output
    o.in_dim, o.n_layers, o.units[0], o.activation[0], o.kernel[0], o.bias[0] = (d if composite else d + L), 1, 2, 7, FAKE, FAKE
    a.focus, a.n_out, a.k_out, a.state_out, a.out = nat.FOCUS['n'], n, FAKE, FAKE, FAKE
    if groups is not None:
        node_begin, set_begin = GROUPS[groups]
        keep.append((C.c_int32 * len(node_begin))(*node_begin))
        a.group_node_begin, a.n_groups = C.cast(keep[-1], C.c_void_p), len(node_begin) - 1
        if set_begin:
            keep.append((C.c_int32 * len(set_begin))(*set_begin))
            a.group_set_begin, a.n_group_sets = C.cast(keep[-1], C.c_void_p), len(set_begin) - 1
    if workspace: a.workspace, a.workspace_bytes = FAKE, 1 << 60
    return a, keep


def malformed():
    """Arguments the plan rejects: the name is ""."""
    out = {}
    a, k = make_args(32, 130); a.abi_version = 9; out['abi_version 9'] = (a, k)
    a, k = make_args(32, 130); a.net_state[0].units[0] = 31; out['state network 31 wide, state 32'] = (a, k)
    a, k = make_args(32, 130, composite=True); a.n_types = 9; out['9 node types'] = (a, k)
    a, k = make_args(32, 130, composite=True); a.max_iteration = 0; out['composite, max_iteration 0'] = (a, k)
    out['group table does not span the nodes'] = make_args(32, 130, groups='fit')
    a, k = make_args(32, 300, groups='fit'); a.n_group_sets = 4; out['more sets than groups'] = (a, k)
    out['NULL'] = (None, None)
    return out


def sections(reduced=False):
    """{section: {line key: [(axis value, make_args keywords)]}}.  `reduced`: the grid of the environment knobs (read once per process)."""
    nets = (('1', False), ('1', True), ('2', False), ('3', False)) if reduced else [(net, soft) for net in NETS for soft in (False, True)]
    flags = ('0', 'GEN2', 'GEN5') if reduced else tuple(FLAGS)
    widths, nodes = ((16, 32, 64, 128, 200), (130, 16448, 32768, 36001, 196608)) if reduced else (WIDTHS, NODES)
    sec = {'homogeneous': {}, 'composite': {}, 'groups': {}, 'composite groups': {}}
    for net, soft in nets:
        for fl in flags:
            for other in (OTHERS[:1] if reduced else OTHERS):
                rest = f'net={net}{" softmax" if soft else ""} flags={fl}{" " + other if other else ""}'
                kw = dict(net=net, soft=soft, flags=FLAGS[fl], other=other)
                for comp in ((False,) if reduced else (False, True)):
                    for d in widths:
                        sec['composite' if comp else 'homogeneous'][f'd={d} {rest}'] = [(n, dict(kw, d=d, n=n, composite=comp)) for n in nodes]
                    for g in (('fit',) if reduced else GROUPS):
                        sec['composite groups' if comp else 'groups'][f'groups={g} {rest}'] = \
                            [(d, dict(kw, d=d, n=GROUPS[g][0][-1], groups=g, composite=comp)) for d in widths if not reduced or d <= 64]
    return {s: lines for s, lines in sec.items() if lines}


def route_name(lib, a):
    return lib.gnn_loop_route_name(C.byref(a) if a is not None else None).decode()


def join_axis(pairs):
    """[(axis value, name)] -> ["v,v,..: name"] with equal neighbours joined."""
    out = []
    for v, name in pairs:
        if out and out[-1][1] == name: out[-1][0].append(v)
        else: out.append(([v], name))
    return [','.join(map(str, vs)) + ': ' + name for vs, name in out]


def compute(lib, reduced=False):
    table = {s: {key: join_axis([(v, route_name(lib, make_args(**kw)[0])) for v, kw in cases]) for key, cases in lines.items()}
             for s, lines in sections(reduced).items()}
    if not reduced: table['malformed'] = {key: route_name(lib, a) for key, (a, keep) in malformed().items()}
    return table


def encode(table):
    """The factored form of the module docstring: {'patterns': {id: names along the last axis}, section: {rest of the key(s): first axis -> id}}."""
    patterns, out = {}, {'patterns': {}}
    for s, lines in table.items():
        if s == 'malformed': out[s] = lines; continue
        rows = {}
        for key, names in lines.items():
            first, rest = key.split(' ', 1)
            axis, value = first.split('=')
            pid = patterns.setdefault(json.dumps(names), f'P{len(patterns)}')
            row = rows.setdefault(rest, [axis, []])
            if row[1] and row[1][-1][1] == pid: row[1][-1][0].append(value)
            else: row[1].append(([value], pid))
        merged = {}
        for rest, (axis, runs) in rows.items():
            merged.setdefault(axis + '=' + ' '.join(','.join(vs) + ':' + pid for vs, pid in runs), []).append(rest)
        common = max(merged, key=lambda text: len(merged[text]))          # the answer most cases share is written once, as "*": every other case
        out[s] = {('*' if text == common and len(rests) > 8 else ' | '.join(rests)): text for text, rests in merged.items()}
    out['patterns'] = {pid: json.loads(names) for names, pid in patterns.items()}
    return out


def decode(coded):
    """The file back to one name per case: {(section, line key, value on the last axis): name}."""
    cases = {}
    for s, lines in coded.items():
        if s == 'patterns': continue
        named = {rest for rests in lines for rest in rests.split(' | ')}
        grid = sections(reduced=': ' in s).get(s.split(': ')[-1], {}) if '*' in lines else {}
        every_other = [rest for rest in dict.fromkeys(key.split(' ', 1)[1] for key in grid) if rest not in named]
        for rests, text in lines.items():
            if s == 'malformed': cases[(s, rests, '')] = text; continue
            axis, runs = text.split('=', 1)
            for run in runs.split(' '):
                values, pid = run.split(':')
                for rest in (every_other if rests == '*' else rests.split(' | ')):
                    for value in values.split(','):
                        for entry in coded['patterns'][pid]:
                            last, name = entry.split(': ', 1)
                            for v in last.split(','): cases[(s, f'{axis}={value} {rest}', v)] = name
    return cases


def dump(table, indent='  '):
    """One line per pattern and per group of cases."""
    body = []
    for s, lines in table.items():
        rows = [f'{indent * 2}{json.dumps(k)}: {json.dumps(v)}' for k, v in lines.items()]
        body.append(f'{indent}{json.dumps(s)}: {{\n' + ',\n'.join(rows) + f'\n{indent}}}')
    return '{\n' + ',\n'.join(body) + '\n}\n'


ENV_SETTINGS = ['GNN_FUSED_KERNEL=2', 'GNN_FUSED_KERNEL=4', 'GNN_FUSED_KERNEL=5', 'GNN_FUSED_KERNEL=6', 'GNN_FUSED_KERNEL=7',
                'GNN_PREFIX_FUSION=0', 'GNN_XWIDE=0', 'GNN_MID_MAX_NODES=1000']


def compute_env_tables():
    """The reduced grid under each setting of a knob that is read once per process: one child process per setting, all at once."""
    procs = []
    for setting in ENV_SETTINGS:
        name, value = setting.split('=')
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), '--reduced'], stdout=subprocess.PIPE, text=True,
                                      env=dict(os.environ, **{name: value})))
    out = {}
    try:
        for setting, pr in zip(ENV_SETTINGS, procs):
            text, _ = pr.communicate(timeout=300)
            assert pr.returncode == 0, setting
            out[setting] = json.loads(text)
    finally:
        for pr in procs:
            if pr.poll() is None: pr.kill()
            pr.wait()
    return out


def compute_xc_min_nodes(lib):
    """GNN_XC_MIN_NODES is read at every call: switched inside this process."""
    old = os.environ.get('GNN_XC_MIN_NODES')
    os.environ['GNN_XC_MIN_NODES'] = '0'
    try:
        return {f'd={d} net=1 flags={fl}': join_axis([(n, route_name(lib, make_args(d=d, n=n, flags=FLAGS[fl])[0])) for n in (130, 16448, 36001)])
                for d in (16, 32, 64, 128) for fl in ('0', 'GEN4')}
    finally:
        if old is None: del os.environ['GNN_XC_MIN_NODES']
        else: os.environ['GNN_XC_MIN_NODES'] = old


def full_table(lib):
    table = compute(lib)
    table['GNN_XC_MIN_NODES=0 (switched inside the process)'] = compute_xc_min_nodes(lib)
    for setting, t in compute_env_tables().items():
        for s, lines in t.items(): table[f'{setting}: {s}'] = lines
    return table


if __name__ == '__main__':
    if len(sys.argv) != 2: sys.exit('usage: python tests/test_loop_route_host.py FILE')
    if sys.argv[1] == '--reduced': print(json.dumps(compute(nat.lib(), reduced=True)))
    else:
        with open(sys.argv[1], 'w') as fh: fh.write(dump(encode(full_table(nat.lib()))))
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


def test_routes_equal_the_committed_table(table, golden):
    """Case by case (the sections of the environment knobs come from child processes), then the file byte for byte."""
    got = encode(table)
    want_cases, got_cases = decode(json.loads(golden)), decode(got)
    moved = [(c, want_cases.get(c), got_cases.get(c)) for c in list(got_cases) + [c for c in want_cases if c not in got_cases]
             if want_cases.get(c) != got_cases.get(c)]
    assert not moved, f'{len(moved)} cases differ from the table (case, table, library); the first: {moved[:10]}'
    assert dump(got) == golden            # the file is what the generator writes: no stale line, no other order


def test_the_knobs_are_honoured(table):
    # GNN_XC_MIN_NODES=0, read per call: the wave-specialised kernel pinned on a small graph reads the constants line
    assert table['GNN_XC_MIN_NODES=0 (switched inside the process)']['d=32 net=1 flags=GEN4'] == ['130,16448,36001: k_state_fused4+xc']
    assert table['homogeneous']['d=32 net=1 flags=GEN4'][0].endswith(': k_state_fused4') and table['malformed']['NULL'] == ''
    # each knob that is read once moves something on the reduced grid
    base = compute(nat.lib(), reduced=True)
    for setting in ENV_SETTINGS:
        assert any(table[f'{setting}: {s}'] != base[s] for s in base), setting


def test_every_row_agrees_with_the_other_queries_and_with_the_launch(lib):
    """For every case: the name does not depend on a workspace being there; gnn_loop_groups_supported and gnn_loop_xc_applies say what the
    name says; and what the name calls refused is refused by gnn_loop_forward with that text (before its first launch: nothing here
    touches a device - only refused rows are ever passed to gnn_loop_forward)."""
    n_refused = 0
    for s, lines in sections().items():
        for key, cases in lines.items():
            for v, kw in cases:
                a, keep = make_args(**kw)
                name = route_name(lib, a)
                sup, xc = lib.gnn_loop_groups_supported(C.byref(a)), lib.gnn_loop_xc_applies(C.byref(a))
                assert xc == int(name.endswith('+xc') and not kw.get('composite') and kw['n'] > 0 and not kw.get('groups')), (s, key, v, name, xc)
                if not kw.get('groups'): assert sup == 0 and name and not name.startswith('refused'), (s, key, v, name, sup)
                elif name.startswith('k_state_lds'): assert sup == 2, (s, key, v, name, sup)
                elif name == 'k_state_small(setup_small)': assert sup == 1 and not kw.get('composite'), (s, key, v, name, sup)
                else:
                    assert name.startswith('refused: '), (s, key, v, name)
                    # (group sets: only the answer 2 runs them - include/gnnloop.h; without sets the answer 1 would have run)
                    assert sup == 0 or (kw['groups'] == 'set' and sup == 1 and 'group sets' in name), (s, key, v, name, sup)
                    assert lib.gnn_loop_forward(C.byref(a)) == 1 and lib.gnn_last_error().decode() == name[len('refused: '):], (s, key, v, name)
                    n_refused += 1
                a.workspace, a.workspace_bytes = None, 0
                assert route_name(lib, a) == name, (s, key, v)
    assert n_refused > 1000
    for key, (a, keep) in malformed().items():
        assert route_name(lib, a) == '', key
        if a is not None: assert lib.gnn_loop_workspace_bytes(C.byref(a)) == 0, key
