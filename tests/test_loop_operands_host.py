"""What the Python layer hands to the library for one batch - no GPU: the real `Loop` / `LoopTrainer` paths run on CPU tensors and
stop at the library's door, against the committed table tests/golden/loop_operands.json.  The seams: `nat.require_device` lets CPU
tensors pass, `nat.current_stream` answers the null stream, `gnn_train_step` / `gnn_train_step_ex` of the loaded library object are a
recorder that snapshots the argument block and raises, `ops.loop_forward` is a recorder that answers zeros of the right shapes.  The
host-only queries (`gnn_train_workspace_bytes`, `gnn_train_groups_supported`, `gnn_train_phases_supported`) run for real.

    python tests/test_loop_operands_host.py FILE      writes the table

A record of a training call holds every field of `TrainArgs` (nested blocks by dotted name) that is not zero / null: integers and floats
by value, pointers as "ptr", arrays without their trailing zeros; the host tables behind `group_node_begin` / `group_out_begin` /
`tile_node_begin`; the sum of `state0` and of `out_index` read through their (host) addresses; `gnn_train_workspace_bytes`.  `tape` /
`tape_bytes` follow the allocation: recorded as "aligned" and "tape_bytes >= workspace".  An inference record holds the arguments of
`ops.loop_forward` (shapes, dtypes, ints, the CSR dims, the `composite` tuple) and the k `Loop` returns.  Every call passes a `seed`:
the Dropout seed otherwise follows `id(model)`.  The cases use the first six MUTAG graphs merged (the refusal of a group above 256
nodes: the first twenty)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

if __name__ == '__main__': sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnnkeras_amd import GraphObject, CompositeGraphObject, ops
from gnnkeras_amd import _native as nat
from gnnkeras_amd.load_MUTAG import load_graphs
from gnnkeras_amd.Models.MLP import MLP, get_inout_dims
from gnnkeras_amd.Models.GNN import GNNnodeBased, GNNarcBased, GNNgraphBased
from gnnkeras_amd.Models.CompositeGNN import CompositeGNNnodeBased, CompositeGNNarcBased, CompositeGNNgraphBased
from gnnkeras_amd.Models.training import LoopTrainer
from gnnkeras_amd.Sequencers.GraphSequencers import MultiGraphSequencer, CompositeMultiGraphSequencer

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'loop_operands.json')
CLS = {'n': GNNnodeBased, 'a': GNNarcBased, 'g': GNNgraphBased}
CCLS = {'n': CompositeGNNnodeBased, 'a': CompositeGNNarcBased, 'g': CompositeGNNgraphBased}
DIMS2 = (14, 9)             # label widths of the two node types (atom kind modulo 2)
A, T, SEED = 3, 2, 11


class Captured(Exception):
    """The recorder's way out of a training call: nothing behind the library call runs."""


# ---- the batches and models -------------------------------------------------------------------------------------------------------
def focused(graphs, focus, composite=False):
    """MUTAG graphs with masks, targets and sample weights for `focus` (graph focus: as loaded); `composite`: two node types."""
    rng = np.random.default_rng(5)
    out = []
    for g in graphs:
        n = g.nodes.shape[0]
        rows = g.arcs.shape[0] if focus == 'a' else n
        if focus == 'g': sm, om, targets, sw = np.ones(n, bool), np.ones(n, bool), g.targets, 1
        else:
            sm, om = rng.random(rows) < 0.8, rng.random(rows) < 0.7
            sm[0] = om[0] = True
            targets = np.eye(2)[rng.integers(0, 2, int(om.sum()))]
            sw = rng.uniform(0.5, 1.5, len(targets))
        kw = dict(focus=focus, set_mask=sm, output_mask=om, sample_weight=sw, aggregation_mode='average')
        if composite:
            out.append(CompositeGraphObject(g.nodes, g.arcs, targets, type_mask=np.eye(2, dtype=bool)[np.argmax(g.nodes, axis=1) % 2],
                                            dim_node_label=DIMS2, **kw))
        else:
            out.append(GraphObject(g.nodes, g.arcs, targets, **kw))
    return out


def batch(graphs, focus, composite=False):
    """(x_list, y, sample_weight) of `graphs` merged, CPU tensors; node offsets [G + 1]; output-row offsets [G + 1] (node / arc focus)."""
    gl = focused(graphs, focus, composite)
    seq = (CompositeMultiGraphSequencer if composite else MultiGraphSequencer)(gl, focus, 'average', len(gl), shuffle=False, device='cpu')
    nodes = np.cumsum([0] + [g.nodes.shape[0] for g in gl]).tolist()
    outs = np.cumsum([0] + [int(np.sum(g.set_mask & g.output_mask)) for g in gl]).tolist()
    return seq[0], nodes, outs


def homogeneous(focus, d, bn=False, dropout=False):
    """The starter widths (`get_inout_dims`): one SELU state layer, a softmax output layer."""
    inp, lay = get_inout_dims('state', 14, A, T, focus, d)
    ns = MLP(inp[0], lay, 'selu', 'lecun_normal', 'lecun_normal', rng=0, batch_normalization=bn, device='cpu',
             **(dict(dropout_rate=[0.3], dropout_pos=[1]) if dropout else {}))
    inp, lay = get_inout_dims('output', 14, A, T, focus, d)
    no = MLP(inp[0], lay, 'softmax', 'glorot_normal', 'glorot_normal', rng=1, batch_normalization=bn, device='cpu')
    m = CLS[focus](ns, no, d, 5, 0.01)
    m.compile(optimizer='adam', loss='categorical_crossentropy')
    return m


def heterogeneous(focus, d):
    S = d if d > 0 else max(DIMS2)
    ns = [MLP((dt + 2 * S + sum(DIMS2) + A,), [S], 'tanh', 'lecun_normal', 'lecun_normal', rng=30 + t, batch_normalization=False, device='cpu')
          for t, dt in enumerate(DIMS2)]
    no = MLP((2 * S + A if focus == 'a' else S,), [T], 'softmax', 'glorot_normal', 'glorot_normal', rng=50, batch_normalization=False, device='cpu')
    m = CCLS[focus](ns, no, d, 5, 0.01)
    m.compile(optimizer='adam', loss='categorical_crossentropy')
    return m


# ---- the recorders ----------------------------------------------------------------------------------------------------------------
def flat(s, prefix=''):
    """{dotted field name: value} of a ctypes structure, zero / null fields left out."""
    out = {}
    for name, kind in s._fields_:
        v, key = getattr(s, name), prefix + name
        if isinstance(v, C.Structure): out.update(flat(v, key + '.'))
        elif isinstance(v, C.Array):
            if issubclass(kind._type_, C.Structure):
                for i, e in enumerate(v): out.update(flat(e, f'{key}[{i}].'))
            else:
                vals = [('ptr' if e else 0) if kind._type_ is C.c_void_p else e for e in v]
                while vals and not vals[-1]: vals.pop()
                if vals: out[key] = vals
        elif isinstance(v, (int, float)):
            if v: out[key] = 'ptr' if kind is C.c_void_p else v
        elif v: out[key] = 'ptr'            # (a typed pointer)
    return out


def host_i32(address, n):
    return list((C.c_int32 * n).from_address(address)) if address else None


def train_record(ta, px=None):
    a = ta.loop
    rec = flat(ta)
    nbytes = rec['gnn_train_workspace_bytes'] = int(nat.lib().gnn_train_workspace_bytes(C.byref(ta)))
    rec['tape'] = 'aligned' if ta.tape and ta.tape % 256 == 0 else repr(ta.tape)
    rec['tape_bytes'] = 'tape_bytes >= workspace' if ta.tape_bytes >= nbytes > 0 else f'{ta.tape_bytes} < {nbytes}'
    if ta.n_groups:
        rec['group_node_begin'] = host_i32(ta.group_node_begin, ta.n_groups + 1)
        rec['group_out_begin'] = host_i32(ta.group_out_begin, ta.n_groups + 1)
    if ta.n_tiles: rec['tile_node_begin'] = host_i32(ta.tile_node_begin, ta.n_tiles + 1)
    if a.state0:
        n = a.n_nodes * a.state_dim
        rec['state0'] = [[a.n_nodes, a.state_dim], float(np.sum(np.ctypeslib.as_array((C.c_float * n).from_address(a.state0)), dtype=np.float64))]
    if a.out_index: rec['sum(out_index)'] = int(sum(host_i32(a.out_index, a.n_out)))
    if a.type_nodes: rec['sum(type_nodes * position)'] = int(sum(i * v for i, v in enumerate(host_i32(a.type_nodes, a.n_nodes))))
    if px is not None: rec.update(flat(px, 'phase.'))
    return rec


def tensor(t):
    return None if t is None else [list(t.shape), str(t.dtype).replace('torch.', ''), bool(t.is_contiguous())]


def csr_dims(c):
    return None if c is None else [c['n_dst'], c['n_src'], c['nnz'], c['w'] is not None, c['row_scale'] is not None]


def net_name(net):
    return [f'{n.input_dim}->{n.units}' for n in (net if isinstance(net, (list, tuple)) else [net])]


def loop_record(nodes, arcs, adj, arcn, ng, net_state, net_output, state0, out_index, ends, state_dim, max_iteration, state_threshold,
                focus, flags, composite=None, loop_events=None, groups=None, group_sets=None, xc=None, xc_valid=False,
                out_index_identity=False):
    rec = dict(nodes=tensor(nodes), arcs=tensor(arcs), adjacency=csr_dims(adj), arcnode=csr_dims(arcn), nodegraph=csr_dims(ng),
               net_state=net_name(net_state), net_output=net_name(net_output), state0=tensor(state0),
               out_index=tensor(out_index) + [int(out_index.sum())], arc_ends=None if ends is None else [tensor(e) for e in ends],
               ints=[state_dim, max_iteration, state_threshold, focus, flags], loop_events=loop_events is not None,
               groups=None if groups is None else [int(v) for v in groups], group_sets=None if group_sets is None else [int(v) for v in group_sets],
               xc=tensor(xc), xc_valid=bool(xc_valid), out_index_identity=bool(out_index_identity))
    if state0 is not None: rec['state0'].append(float(state0.sum(dtype=torch.float64)))
    if composite is not None:
        type_nodes, offsets, dims, cas = composite
        rec['composite'] = dict(type_nodes=tensor(type_nodes) + [int((type_nodes.long() * torch.arange(len(type_nodes))).sum())],
                                offsets=[int(v) for v in offsets], dims=[int(v) for v in dims], adjacencies=[csr_dims(c) for c in cas])
    return rec


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(nat.LIB_PATH):
        nat.build()
    return nat.lib()


class Seams:
    """The four seams, in place for the time of a `with`; `.calls` collects what reached them."""

    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def __enter__(self):
        self.saved = (nat.require_device, nat.current_stream, ops.loop_forward, self.lib.gnn_train_step, self.lib.gnn_train_step_ex)
        nat.require_device = lambda t, name: None
        nat.current_stream = lambda device: C.c_void_p(0)

        def step(ta_ref):
            self.calls.append(train_record(ta_ref._obj))
            raise Captured()

        def step_ex(ta_ref, px_ref):
            self.calls.append(train_record(ta_ref._obj, px_ref._obj))
            raise Captured()

        def loop_forward(*args, **kw):
            self.calls.append(loop_record(*args, **kw))
            nodes, out_index, state_dim = args[0], args[8], args[10]
            n_k = len(kw['groups']) - 1 if kw.get('groups') is not None else None
            k = torch.zeros(()) if n_k is None else torch.arange(n_k, dtype=torch.float32) + 1       # (the set fold keeps the minimum of every set)
            rows = args[4]['n_dst'] if args[4] is not None else len(out_index)
            return k, torch.zeros(nodes.shape[0], state_dim or nodes.shape[1]), torch.zeros(rows, T)
        self.lib.gnn_train_step, self.lib.gnn_train_step_ex, ops.loop_forward = step, step_ex, loop_forward
        return self

    def __exit__(self, *exc):
        nat.require_device, nat.current_stream, ops.loop_forward, self.lib.gnn_train_step, self.lib.gnn_train_step_ex = self.saved
        return False


def run(lib, fn):
    """What one call handed over: the records of the seams it reached, or the exception that ended it before."""
    with Seams(lib) as s:
        try:
            res = fn()
        except Captured:
            res = None
        except Exception as e:      # a refusal in front of the library: part of the record
            return {'raises': [type(e).__name__, str(e)]}
    rec = {'calls': s.calls}
    if res is not None: rec['k'] = [float(v) for v in res[0].reshape(-1)]
    return rec


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def cases(lib, graphs):
    table = {}
    for composite in (False, True):
        for focus, d in ([(f, d) for f in 'nag' for d in (0, 8)] if not composite else [('n', 8), ('a', 0), ('g', 8)]):
            (x, y, sw), nodes_b, out_b = batch(graphs[:6], focus, composite)
            m = heterogeneous(focus, d) if composite else homogeneous(focus, d)
            name = f'{"heterogeneous" if composite else "homogeneous"} focus={focus} d={d}: '
            inputs = lambda: m.process_inputs(x)
            tr = lambda: LoopTrainer(m)
            table[name + 'Loop'] = run(lib, lambda: m.Loop(*inputs(), seed=SEED))
            if not composite:
                table[name + 'Loop groups'] = run(lib, lambda: m.Loop(*inputs(), seed=SEED, node_level=focus == 'g', groups=nodes_b))
                sets = [0, 1, 3, 6, 7]                  # (as if batches 1 and 2 had been cut into 2 and 3 groups)
                table[name + 'Loop group_sets'] = run(lib, lambda: m.Loop(*inputs(), seed=SEED, node_level=focus == 'g',
                                                                          groups=nodes_b[:4] + [nodes_b[4] - 1] + nodes_b[4:], group_sets=sets))
            table[name + 'train_step'] = run(lib, lambda: tr().train_step(x, y, sw, seed=SEED))
            table[name + 'forward_native'] = run(lib, lambda: tr().forward_native(x, seed=SEED))
            table[name + 'Loop(training=True)'] = run(lib, lambda: m.Loop(*inputs(), training=True, seed=SEED))
            if focus == 'g':
                table[name + 'forward_native node_level'] = run(lib, lambda: tr().forward_native(x, seed=SEED, node_level=True))
                table[name + 'forward_native groups, refused'] = run(lib, lambda: tr().forward_native(x, seed=SEED, groups=nodes_b))
            table[name + 'forward_native groups'] = run(lib, lambda: tr().forward_native(x, seed=SEED, node_level=True, groups=nodes_b))
            gob = nodes_b if focus == 'g' else out_b
            table[name + 'forward_native groups group_out_begin'] = run(lib, lambda: tr().forward_native(x, seed=SEED, node_level=True, groups=nodes_b,
                                                                                                         group_out_begin=gob))
            table[name + 'forward_phase'] = run(lib, lambda: tr().forward_phase(x, seed=SEED))
            table[name + 'train_step groups, refused'] = run(lib, lambda: tr()._train_step_native(x, y, sw, None, SEED, False, groups=nodes_b))
    (x, y, sw), nodes_b, out_b = batch(graphs[:6], 'g')
    for label, kw in (('BatchNormalization', dict(bn=True)), ('Dropout behind the state Dense', dict(dropout=True))):
        m = homogeneous('g', 8, **kw)
        table[f'{label}: train_step'] = run(lib, lambda: LoopTrainer(m).train_step(x, y, sw, seed=SEED))
        table[f'{label}: forward_native'] = run(lib, lambda: LoopTrainer(m).forward_native(x, seed=SEED))
        table[f'{label}: Loop'] = run(lib, lambda: m.Loop(*m.process_inputs(x), seed=SEED))
    s0 = torch.full((x[0].shape[0], 8), 0.25, dtype=torch.float64)
    m = homogeneous('g', 8)
    table['state0 given (float64): train_step'] = run(lib, lambda: LoopTrainer(m).train_step(x, y, sw, state0=s0, seed=SEED))
    table['state0 given (float64): Loop'] = run(lib, lambda: m.Loop(*m.process_inputs(x), state0=s0, seed=SEED))
    for call, fn in (('train_step', lambda: LoopTrainer(m).train_step(x, y, sw, state0=s0[:1], seed=SEED)),
                     ('forward_native', lambda: LoopTrainer(m).forward_native(x, state0=s0[:1], seed=SEED)),
                     ('Loop', lambda: m.Loop(*m.process_inputs(x), state0=s0[:1], seed=SEED))):
        table[f'state0 of one row, refused: {call}'] = run(lib, fn)
    (x, y, sw), nodes_b, out_b = batch([g for g in graphs[:6] if g.nodes.shape[0] <= 64], 'g')       # (tiles of <= 64 nodes exist)
    m = homogeneous('g', 8)
    m.compile(optimizer='adam', loss='mse')
    table['graphs of at most 64 nodes, mse: train_step'] = run(lib, lambda: LoopTrainer(m).train_step(x, y, sw, seed=SEED))
    table['graphs of at most 64 nodes, mse: forward_native groups'] = run(lib, lambda: LoopTrainer(m).forward_native(x, seed=SEED, node_level=True, groups=nodes_b))
    (x, y, sw), nodes_b, out_b = batch(graphs[:20], 'n')
    m = homogeneous('n', 8)
    table['a group above 256 nodes, refused'] = run(lib, lambda: LoopTrainer(m).forward_native(x, seed=SEED, groups=[0, nodes_b[-1]]))
    return table


def dump(table, indent='  '):
    """One line per call that reached a seam."""
    body = []
    for name, rec in table.items():
        rows = [f'{indent * 2}{json.dumps(k)}: {json.dumps(v)}' for k, v in rec.items() if k != 'calls']
        rows += [f'{indent * 2}"call {i}": {json.dumps(c)}' for i, c in enumerate(rec.get('calls', []))]
        body.append(f'{indent}{json.dumps(name)}: {{\n' + ',\n'.join(rows) + f'\n{indent}}}')
    return '{\n' + ',\n'.join(body) + '\n}\n'


if __name__ == '__main__':
    if len(sys.argv) != 2: sys.exit('usage: python tests/test_loop_operands_host.py FILE')
    with open(sys.argv[1], 'w') as fh: fh.write(dump(cases(nat.lib(), load_graphs(limit=20))))
    sys.exit(0)


@pytest.fixture(scope='module')
def table(lib, mutag_graphs):
    return cases(lib, mutag_graphs[:20])


def test_operands_equal_the_committed_table(table):
    """Case by case, then the file byte for byte."""
    with open(TABLE) as fh: golden = fh.read()
    want = json.loads(golden)
    got = json.loads(dump(table))
    moved = [(name, want.get(name), rec) for name, rec in got.items() if want.get(name) != rec]
    assert not moved, f'{len(moved)} cases differ from the table (case, table, this tree); the first: {moved[:2]}'
    assert dump(table) == golden


def test_the_cases_reach_the_library_and_the_refusals_do_not(table):
    for name, rec in table.items():
        if 'refused' in name: assert 'raises' in rec and rec['raises'][0] in ('NotImplementedError', 'ValueError'), (name, rec)
    reached = [name for name, rec in table.items() if rec.get('calls')]
    assert len(reached) >= 60, len(reached)
    full = table['homogeneous focus=g d=8: train_step']['calls'][0]
    assert full['targets'] == 'ptr' and full['adjacency_by_source.rowptr'] == 'ptr' and 'forward_only' not in full
    fwd = table['homogeneous focus=g d=8: forward_native']['calls'][0]
    assert fwd['forward_only'] == 1 and 'targets' not in fwd and 'adjacency_by_source.rowptr' not in fwd
    assert table['homogeneous focus=g d=8: forward_native node_level']['calls'][0].get('loop.focus', 0) == nat.FOCUS['n'] != fwd['loop.focus']
    assert table['homogeneous focus=g d=8: forward_phase']['calls'][0]['phase.phase'] == nat.TRAIN_PHASE_FORWARD
    assert table['homogeneous focus=n d=8: forward_native groups']['calls'][0]['n_groups'] == 6
    assert table['homogeneous focus=n d=8: Loop group_sets']['k'] == [1.0, 2.0, 4.0, 7.0]


# ---- the two places where the paths used to disagree ------------------------------------------------------------------------
def one_node_batch():
    nodes = np.zeros((1, 14)); nodes[0, 3] = 1.0
    g = CompositeGraphObject(nodes, np.array([[0, 0, 1.0, 0.0, 0.0]]), np.eye(2)[:1], type_mask=np.array([[False, True]]),
                             dim_node_label=DIMS2, focus='n', aggregation_mode='average')
    return CompositeMultiGraphSequencer([g], 'n', 'average', 1, shuffle=False, device='cpu')[0]


@pytest.mark.parametrize('call', ['Loop', 'Loop(training=True)', 'train_step', 'forward_native'])
def test_a_heterogeneous_graph_of_one_node_keeps_its_node_axis(lib, call):
    """`process_inputs` squeezes (T, 1, 1) to (T, 1): a second squeeze would leave (T,), which `_type_lists` refuses."""
    x, y, sw = one_node_batch()
    m = heterogeneous('n', 8)
    rec = run(lib, {'Loop': lambda: m.Loop(*m.process_inputs(x), seed=SEED),
                    'Loop(training=True)': lambda: m.Loop(*m.process_inputs(x), training=True, seed=SEED),
                    'train_step': lambda: LoopTrainer(m).train_step(x, y, sw, seed=SEED),
                    'forward_native': lambda: LoopTrainer(m).forward_native(x, seed=SEED)}[call])
    assert 'raises' not in rec and len(rec['calls']) == 1, rec
    c = rec['calls'][0]
    assert (c['composite']['offsets'] if call == 'Loop' else c['loop.type_offsets']) == [0, 0, 1]


def test_the_building_block_forward_checks_the_shape_of_state0(lib):
    class Reached(Exception): pass

    class NoPrimitives:
        def __init__(self, device): pass

        def __getattr__(self, name): raise Reached(name)
    (x, y, sw), _, _ = batch(load_graphs(limit=2), 'g')
    tr = LoopTrainer(homogeneous('g', 8))
    tr.prim_cls = NoPrimitives
    with Seams(lib):
        with pytest.raises(ValueError, match=r'state0 must be \(n_nodes, state_vect_dim\)'):
            tr.forward(x, state0=torch.zeros(1, 8), seed=SEED)
