"""Host side of the training-mode convergence groups (C ABI 10) - no GPU: struct layout and exports through `_native`,
`gnn_train_groups_supported` on covered / uncovered / oversized / malformed arguments (dims and host arrays only), the run planner of the
grouped serial propagation, the vectorised relabelling against `update_graph` graph by graph, and the `serial_propagation` keyword."""
import ctypes as C
import os

import numpy as np
import pytest

from gnnkeras_amd import GraphObject
from gnnkeras_amd import _native as nat
from gnnkeras_amd.Models.MLP import MLP, get_inout_dims
from gnnkeras_amd.Models.GNN import GNNnodeBased, GNNarcBased, GNNgraphBased
from gnnkeras_amd.Models.LGNN import LGNN, plan_runs, relabel_graphs

CLS = {'n': GNNnodeBased, 'a': GNNarcBased, 'g': GNNgraphBased}


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(nat.LIB_PATH):
        nat.build()
    return nat.lib()


def test_abi_10_layout_and_exports(lib):
    assert nat.GNN_ABI_VERSION == 10 and lib.gnn_abi_version() == 10
    assert 'gnn_train_groups_supported' in nat.EXPORTS and lib.gnn_train_groups_supported is not None
    assert lib.gnn_struct_size(4) == C.sizeof(nat.TrainArgs)
    names = [f[0] for f in nat.TrainArgs._fields_]
    assert names[-5:] == ['forward_only', 'group_node_begin', 'n_groups', 'group_out_begin', 'k_groups']
    assert nat.TrainArgs.group_node_begin.offset > nat.TrainArgs.forward_only.offset
    assert nat.TRAIN_GROUP_MAX_NODES >= 256


def _train_args(S=14, d=0, L=14, A=3, T=2, n_nodes=300, n_out=300, focus='n', state_layers=1, out_layers=1, act_state=2):
    ta = nat.TrainArgs()
    a = ta.loop
    a.abi_version, a.n_types = nat.GNN_ABI_VERSION, 1
    a.n_nodes, a.n_arcs, a.dim_node_label, a.dim_arc_label = n_nodes, 2 * n_nodes, L, A
    a.state_dim, a.max_iteration, a.state_threshold = d, 5, 0.01
    width = d if d > 0 else L
    m = a.net_state[0]
    m.in_dim, m.n_layers = (2 * width + 2 * L + A if d > 0 else 2 * width + A), state_layers
    for i in range(state_layers): m.units[i], m.activation[i] = (width if i == state_layers - 1 else 20), act_state
    o = a.net_output
    node_part = width + L if d > 0 else width
    o.in_dim, o.n_layers = (2 * node_part + A if focus == 'a' else node_part), out_layers
    for i in range(out_layers): o.units[i], o.activation[i] = (T if i == out_layers - 1 else 10), 7
    a.focus, a.n_out = nat.FOCUS[focus], n_out
    ta.forward_only = 1
    return ta


def _with_groups(ta, node_begin, out_begin):
    nb, ob = (C.c_int32 * len(node_begin))(*node_begin), (C.c_int32 * len(out_begin))(*out_begin)
    ta.group_node_begin, ta.group_out_begin, ta.n_groups = C.cast(nb, C.c_void_p), C.cast(ob, C.c_void_p), len(node_begin) - 1
    return ta, (nb, ob)


def test_train_groups_supported_answers_from_dims_and_host_arrays(lib):
    ok = lambda ta, nb, ob: lib.gnn_train_groups_supported(C.byref(_with_groups(ta, nb, ob)[0]))
    assert ok(_train_args(), [0, 100, 300], [0, 100, 300]) == nat.TRAIN_GROUPS_OK
    assert ok(_train_args(), [0, 100, 300], [0, 0, 300]) == nat.TRAIN_GROUPS_OK                      # a group without output rows
    assert ok(_train_args(d=8), [0, 100, 300], [0, 100, 300]) == nat.TRAIN_GROUPS_OK                 # Kc = 2 * 14 + 3 = 31
    assert ok(_train_args(focus='a', n_out=600), [0, 100, 300], [0, 200, 600]) == nat.TRAIN_GROUPS_OK
    assert ok(_train_args(L=46), [0, 256, 300], [0, 256, 300]) == nat.TRAIN_GROUPS_OK                # 256 nodes at width 64
    # workspace: O(N S) - all of MUTAG (131 488 nodes, 4 337 graphs) at width 64 in one run, far below the tape of a training step
    big = _train_args(L=46, n_nodes=131488, n_out=131488)
    nb = [min(31 * i, 131488) for i in range(4337)] + [131488]
    big, keep = _with_groups(big, nb, nb)
    need = lib.gnn_train_workspace_bytes(C.byref(big))
    assert 0 < need < 256 << 20, need
    # not covered
    assert ok(_train_args(d=8, L=22), [0, 100, 300], [0, 100, 300]) == nat.TRAIN_GROUPS_UNCOVERED    # Kc = 47
    assert ok(_train_args(state_layers=2), [0, 100, 300], [0, 100, 300]) == nat.TRAIN_GROUPS_UNCOVERED
    assert ok(_train_args(out_layers=2), [0, 100, 300], [0, 100, 300]) == nat.TRAIN_GROUPS_UNCOVERED
    assert ok(_train_args(act_state=7), [0, 100, 300], [0, 100, 300]) == nat.TRAIN_GROUPS_UNCOVERED  # softmax state
    assert ok(_train_args(L=70), [0, 100, 300], [0, 100, 300]) == nat.TRAIN_GROUPS_UNCOVERED         # state wider than 64
    assert ok(_train_args(focus='g'), [0, 100, 300], [0, 100, 300]) == nat.TRAIN_GROUPS_UNCOVERED    # pooled output
    ta = _train_args(); ta.forward_only = 0
    assert ok(ta, [0, 100, 300], [0, 100, 300]) == nat.TRAIN_GROUPS_UNCOVERED
    ta = _train_args(); ta.drop_output.n = 1
    assert ok(ta, [0, 100, 300], [0, 100, 300]) == nat.TRAIN_GROUPS_UNCOVERED
    # oversized: the first such group, as g + 1
    assert ok(_train_args(), [0, 10, 300], [0, 10, 300]) == 2
    assert ok(_train_args(n_nodes=600, n_out=600), [0, 257, 300, 600], [0, 257, 300, 600]) == 1
    # malformed
    for nb, ob in (([0, 100, 299], [0, 100, 300]), ([1, 100, 300], [0, 100, 300]), ([0, 0, 300], [0, 0, 300]), ([0, 200, 100, 300], [0, 1, 2, 300]),
                   ([0, 100, 300], [0, 100, 299]), ([0, 100, 200, 300], [0, 200, 100, 300]), ([0, 100, 300], [0, 301, 300])):
        assert ok(_train_args(), nb, ob) == nat.TRAIN_GROUPS_MALFORMED, (nb, ob)
    ta = _train_args(); ta.n_groups = 2
    assert lib.gnn_train_groups_supported(C.byref(ta)) == nat.TRAIN_GROUPS_MALFORMED                  # NULL tables
    assert lib.gnn_train_groups_supported(None) == nat.TRAIN_GROUPS_UNCOVERED
    # the step itself refuses before any launch, with a message
    ta, keep = _with_groups(_train_args(), [0, 10, 300], [0, 10, 300])
    ta.tape, ta.tape_bytes = 256, 1 << 30
    assert lib.gnn_train_step(C.byref(ta)) != 0 and b'at most 256' in lib.gnn_last_error()
    ta, keep = _with_groups(_train_args(), [0, 100, 299], [0, 100, 300])
    ta.tape, ta.tape_bytes = 256, 1 << 30
    assert lib.gnn_train_step(C.byref(ta)) != 0 and b'span' in lib.gnn_last_error()
    ta, keep = _with_groups(_train_args(), [0, 100, 300], [0, 100, 300])
    ta.tape, ta.tape_bytes, ta.forward_only = 256, 1 << 30, 0
    assert lib.gnn_train_step(C.byref(ta)) != 0 and b'forward_only' in lib.gnn_last_error()


def test_plan_runs_keeps_order_and_isolates_oversized_graphs():
    sizes = [10, 20, 300, 30, 40, 257, 256, 5]
    plan = plan_runs(sizes, 256, 1 << 30)
    assert plan == [('run', 0, 2), ('single', 2), ('run', 3, 5), ('single', 5), ('run', 6, 8)]
    # a workspace bound cuts runs, never reorders: every graph once, ascending
    plan = plan_runs(sizes, 256, 60)
    seen = [i for e in plan for i in ([e[1]] if e[0] == 'single' else range(e[1], e[2]))]
    assert seen == list(range(len(sizes)))
    for e in plan:
        if e[0] == 'run': assert sum(sizes[e[1]:e[2]]) <= 60 or e[2] - e[1] == 1
        else: assert sizes[e[1]] > 256
    assert plan_runs([], 256, 100) == [] and plan_runs([7], 256, 100) == [('run', 0, 1)]
    assert plan_runs([5] * 10, 256, 1 << 30, max_graphs=4) == [('run', 0, 4), ('run', 4, 8), ('run', 8, 10)]
    # a MUTAG-sized set with nothing above the cap is ONE run
    rng = np.random.default_rng(0)
    sizes = rng.integers(4, 200, 4337).tolist()
    assert plan_runs(sizes, 256, 1 << 30) == [('run', 0, 4337)]


def _graphs(focus, rng, count=7):
    out = []
    for i in range(count):
        n = int(rng.integers(3, 12))
        e = int(rng.integers(n, 3 * n))
        pairs = rng.permutation(n * n)[:e]
        arcs = np.concatenate([np.stack([pairs // n, pairs % n], 1).astype(np.float64), rng.normal(size=(e, 3))], axis=1)
        rows = e if focus == 'a' else n
        om = rng.random(rows) < 0.7
        if i == 2: om[:] = False                                  # a graph without output rows
        sm = rng.random(rows) < 0.8
        n_t = 1 if focus == 'g' else int((om & sm).sum())
        out.append(GraphObject(nodes=rng.normal(size=(n, 4)), arcs=arcs, targets=np.eye(2)[rng.integers(0, 2, n_t)], focus=focus,
                               set_mask=sm, output_mask=om, sample_weight=np.ones(n_t), aggregation_mode='average'))
    return out


@pytest.mark.parametrize('focus', ['n', 'a', 'g'])
@pytest.mark.parametrize('get_state,get_output', [(True, True), (True, False), (False, True)])
def test_relabel_graphs_equals_update_graph_bit_for_bit(focus, get_state, get_output):
    rng = np.random.default_rng(3)
    graphs = _graphs(focus, rng)
    S, T = 5, 2
    gnns = []
    for _ in range(2):
        ns = MLP(2 * S + 2 * 4 + 3, [S], 'selu', 'lecun_normal', 'lecun_normal', rng=1, batch_normalization=False)
        no = MLP(2 * (S + 4) + 3 if focus == 'a' else S + 4, [T], 'softmax', 'glorot_normal', 'glorot_normal', rng=2, batch_normalization=False)
        gnns.append(CLS[focus](ns, no, S, 3, 0.01))
    lg = LGNN(gnns, get_state, get_output)
    states = [rng.normal(size=(g.nodes.shape[0], S)).astype(np.float32) for g in graphs]
    masks = [np.logical_and(np.asarray(g.set_mask).reshape(-1), np.asarray(g.output_mask).reshape(-1)) for g in graphs]
    outs = [rng.random((int(m.sum()), T)).astype(np.float32) for m in masks]
    want = [lg.update_graph(g.nodes, g.arcs, g.DIM_NODE_LABEL, g.set_mask, g.output_mask, s, o) for g, s, o in zip(graphs, states, outs)]
    got = [g.copy() for g in graphs]
    relabel_graphs(got, np.concatenate(states), np.concatenate(outs), get_state, get_output, focus == 'a')
    for g, (n, a, l), g0 in zip(got, want, graphs):
        assert g.nodes.dtype == np.float32 and g.arcs.dtype == np.float32
        assert g.nodes.shape == n.shape and np.array_equal(g.nodes, n)
        assert g.arcs.shape == a.shape and np.array_equal(g.arcs, a)
        assert np.array_equal(np.asarray(g.DIM_NODE_LABEL), np.asarray(l))
        assert np.array_equal(g0.nodes, g0.nodes) and g0.nodes.shape[1] == 4          # the inputs are untouched


def test_serial_propagation_keyword_and_attribute():
    from gnnkeras_amd.Models.training import Adam
    inp, lay = get_inout_dims('state', 14, 3, 2, 'g', 0)
    ns = MLP(inp[0], lay, 'selu', 'lecun_normal', 'lecun_normal', rng=1, batch_normalization=True)
    inp, lay = get_inout_dims('output', 14, 3, 2, 'g', 0)
    no = MLP(inp[0], lay, 'softmax', 'glorot_normal', 'glorot_normal', rng=2, batch_normalization=True)
    lg = LGNN([GNNgraphBased(ns, no, 0, 5, 0.01)], True, True)
    assert lg.serial_propagation == 'per_graph'
    with pytest.raises(ValueError, match='serial_propagation'):
        lg.compile(optimizer=Adam(0.01), loss='categorical_crossentropy', training_mode='serial', serial_propagation='nonsense')
    lg.compile(optimizer=Adam(0.01), loss='categorical_crossentropy', training_mode='serial', serial_propagation='grouped')
    assert lg.serial_propagation == 'grouped' and lg.training_mode == 'serial'
    lg.compile(optimizer=Adam(0.01), loss='categorical_crossentropy', training_mode='serial')
    assert lg.serial_propagation == 'per_graph'
    lg.serial_propagation = 'nonsense'
    with pytest.raises(ValueError, match='serial_propagation'):
        lg._propagate(lg.gnns[0], None, None)
