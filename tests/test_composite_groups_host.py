"""Host side of the inference convergence groups of HETEROGENEOUS models (`CompositeGNN*.Loop(training=False, groups=...)`) - no GPU:
`CompositeMultiGraphSequencer.merged_batches` against `CompositeGraphObject.merge`, array by array, and what `gnn_loop_groups_supported`
/ `gnn_loop_workspace_bytes` / `gnn_loop_group_max_nodes` answer for composite arguments (dims and host arrays only)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from gnnkeras_amd import CompositeGraphObject, SparseMatrix
from gnnkeras_amd import _native as nat
from gnnkeras_amd.Sequencers.GraphSequencers import CompositeMultiGraphSequencer
from gnnkeras_amd.synth import er_composite_graph


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(nat.LIB_PATH):
        nat.build()
    return nat.lib()


# ---- 1. merged_batches -----------------------------------------------------------------------------------------------------------------------
DIMS, T = (5, 3, 4), 2


def _graphs(count, mode, focus='n'):
    out = []
    rng = np.random.default_rng(5)
    for i in range(count):
        n = 9 + 2 * i
        g = er_composite_graph(n, 3 * n, dim_node_label=DIMS, seed=70 + i)
        rows = g.arcs.shape[0] if focus == 'a' else n
        om, sm = rng.random(rows) < 0.7, rng.random(rows) < 0.8
        om[0] = sm[0] = True
        out.append(CompositeGraphObject(nodes=g.nodes, arcs=g.arcs, targets=np.eye(T)[rng.integers(0, T, int(om.sum()))], type_mask=g.type_mask,
                                        dim_node_label=DIMS, focus=focus, set_mask=sm, output_mask=om, aggregation_mode=mode))
    return out


def _coo(m):
    """Sorted (row, col, value) rows of a scipy matrix or of a sequencer's sparse triple."""
    if not hasattr(m, 'tocoo'): m = SparseMatrix.from_triple(m).to_scipy()
    m = m.tocoo()
    rows = np.stack([m.row.astype(np.float64), m.col.astype(np.float64), m.data.astype(np.float64)], axis=1)
    return rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))], tuple(m.shape)


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


@pytest.mark.parametrize('mode,focus', [('composite_average', 'n'), ('average', 'a'), ('sum', 'n')])
def test_merged_batches_equal_the_composite_merge(mode, focus):
    graphs = _graphs(8, mode, focus)
    seq = CompositeMultiGraphSequencer(list(graphs), focus, mode, 2, shuffle=False, device='cpu')
    got = seq.merged_batches([1, 3])
    assert got is not None, 'CompositeMultiGraphSequencer.merged_batches answers None'
    x, node_begin = got
    members = graphs[2:4] + graphs[6:8]
    want = CompositeGraphObject.merge(members, focus=focus, aggregation_mode=mode)
    assert node_begin == [0, sum(g.nodes.shape[0] for g in graphs[2:4]), sum(g.nodes.shape[0] for g in members)]
    nodes, arcs, dim_node_label, type_mask, set_mask, output_mask, cas, adjacency, arcnode, nodegraph = x
    assert np.array_equal(_np(nodes), want.nodes.astype(np.float32))
    assert np.array_equal(_np(arcs), want.arcs.astype(np.float32))
    assert np.array_equal(_np(dim_node_label).reshape(-1), np.asarray(DIMS))
    assert np.array_equal(_np(type_mask).reshape(len(DIMS), -1), want.type_mask.transpose())
    assert np.array_equal(_np(set_mask).reshape(-1), want.set_mask) and np.array_equal(_np(output_mask).reshape(-1), want.output_mask)
    for name, a, b in [('Adjacency', adjacency, want.Adjacency), ('ArcNode', arcnode, want.ArcNode), ('NodeGraph', nodegraph, want.NodeGraph)] + \
                      [(f'CompositeAdjacency[{t}]', cas[t], want.CompositeAdjacencies[t]) for t in range(len(DIMS))]:
        (ra, sa), (rb, sb) = _coo(a), _coo(b)
        assert sa == sb and ra.shape == rb.shape and np.array_equal(ra[:, :2], rb[:, :2]), name
        assert np.array_equal(ra[:, 2].astype(np.float32), rb[:, 2].astype(np.float32)), name
    assert len(cas) == len(DIMS)
    # a range and the list of its members: the same (cached) object; targets of the merge = the batches' targets in order
    assert seq.merged_batches(1, 3) is seq.merged_batches([1, 2])
    assert seq.merged_batches([1, 3]) is got
    # 'normalized' divides by the arc count of the merge
    for g in graphs: g.setAggregation('normalized')
    assert CompositeMultiGraphSequencer(list(graphs), focus, 'normalized', 2, shuffle=False, device='cpu').merged_batches([1, 3]) is None


# ---- 2. the library's answers ----------------------------------------------------------------------------------------------------------------
def _composite_args(dims=(5, 3, 4), S=6, d=6, A=3, n_out_classes=2, n_nodes=300, focus='n', state_layers=1, act_state=2, flags=0, max_iteration=5,
                    bad_layers_type=None):
    """Composite loop arguments from dims alone: network t sees [labels[:, :d_t] | state | Adj^T state | aggregated_component],
    in_dim_t = d_t + 2 S + sum(dims) + A; the output network the state alone (arc focus: both ends' state and the arc label)."""
    a = nat.LoopArgs()
    n_types = len(dims)
    a.abi_version, a.composite, a.n_types = nat.GNN_ABI_VERSION, 1, n_types
    a.n_nodes, a.n_arcs, a.dim_node_label, a.dim_arc_label = n_nodes, 2 * n_nodes, max(dims), A
    a.state_dim, a.max_iteration, a.state_threshold, a.flags = d, max_iteration, 0.01, flags
    assert (d if d > 0 else max(dims)) == S
    w_comp = sum(dims) + A
    off = 0
    for t, d_t in enumerate(dims):
        a.type_dim_label[t] = d_t
        a.type_offsets[t] = off
        off += n_nodes // n_types + (1 if t < n_nodes % n_types else 0)
        m = a.net_state[t]
        layers = state_layers if bad_layers_type in (None, t) else 1
        m.in_dim, m.n_layers = d_t + 2 * S + w_comp, layers
        for i in range(layers): m.units[i], m.activation[i] = (S if i == layers - 1 else 20), act_state
    a.type_offsets[n_types] = off
    o = a.net_output
    o.in_dim, o.n_layers = (2 * S + A if focus == 'a' else S), 1
    o.units[0], o.activation[0] = n_out_classes, 7
    a.focus, a.n_out = nat.FOCUS[focus], n_nodes
    return a


def _with_groups(a, node_begin, set_begin=None):
    nb = (C.c_int32 * len(node_begin))(*node_begin)
    a.group_node_begin, a.n_groups = C.cast(nb, C.c_void_p), len(node_begin) - 1
    keep = [nb]
    if set_begin is not None:
        sb = (C.c_int32 * len(set_begin))(*set_begin)
        a.group_set_begin, a.n_group_sets = C.cast(sb, C.c_void_p), len(set_begin) - 1
        keep.append(sb)
    return a, keep


def _supported(lib, a, node_begin, set_begin=None):
    a, keep = _with_groups(a, node_begin, set_begin)
    return lib.gnn_loop_groups_supported(C.byref(a))


def test_composite_groups_supported_workspace_and_max_nodes(lib):
    lib.gnn_loop_group_max_nodes.restype, lib.gnn_loop_group_max_nodes.argtypes = C.c_int, [C.POINTER(nat.LoopArgs)]
    G3 = [0, 100, 180, 300]
    a, keep = _with_groups(_composite_args(), G3)
    assert lib.gnn_loop_workspace_bytes(C.byref(a)) > 0, lib.gnn_last_error()
    assert lib.gnn_loop_groups_supported(C.byref(a)) == 2                                           # three types, state 6 (padded 16)
    assert _supported(lib, _composite_args(S=20, d=20), G3) == 2                                    # padded 32
    assert _supported(lib, _composite_args(dims=(10,), S=10, d=0), G3) == 2                         # one type, state = labels
    assert _supported(lib, _composite_args(dims=(3,) * 8), G3) == 2                                 # GNN_MAX_TYPES types
    assert _supported(lib, _composite_args(focus='a'), G3) == 2 and _supported(lib, _composite_args(focus='g'), G3) == 2
    assert _supported(lib, _composite_args(), G3, [0, 1, 3]) == 2                                   # groups 1 and 2: one set
    # not covered: a two-layer state network of any one type, state width 40, a softmax state, the un-fused kernels
    for t in range(3):
        assert _supported(lib, _composite_args(state_layers=2, bad_layers_type=t), G3) == 0, t
    assert _supported(lib, _composite_args(S=40, d=40), G3) == 0
    assert _supported(lib, _composite_args(act_state=7), G3) == 0
    assert _supported(lib, _composite_args(flags=nat.FLAG_UNFUSED), G3) == 0
    assert _supported(lib, _composite_args(flags=nat.FLAG_FUSED_GEN2), G3) == 0                     # another kernel pinned
    assert _supported(lib, _composite_args(flags=nat.FLAG_FUSED_GEN7), G3) == 2
    # the largest group: at the export's figure it fits, one node above it does not
    for kw in (dict(), dict(S=20, d=20), dict(dims=(3,) * 8, S=20, d=20)):
        cap = lib.gnn_loop_group_max_nodes(C.byref(_composite_args(**kw)))
        assert cap > 0
        n = cap + 40
        assert _supported(lib, _composite_args(n_nodes=n, **kw), [0, cap, n]) == 2, (kw, cap)
        assert _supported(lib, _composite_args(n_nodes=n + 1, **kw), [0, cap + 1, n + 1]) == 0, (kw, cap)
    # sets with more groups than can be resident at once (one workgroup per CU, at most 1 024 CUs on any device)
    many = list(range(0, 3 * 2049, 3))
    assert _supported(lib, _composite_args(n_nodes=many[-1]), many) == 2
    assert _supported(lib, _composite_args(n_nodes=many[-1]), many, [0, 2, len(many) - 1]) == 0
    # malformed tables: refused as for homogeneous calls
    for nb in ([0, 100, 299], [1, 100, 300], [0, 0, 300], [0, 200, 100, 300]):
        assert _supported(lib, _composite_args(), nb) == 0, nb
        a, keep = _with_groups(_composite_args(), nb)
        assert lib.gnn_loop_workspace_bytes(C.byref(a)) == 0, nb
    assert _supported(lib, _composite_args(), G3, [0, 1, 2]) == 0 and _supported(lib, _composite_args(), G3, [0, 2, 2, 3]) == 0
    a = _composite_args(); a.n_groups = 2
    assert lib.gnn_loop_groups_supported(C.byref(a)) == 0                                           # NULL table


def test_max_nodes_shrinks_with_types_and_stays_below_the_homogeneous_figure(lib):
    lib.gnn_loop_group_max_nodes.restype, lib.gnn_loop_group_max_nodes.argtypes = C.c_int, [C.POINTER(nat.LoopArgs)]
    for S in (6, 20):
        h = nat.LoopArgs()
        h.abi_version, h.n_types = nat.GNN_ABI_VERSION, 1
        h.dim_node_label, h.dim_arc_label, h.state_dim, h.max_iteration = 5, 3, S, 5
        h.net_state[0].in_dim, h.net_state[0].n_layers, h.net_state[0].units[0], h.net_state[0].activation[0] = 2 * S + 2 * 5 + 3, 1, S, 2
        h.net_output.in_dim, h.net_output.n_layers, h.net_output.units[0], h.net_output.activation[0] = S + 5, 1, 2, 7
        homog = lib.gnn_loop_group_max_nodes(C.byref(h))
        assert homog == (158 * 1024) // (4 * (16 if S <= 16 else 32) + 16), homog             # what the homogeneous planner computes itself
        caps = [lib.gnn_loop_group_max_nodes(C.byref(_composite_args(dims=(3,) * n_types, S=S, d=S))) for n_types in range(1, 9)]
        assert all(a > b for a, b in zip(caps, caps[1:])), caps
        assert 0 < caps[-1] and caps[0] <= homog, (caps, homog)
    assert lib.gnn_loop_group_max_nodes(C.byref(_composite_args(S=40, d=40))) == 0                  # no LDS-resident kernel at this width
