"""The key of a batch's constants line (gnnkeras_amd/sparse.py: `xc_key`, `SparseMatrix.constants_line`) - no GPU: the same tensors
hit; an in-place edit, another tensor object, another ArcNode, another label width / layout, another device or a dead reference miss;
a miss refills into the same buffer; nothing is valid before the caller reports the fill.  Plus the binding of the two new fields."""
import ctypes as C
import gc
import os

import numpy as np
import pytest
import torch

from gnnkeras_amd import _native as nat
from gnnkeras_amd import sparse
from gnnkeras_amd.sparse import SparseMatrix, xc_key, xc_key_matches


def _matrix(n_src, n_dst):
    return SparseMatrix(np.array([[0, 1], [1, 0]], dtype=np.int64), np.ones(2, np.float32), (n_src, n_dst))


def _batch(N=6, E=9, L=4, A=3):
    nodes, arcs = torch.rand(N, L), torch.rand(E, 2 + A)
    return nodes, arcs, _matrix(N, N), _matrix(E, N)


def test_same_tensors_hit_and_every_ingredient_misses():
    nodes, arcs, adj, arcnode = _batch()
    key = xc_key(nodes, arcs, arcnode, 4, True, 'cpu')
    args = (nodes, arcs, arcnode, 4, True, 'cpu')
    assert xc_key_matches(key, *args)
    assert xc_key_matches(key, nodes, arcs, arcnode, 4, True, torch.device('cpu'))          # however the device is spelled
    # other objects with the same contents (what `.to(float32).contiguous()` of another dtype would hand over at every call)
    assert not xc_key_matches(key, nodes.clone(), arcs, arcnode, 4, True, 'cpu')
    assert not xc_key_matches(key, nodes, arcs.clone(), arcnode, 4, True, 'cpu')
    assert not xc_key_matches(key, nodes, arcs, _matrix(9, 6), 4, True, 'cpu')               # another ArcNode
    assert not xc_key_matches(key, nodes, arcs, arcnode, 3, True, 'cpu')                     # another dim_node_label
    assert not xc_key_matches(key, nodes, arcs, arcnode, 4, False, 'cpu')                    # a model that does not see the labels: another line
    assert not xc_key_matches(key, nodes, arcs, arcnode, 4, True, 'meta')                    # another device
    nodes.mul_(2)                                                                            # a version bump
    assert not xc_key_matches(key, *args)
    key = xc_key(*args)
    assert xc_key_matches(key, *args)
    arcs[0, 2] = 5.0
    assert not xc_key_matches(key, *args)


def test_view_edits_and_dead_references_miss():
    nodes, arcs, adj, arcnode = _batch()
    key = xc_key(nodes, arcs, arcnode, 4, True, 'cpu')
    nodes[2:4].zero_()                                            # through a view: the version is shared with the base
    assert not xc_key_matches(key, nodes, arcs, arcnode, 4, True, 'cpu')
    key = xc_key(nodes, arcs, arcnode, 4, True, 'cpu')
    other = torch.rand_like(nodes)
    del nodes
    gc.collect()
    assert key['nodes']() is None
    assert not xc_key_matches(key, other, arcs, arcnode, 4, True, 'cpu')


def test_constants_line_cache_protocol():
    nodes, arcs, adj, arcnode = _batch()
    args = (nodes, arcs, arcnode, 4, True, 'cpu')
    line, valid = adj.constants_line(*args)
    assert not valid and tuple(line.shape) == (6, 32) and line.dtype == torch.float32
    line2, valid = adj.constants_line(*args)                      # the fill was never reported (a call that failed): still a fill
    assert not valid and line2 is line
    adj.constants_line_filled()
    line3, valid = adj.constants_line(*args)
    assert valid and line3 is line
    nodes.add_(1)                                                 # stale: refill, into the same buffer (one line per batch)
    line4, valid = adj.constants_line(*args)
    assert not valid and line4 is line
    adj.constants_line_filled()
    assert adj.constants_line(*args)[1]
    assert not adj.constants_line(nodes, arcs, arcnode, 4, False, 'cpu')[1]      # another layout
    assert not adj.constants_line(*args)[1]                       # ... which took the slot: the first layout is refilled
    other = _matrix(6, 6)                                         # another batch object knows nothing
    assert '_xc' not in other.__dict__ and not other.constants_line(*args)[1]


def test_reuse_switch_is_read_at_every_call(monkeypatch):
    monkeypatch.delenv('GNN_XC_REUSE', raising=False)
    assert sparse.xc_reuse_enabled()
    monkeypatch.setenv('GNN_XC_REUSE', '0')
    assert not sparse.xc_reuse_enabled()


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(nat.LIB_PATH):
        nat.build()
    return nat.lib()


def test_binding_carries_the_line(lib):
    names = [f[0] for f in nat.LoopArgs._fields_]
    assert names[-2:] == ['xc', 'xc_mode'] and (nat.XC_FILL, nat.XC_VALID) == (0, 1)
    assert lib.gnn_struct_size(2) == C.sizeof(nat.LoopArgs) and lib.gnn_struct_size(4) == C.sizeof(nat.TrainArgs)
    assert nat.TrainArgs.loop.offset == 0                          # the training step reads the same two fields of its `loop` member
    a = nat.LoopArgs()
    a.abi_version, a.n_types = nat.GNN_ABI_VERSION, 1
    a.n_nodes, a.n_arcs, a.dim_node_label, a.dim_arc_label = 300_000, 3_000_000, 14, 3
    a.state_dim, a.max_iteration, a.state_threshold = 64, 5, 0.01
    m = a.net_state[0]
    m.in_dim, m.n_layers, m.units[0], m.activation[0] = 2 * 64 + 2 * 14 + 3, 1, 64, 2
    o = a.net_output
    o.in_dim, o.n_layers, o.units[0], o.activation[0] = 64 + 14, 1, 2, 7
    a.n_out = 300_000
    assert lib.gnn_loop_xc_applies(C.byref(a)) == 1                # a large homogeneous graph, d = 64: the XC form
    small = nat.LoopArgs.from_buffer_copy(a); small.n_nodes = small.n_out = 1000
    assert lib.gnn_loop_xc_applies(C.byref(small)) == 0
    wide = nat.LoopArgs.from_buffer_copy(a)
    wide.state_dim = 128; wide.net_state[0].in_dim = 2 * 128 + 2 * 14 + 3; wide.net_state[0].units[0] = 128; wide.net_output.in_dim = 128 + 14
    assert lib.gnn_loop_xc_applies(C.byref(wide)) == 0
    comp = nat.LoopArgs.from_buffer_copy(a); comp.composite = 1
    assert lib.gnn_loop_xc_applies(C.byref(comp)) == 0
    w = (C.c_float * 1)(1.0)
    weighted = nat.LoopArgs.from_buffer_copy(a); weighted.adjacency.w = C.cast(w, C.c_void_p)       # (only its being non-NULL is read)
    assert lib.gnn_loop_xc_applies(C.byref(weighted)) == 0
    assert lib.gnn_loop_xc_applies(None) == 0
    ta = nat.TrainArgs()
    C.memmove(C.byref(ta), C.byref(a), C.sizeof(nat.LoopArgs))
    ta.loop.max_iteration = 10
    assert lib.gnn_train_xc_applies(C.byref(ta)) == 1
    ta.loop.n_nodes = ta.loop.n_out = 1000
    assert lib.gnn_train_xc_applies(C.byref(ta)) == 0
    assert lib.gnn_train_xc_applies(None) == 0
