"""Host side of the training-mode convergence groups of HETEROGENEOUS models (one state network per node type) - no GPU:
`gnn_train_groups_supported` on composite dims (covered / uncovered / oversized / malformed; dims and host arrays only), the workspace
of a composite MUTAG-sized run, the step's refusal of an oversized group before any launch, and which sequencers / layers
`LGNN._grouped_applies` admits."""
import ctypes as C
import os

import numpy as np
import pytest

from gnnkeras_amd import _native as nat
from gnnkeras_amd.Models.MLP import MLP, get_inout_dims
from gnnkeras_amd.Models.GNN import GNNnodeBased
from gnnkeras_amd.Models.LGNN import LGNN


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(nat.LIB_PATH):
        nat.build()
    return nat.lib()


def _composite_args(dims=(5, 3, 4), S=6, d=6, A=3, T=2, n_nodes=300, n_out=300, focus='n', state_layers=1, out_layers=1, act_state=2,
                    L=None, counts=None):
    """Composite train arguments from dims alone: network t sees [labels[:, :d_t] | state | Adj^T state | aggregated_component],
    in_dim_t = d_t + 2 S + sum(dims) + A; the output network the state alone (arc focus: both ends' state and the arc label)."""
    ta = nat.TrainArgs()
    a = ta.loop
    n_types = len(dims)
    L = max(dims) if L is None else L
    a.abi_version, a.composite, a.n_types = nat.GNN_ABI_VERSION, 1, n_types
    a.n_nodes, a.n_arcs, a.dim_node_label, a.dim_arc_label = n_nodes, 2 * n_nodes, L, A
    a.state_dim, a.max_iteration, a.state_threshold = d, 5, 0.01
    width = d if d > 0 else L
    assert width == S
    w_comp = sum(dims) + A
    counts = counts if counts is not None else [n_nodes // n_types + (1 if t < n_nodes % n_types else 0) for t in range(n_types)]
    off = 0
    for t, d_t in enumerate(dims):
        a.type_dim_label[t] = d_t
        a.type_offsets[t] = off
        off += counts[t]
        m = a.net_state[t]
        m.in_dim, m.n_layers = d_t + 2 * S + w_comp, state_layers
        for i in range(state_layers): m.units[i], m.activation[i] = (S if i == state_layers - 1 else 20), act_state
    a.type_offsets[n_types] = off
    o = a.net_output
    o.in_dim, o.n_layers = (2 * S + A if focus == 'a' else S), out_layers
    for i in range(out_layers): o.units[i], o.activation[i] = (T if i == out_layers - 1 else 10), 7
    a.focus, a.n_out = nat.FOCUS[focus], n_out
    ta.forward_only = 1
    return ta


def _with_groups(ta, node_begin, out_begin):
    nb, ob = (C.c_int32 * len(node_begin))(*node_begin), (C.c_int32 * len(out_begin))(*out_begin)
    ta.group_node_begin, ta.group_out_begin, ta.n_groups = C.cast(nb, C.c_void_p), C.cast(ob, C.c_void_p), len(node_begin) - 1
    return ta, (nb, ob)


def test_composite_groups_supported_answers_from_dims_and_host_arrays(lib):
    ok = lambda ta, nb, ob: lib.gnn_train_groups_supported(C.byref(_with_groups(ta, nb, ob)[0]))
    G2 = ([0, 100, 300], [0, 100, 300])
    assert ok(_composite_args(), *G2) == nat.TRAIN_GROUPS_OK                                        # 3 types, Kc_t = 20, 18, 19
    assert ok(_composite_args(), [0, 100, 300], [0, 0, 300]) == nat.TRAIN_GROUPS_OK                 # a group without output rows
    assert ok(_composite_args(focus='a', n_out=600), [0, 100, 300], [0, 200, 600]) == nat.TRAIN_GROUPS_OK
    assert ok(_composite_args(dims=(10,), S=10, d=0), *G2) == nat.TRAIN_GROUPS_OK                   # one type, state = labels
    # layer >= 1 of the reference's composite stack: d_t = 26, W_comp = 29 -> Kc = 55; and the bound itself, Kc = 64
    assert ok(_composite_args(dims=(26,), S=10, d=10), *G2) == nat.TRAIN_GROUPS_OK
    assert ok(_composite_args(dims=(20, 21), S=64, d=64, A=2, n_nodes=600, n_out=600), [0, 256, 600 - 256, 600], [0, 256, 600 - 256, 600]) == nat.TRAIN_GROUPS_OK      # Kc = 64 at width 64
    # not covered
    assert ok(_composite_args(dims=(20, 22), S=6, d=6, A=1), *G2) == nat.TRAIN_GROUPS_UNCOVERED     # Kc_1 = 22 + 43 = 65
    assert ok(_composite_args(state_layers=2), *G2) == nat.TRAIN_GROUPS_UNCOVERED
    assert ok(_composite_args(out_layers=2), *G2) == nat.TRAIN_GROUPS_UNCOVERED
    assert ok(_composite_args(S=70, d=70), *G2) == nat.TRAIN_GROUPS_UNCOVERED                       # state wider than 64
    assert ok(_composite_args(act_state=7), *G2) == nat.TRAIN_GROUPS_UNCOVERED                      # softmax state
    assert ok(_composite_args(focus='g'), *G2) == nat.TRAIN_GROUPS_UNCOVERED                        # pooled output
    ta = _composite_args(); ta.drop_state[1].n = 1
    assert ok(ta, *G2) == nat.TRAIN_GROUPS_UNCOVERED
    ta = _composite_args(); ta.drop_output.n = 1
    assert ok(ta, *G2) == nat.TRAIN_GROUPS_UNCOVERED
    ta = _composite_args(); ta.forward_only = 0
    assert ok(ta, *G2) == nat.TRAIN_GROUPS_UNCOVERED
    # oversized: the first such group, as g + 1
    assert ok(_composite_args(), [0, 10, 300], [0, 10, 300]) == 2
    assert ok(_composite_args(n_nodes=600, n_out=600), [0, 257, 300, 600], [0, 257, 300, 600]) == 1
    # malformed
    for nb, ob in (([0, 100, 299], [0, 100, 300]), ([1, 100, 300], [0, 100, 300]), ([0, 0, 300], [0, 0, 300]), ([0, 200, 100, 300], [0, 1, 2, 300]),
                   ([0, 100, 300], [0, 100, 299]), ([0, 100, 200, 300], [0, 200, 100, 300])):
        assert ok(_composite_args(), nb, ob) == nat.TRAIN_GROUPS_MALFORMED, (nb, ob)
    ta = _composite_args(); ta.n_groups = 2
    assert lib.gnn_train_groups_supported(C.byref(ta)) == nat.TRAIN_GROUPS_MALFORMED                # NULL tables


def test_composite_groups_workspace_and_refusals(lib):
    # all of composite MUTAG (131 488 nodes, 4 337 graphs) at width 64, three types, in one run: O(N S) plus the statistics slots per type
    big = _composite_args(dims=(14, 14, 14), S=64, d=64, n_nodes=131488, n_out=131488, L=14)
    nb = [min(31 * i, 131488) for i in range(4337)] + [131488]
    big, keep = _with_groups(big, nb, nb)
    need = lib.gnn_train_workspace_bytes(C.byref(big))
    assert 0 < need < 512 << 20, need
    # the step itself refuses before any launch, with a message
    ta, keep = _with_groups(_composite_args(), [0, 10, 300], [0, 10, 300])
    ta.tape, ta.tape_bytes = 256, 1 << 30
    assert lib.gnn_train_step(C.byref(ta)) != 0 and b'at most 256' in lib.gnn_last_error()
    ta, keep = _with_groups(_composite_args(), [0, 100, 299], [0, 100, 300])
    ta.tape, ta.tape_bytes = 256, 1 << 30
    assert lib.gnn_train_step(C.byref(ta)) != 0 and b'span' in lib.gnn_last_error()
    ta, keep = _with_groups(_composite_args(), [0, 100, 300], [0, 100, 300])
    ta.tape, ta.tape_bytes, ta.forward_only = 256, 1 << 30, 0
    assert lib.gnn_train_step(C.byref(ta)) != 0 and b'forward_only' in lib.gnn_last_error()
    ta, keep = _with_groups(_composite_args(state_layers=2), [0, 100, 300], [0, 100, 300])
    ta.tape, ta.tape_bytes = 256, 1 << 30
    assert lib.gnn_train_step(C.byref(ta)) != 0 and b'do not cover' in lib.gnn_last_error()


def _composite_graphs(count=3):
    from gnnkeras_amd import CompositeGraphObject
    from gnnkeras_amd.synth import er_composite_graph
    dims, T = (5, 3, 4), 2
    out = []
    for i in range(count):
        n = 12 + i
        g = er_composite_graph(n, 30, dim_node_label=dims, seed=40 + i)
        out.append(CompositeGraphObject(nodes=g.nodes, arcs=g.arcs, targets=np.eye(T)[np.zeros(n, int)], type_mask=g.type_mask,
                                        dim_node_label=dims, focus='n', set_mask=np.ones(n, bool), output_mask=np.ones(n, bool),
                                        aggregation_mode='composite_average'))
    return out


def test_grouped_applies_admits_the_composite_multi_graph_sequencer():
    from gnnkeras_amd.Models.CompositeGNN import CompositeGNNnodeBased
    from gnnkeras_amd.Models.CompositeLGNN import CompositeLGNN
    from gnnkeras_amd.Sequencers.GraphSequencers import (CompositeMultiGraphSequencer, CompositeSingleGraphSequencer, MultiGraphSequencer)
    dims, D, T, A = (5, 3, 4), 6, 2, 3
    inp, lay = get_inout_dims('state', dims, A, T, 'n', D)
    ns = [MLP(i, lay, 'tanh', 'lecun_normal', 'lecun_normal', rng=30 + t, batch_normalization=True) for t, i in enumerate(inp)]
    inp, lay = get_inout_dims('output', dims, A, T, 'n', D)
    no = MLP(inp[0], lay, 'softmax', 'glorot_normal', 'glorot_normal', rng=50, batch_normalization=True)
    comp = CompositeGNNnodeBased(ns, no, D, 4, 0.0)
    lg = CompositeLGNN([comp], True, True)
    graphs = _composite_graphs()
    seq = CompositeMultiGraphSequencer(list(graphs), 'n', 'composite_average', 2, shuffle=False, device='cpu')
    assert lg._grouped_applies(comp, seq)
    # 'normalized' divides by the arc count of the merge
    for g in graphs: g.setAggregation('normalized')
    seq_n = CompositeMultiGraphSequencer(list(graphs), 'n', 'normalized', 2, shuffle=False, device='cpu')
    assert not lg._grouped_applies(comp, seq_n)
    # the single-graph sequencers stay excluded
    single = CompositeSingleGraphSequencer(_composite_graphs(1)[0], 'n', 4, shuffle=False, device='cpu')
    assert not lg._grouped_applies(comp, single)
    # a composite layer wants the composite sequencer, a homogeneous layer the homogeneous one
    inp, lay = get_inout_dims('state', 14, 3, 2, 'n', 0)
    hs = MLP(inp[0], lay, 'selu', 'lecun_normal', 'lecun_normal', rng=1, batch_normalization=True)
    inp, lay = get_inout_dims('output', 14, 3, 2, 'n', 0)
    ho = MLP(inp[0], lay, 'softmax', 'glorot_normal', 'glorot_normal', rng=2, batch_normalization=True)
    homog = GNNnodeBased(hs, ho, 0, 5, 0.01)
    assert not LGNN([homog], True, True)._grouped_applies(homog, seq)
    assert not type(seq) is MultiGraphSequencer
