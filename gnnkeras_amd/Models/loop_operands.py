"""The one place where "what a sequencer yields" becomes "what the library is handed" (DESIGN.md 6b): `prepare_operands` serves the
inference `Loop` of both model kinds, the building-block `LoopTrainer.forward` and every mode of the in-library training step, so a
batch means the same to all of them.  Around it the small pieces those callers share: per-type label widths, the draw of the initial
state, the fold of k per group into k per set, the loss kind, the "Dropout in front of a first Dense" test."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

from .. import _native as nat
from ..sparse import SparseMatrix


def _squeeze_last(x):
    return x.squeeze(-1) if isinstance(x, torch.Tensor) and x.dim() > 1 and x.shape[-1] == 1 else x


def _arc_endpoints(adjacency: SparseMatrix, device):
    key = ('endpoints', str(device))
    if key not in adjacency._dev:
        idx = torch.from_numpy(adjacency.indices.astype(np.int32)).to(device)
        adjacency._dev[key] = (idx[:, 0].contiguous(), idx[:, 1].contiguous())
    return adjacency._dev[key]


def type_mask_2d(type_mask):
    """(T, N) from (T, N, 1) as the sequencers hand it over; a mask that is (T, N) already stays - a graph of ONE node, (T, 1), must not
    lose its node axis to a second squeeze."""
    return _squeeze_last(type_mask) if type_mask.dim() == 3 else type_mask


def type_widths(dim_node_label):
    """Label width of every node type, as ints."""
    return [int(v) for v in (dim_node_label.reshape(-1).tolist() if isinstance(dim_node_label, torch.Tensor)
                             else np.asarray(dim_node_label).reshape(-1))]


def initial_state(state0, n_nodes, d, device, seed=None):
    """The loop's first state, float32 [n_nodes, d] on `device`: `state0` when given, else the reference's `tf.random.normal(stddev=0.1)`
    draw (reproducible with `seed`); None at d == 0, where the loop starts from the labels."""
    if d <= 0: return None
    if state0 is None:
        gen = None
        if seed is not None:
            gen = torch.Generator(device=device); gen.manual_seed(int(seed))
        state0 = torch.empty((n_nodes, d), device=device, dtype=torch.float32).normal_(0.0, 0.1, generator=gen)      # one launch
    state0 = state0.to(device, torch.float32).contiguous()
    if tuple(state0.shape) != (n_nodes, d): raise ValueError('state0 must be (n_nodes, state_vect_dim)')
    return state0


def set_ids(group_sets, device):
    """The set of every group from first-group offsets [B + 1]; uploaded BEFORE the launch whose k `fold_sets` reads: a pageable
    host-to-device copy behind it would block the host until the loop has finished."""
    gs_ = np.asarray([int(v) for v in group_sets], dtype=np.int64)
    return torch.as_tensor(np.repeat(np.arange(len(gs_) - 1), np.diff(gs_)), device=device)


def fold_sets(k, set_id, n_sets):
    """k per set from k per group: the groups of a set report the same k - or -1e9 where a member's wait for the others expired (any
    member: the minimum keeps it, so _check_k / check_last_k see it)."""
    return torch.full((n_sets,), float('inf'), device=k.device).scatter_reduce_(0, set_id, k, 'amin')


def loss_kind(model):
    """`nat.LOSSES` code of the compiled loss, or None where the loss has no device gradient; and its name."""
    m = model
    name = m.loss if isinstance(m.loss, str) else getattr(m.loss, '__name__', str(m.loss))
    return nat.LOSSES.get(str(name).lower()), name


def state_networks(model):
    return list(model.net_state) if isinstance(model.net_state, (list, tuple)) else [model.net_state]


def dropout_in_front(model) -> bool:
    """Does a network of `model` carry a Dropout layer in FRONT of its first Dense (position 0)?  Those run on the building blocks only."""
    return any(float(r) > 0 and int(q) == 0 for n_ in state_networks(model) + [model.net_output]
               for r, q in zip(n_.dropout_rate or [], n_.dropout_pos or []))


def prepare_operands(model, inputs, state0=None, seed=None, node_level=False):
    """The operands of one `Loop` over the batch `inputs` (the model's `process_inputs` order; raw triples and unsqueezed masks are
    taken too) as a plain record:
        nodes, arcs               float32, contiguous; caller_nodes / caller_arcs: the objects handed in (what a constants line's key holds)
        N, L, A, d, S, dev        nodes, label columns, arc-label columns, state_vect_dim, state width (d, or L at d == 0), device
        focus, out_index, n_rows  the effective focus (`node_level`: a graph-focused model stops at its nodes), the rows of
                                  set_mask & output_mask, the row count of the result (graphs under graph focus)
        adjacency, adj            the `SparseMatrix` and its device CSR; arcnode, an likewise; nodegraph (matrix) and ng (CSR, graph focus only)
        ends, state0              (arc_src, arc_dst), arc focus only; the first state, given or drawn, checked - None at d == 0
        composite                 heterogeneous model?  then dims, type_nodes, offsets, cas (matrices), ca_csr - else dims = [L]
    The networks are moved to the batch's device.  By-source transposes are not built here: only a backward pass reads them."""
    m = model
    op = SimpleNamespace(composite=isinstance(m.net_state, (list, tuple)))
    if op.composite: nodes, arcs, dim_node_label, type_mask, set_mask, output_mask, cas, adjacency, arcnode, nodegraph = inputs
    else: nodes, arcs, dim_node_label, set_mask, output_mask, adjacency, arcnode, nodegraph = inputs
    nat.require_device(nodes, 'nodes'); nat.require_device(arcs, 'arcs')
    dev = op.dev = nodes.device
    op.caller_nodes, op.caller_arcs = nodes, arcs
    op.nodes, op.arcs = nodes.to(torch.float32).contiguous(), arcs.to(torch.float32).contiguous()
    op.N, op.L = nodes.shape
    op.A, op.d = arcs.shape[1] - 2, m.state_vect_dim
    op.S = op.d if op.d > 0 else op.L
    op.focus = 'n' if (node_level and m._focus == 'g') else m._focus
    for n_ in state_networks(m) + [m.net_output]: n_.to(dev)
    op.dims, op.type_nodes, op.offsets, op.cas, op.ca_csr = [op.L], None, None, None, None
    if op.composite:
        # (`nodes[:, :d_t]` of the reference stops at the last column: from the third layer of a joint CompositeLGNN step on, `update_graph`
        # hands on widths above the column count - it widens the widths it is handed, the labels it builds anew from the first layer's)
        op.dims = [min(dt, int(op.L)) for dt in type_widths(dim_node_label)]
        T = len(op.dims)
        if T != len(m.net_state): raise ValueError(f'{T} node types but {len(m.net_state)} state networks')
        if T > nat.GNN_MAX_TYPES: raise ValueError(f'at most {nat.GNN_MAX_TYPES} node types are supported')
        op.type_nodes, op.offsets = m._type_lists(type_mask_2d(type_mask).to(dev))
        op.cas = [SparseMatrix.from_triple(c) for c in cas]
        op.ca_csr = [c.device_csr(dev) for c in op.cas]
    op.out_index = m._out_index(_squeeze_last(set_mask).to(dev), _squeeze_last(output_mask).to(dev))
    op.adjacency, op.arcnode, op.nodegraph = (SparseMatrix.from_triple(t) for t in (adjacency, arcnode, nodegraph))
    op.adj, op.an = op.adjacency.device_csr(dev), op.arcnode.device_csr(dev)
    op.ends = _arc_endpoints(op.adjacency, dev) if op.focus == 'a' else None
    op.ng = op.nodegraph.device_csr(dev) if op.focus == 'g' else None
    op.n_rows = op.ng['n_dst'] if op.focus == 'g' else len(op.out_index)
    op.state0 = initial_state(state0, op.N, op.d, dev, seed)
    return op
