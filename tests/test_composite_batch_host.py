"""Device assembly of heterogeneous batches, host side (gnnkeras_amd/device_batch.py `CompositeDeviceDataset`) - no GPU, no library: the data
set is built with device='cpu', the batches are planned, and the plan (the table `gnn_ragged_copy` would execute) is run by a numpy
restatement of the eight descriptor kinds of include/gnnloop.h.  Every array is then compared, exactly, with the host merge
(`CompositeGraphObject.merge` -> `CompositeGraphTensor`, reference composite_graph_class.py:142-167) of the same graphs."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from gnnkeras_amd import CompositeGraphObject
from gnnkeras_amd import _native as nat
from gnnkeras_amd.device_batch import CompositeDeviceDataset, DeviceDataset, lookup_type_lists
from gnnkeras_amd.Models.CompositeGNN import CompositeGNNnodeBased
from gnnkeras_amd.Sequencers.GraphSequencers import CompositeMultiGraphSequencer

DIMS = (3, 2, 1)
# (node types, arcs): 1 .. 6 nodes.  0: no arcs; 1: no node of type 2, node 3 without incoming arc; 2: node 2 is entered from types 0, 1, 1
# (weights 1, 1/2, 1/2 under 'composite_average': one weight per entry); 3: node 0 is entered from types 2 and 1 (weights 1 and 1: still one
# scale per row); 4 .. 6: every destination entered from one type, or from one node of each
SHAPES = [([0], []),
          ([0, 1, 0, 1], [(0, 1), (1, 0), (2, 1), (3, 2)]),
          ([0, 1, 2, 0, 1, 2], [(0, 2), (1, 2), (4, 2), (2, 3), (3, 5), (5, 0), (5, 1)]),
          ([2, 2, 1], [(0, 1), (1, 0), (2, 0)]),
          ([0, 0, 0, 1, 2], [(0, 1), (1, 2), (2, 0), (3, 4), (4, 3), (0, 2)]),
          ([1, 2], [(0, 1), (1, 0)]),
          ([0, 1, 2], [(0, 1), (2, 1), (1, 2)])]
BATCHES = [[0, 1, 2], [3, 4, 5], [6]]          # batch size 3: the first needs per-entry weights, the second does not, the last is one graph


def make_graphs(focus, dims=DIMS, shapes=SHAPES):
    """(the graphs' own operators are 'sum': a merge builds the batch's from the mode it is given, and 'normalized' cannot be built for the
    graph without arcs alone)"""
    rng = np.random.default_rng(11)
    out = []
    for types, arcs in shapes:
        n, e = len(types), len(arcs)
        rows = {'n': n, 'a': e, 'g': n}[focus]
        sm, om = rng.random(rows) < 0.8, rng.random(rows) < 0.7
        if focus == 'g': sm, om, n_t = np.ones(n, bool), np.ones(n, bool), 1
        else: n_t = int(om.sum())
        a = np.concatenate([np.array(arcs, dtype=float).reshape(e, 2), rng.normal(size=(e, 2))], axis=1)
        out.append(CompositeGraphObject(nodes=rng.normal(size=(n, max(dims))), arcs=a, targets=rng.normal(size=(n_t, 2)),
                                        type_mask=np.eye(len(dims), dtype=bool)[types], dim_node_label=dims, focus=focus, set_mask=sm, output_mask=om,
                                        sample_weight=rng.uniform(0.5, 1.5, n_t)))
    return out


def run_plan(D):
    """The eight kinds of `enum gnn_ragged_kind`, descriptor by descriptor, over the plan's (CPU) tensors; offsets count elements."""
    for d in D:
        dst = d['dst'].view(-1).numpy()
        src = None if d['src'] is None else d['src'].view(-1).numpy()
        k = len(d['count'])
        col = lambda name: np.broadcast_to(np.asarray(d.get(name, 0)), (k,))
        for j in range(k):
            c, so, do = int(d['count'][j]), int(d['src_off'][j]), int(d['dst_off'][j])
            iadd, fval, width, i = col('iadd')[j], col('fval')[j], int(col('width')[j]), np.arange(c)
            if d['kind'] in (nat.RC_COPY_F32, nat.RC_COPY_U8): dst[do:do + c] = src[so:so + c]
            elif d['kind'] == nat.RC_COPY_I32_ADD: dst[do:do + c] = src[so:so + c] + np.int32(iadd)
            elif d['kind'] == nat.RC_COPY_ROWS_ADD2: dst[do:do + c] = np.where(i % max(width, 1) < 2, src[so:so + c] + np.float32(fval), src[so:so + c])
            elif d['kind'] == nat.RC_FILL_F32: dst[do:do + c] = np.float32(fval)
            elif d['kind'] == nat.RC_FILL_I32: dst[do:do + c] = np.int32(iadd)
            elif d['kind'] == nat.RC_IOTA_I32: dst[do:do + c] = np.int32(iadd) + i.astype(np.int32)
            elif d['kind'] == nat.RC_TYPE_ROWS_U8:
                for t in range(width): dst[do + t * int(iadd):do + t * int(iadd) + c] = src[so:so + c] == t
            else: raise AssertionError(f"kind {d['kind']}")


def eff_scale(c):
    deg = np.diff(c['rowptr'].numpy())
    if c['w'] is not None: return c['w'].numpy()
    s = np.ones(c['n_dst'], np.float32) if c['row_scale'] is None else c['row_scale'].numpy()
    return np.repeat(s, deg)                  # per entry; rows without entries never matter


def same_csr(mh, md, tag):
    ch, cd = mh.device_csr('cpu'), md.device_csr('cpu')
    assert (ch['n_dst'], ch['n_src'], ch['nnz']) == (cd['n_dst'], cd['n_src'], cd['nnz']), tag
    assert torch.equal(ch['rowptr'], cd['rowptr']) and torch.equal(ch['src'], cd['src']), tag
    assert np.array_equal(eff_scale(ch), eff_scale(cd)), tag
    assert (ch['w'] is None) == (cd['w'] is None), tag                 # one weight per entry, or one scale per row: the same choice


@pytest.mark.parametrize('focus', ['n', 'a', 'g'])
@pytest.mark.parametrize('mode', ['sum', 'average', 'normalized', 'composite_average'])
def test_planned_batches_equal_host_merged_ones(focus, mode):
    graphs = make_graphs(focus)
    host = CompositeMultiGraphSequencer(graphs, focus, mode, 3, shuffle=False, device='cpu', assemble='host')
    ds = CompositeDeviceDataset(graphs, focus, mode, 'cpu')
    plan = ds.plan(BATCHES)
    run_plan(plan.D)
    batches = ds.batches_of(plan)
    assert len(batches) == len(host) == 3
    if mode == 'composite_average': assert plan.row_scale_form.tolist() == [False, True, True]
    stub = SimpleNamespace(_type_cache={})
    for i, (h, d) in enumerate(zip(host.graph_tensors, batches)):
        for name in ('nodes', 'arcs', 'set_mask', 'output_mask', 'targets', 'sample_weight', 'type_mask', 'DIM_NODE_LABEL'):
            a, b = getattr(h, name), getattr(d, name)
            assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), (i, name)
        assert d.type_mask.is_contiguous() and (d.DIM_ARC_LABEL, d.DIM_TARGET) == (h.DIM_ARC_LABEL, h.DIM_TARGET)
        for name in ('Adjacency', 'ArcNode') + (('NodeGraph',) if focus == 'g' else ()):
            same_csr(getattr(h, name), getattr(d, name), (i, name))
            assert getattr(h, name).shape == getattr(d, name).shape
        if mode == 'composite_average':
            assert (d.Adjacency.device_csr('cpu')['w'] is None) == (i > 0) and (d.ArcNode.device_csr('cpu')['w'] is None) == (i > 0)
        assert len(d.CompositeAdjacencies) == len(h.CompositeAdjacencies) == len(DIMS)
        for t, (mh, md) in enumerate(zip(h.CompositeAdjacencies, d.CompositeAdjacencies)):
            same_csr(mh, md, (i, 'CA', t))
            assert np.array_equal(mh.indices, md.indices) and np.array_equal(mh.values, md.values) and mh.shape == md.shape
        want_nodes, want_off = CompositeGNNnodeBased._type_lists(stub, h.type_mask)
        got_nodes, got_off = lookup_type_lists(d.type_mask)
        assert got_nodes.dtype == torch.int32 and torch.equal(got_nodes, want_nodes) and np.array_equal(got_off, want_off)
        assert np.array_equal(d.Adjacency.block_starts(), np.concatenate([[0], np.cumsum([len(SHAPES[j][0]) for j in BATCHES[i]])]))      # one block per graph
    d.type_mask[0, 0] = not bool(d.type_mask[0, 0])                   # an in-place edit: the registered lists no longer answer
    assert lookup_type_lists(d.type_mask) is None


def test_refusals():
    graphs = make_graphs('n')
    with pytest.raises(ValueError):                                    # the homogeneous class keeps refusing typed graphs
        DeviceDataset(graphs, 'n', 'sum', 'cpu')
    two = make_graphs('n')[1]
    two.type_mask[0, 1] = True                                         # node 0 has two types
    with pytest.raises(ValueError, match='one-hot'):
        CompositeDeviceDataset(graphs[:2] + [two], 'n', 'sum', 'cpu')
    other = make_graphs('n', dims=(3, 1, 1))[3]
    with pytest.raises(ValueError, match='DIM_NODE_LABEL'):
        CompositeDeviceDataset(graphs[:2] + [other], 'n', 'sum', 'cpu')
    with pytest.raises(ValueError):
        CompositeDeviceDataset(graphs, 'n', 'mean', 'cpu')
