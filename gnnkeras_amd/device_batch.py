"""Batch assembly on the device: `GraphObject.merge` + `GraphTensor.fromGraphObject` (reference `GNN/graph_class.py:386-413`,
`:539-560`, driven by `MultiGraphSequencer.build_batches / on_epoch_end`, `GNN/Sequencers/GraphSequencers.py:42-46, :123-127`)
without the host in the data path.

The reference re-merges every batch in numpy at each `on_epoch_end` (reshuffle) and converts it to tensors; the host port of
that costs ≈1.3 ms per MUTAG batch (merge + upload + CSR build) = 0.18 s per epoch next to 0.05 s of forwards. Here the
DATASET is uploaded once: all graphs concatenated in dataset order, with node / arc ids made graph-local, together with
everything a merged batch needs that is a per-graph property (by-destination CSR pieces of Adjacency and ArcNode,
their by-source forms for the backward pass, 'average' row scales). A merged batch is then the block-diagonal
concatenation of its graphs: each of its arrays is a run of per-graph segments with a per-segment offset added to the ids.
`DeviceDataset.assemble(ids)` builds the table of segment operations with vectorised numpy (≈0.5 k descriptors for 32 graphs),
uploads it with ONE small copy and runs ONE `gnn_ragged_copy` launch; the by-source operands (training) and the COO triples
(API compatibility, tests) are assembled / materialised lazily, only when somebody asks.

What is batch-dependent rather than per-graph: 'normalized' weights (1 / #arcs of the MERGED graph, `graph_class.py:110`)
become one constant row scale per batch; NodeGraph (`:127-138`, block_diag at `:407`) is generated (iota / fills).
Results are identical to the host path — same arrays, same CSR order, same weights — `tests/test_gpu_batch.py` compares
them array by array and through the model.

Heterogeneous data sets (`CompositeGraphObject.merge`, reference `GNN/composite_graph_class.py:142-167`) go the same way through
`CompositeDeviceDataset`: per graph it also keeps a type id per node, every type's node list and the by-destination CSR of every
composite adjacency (`:57-70`), so that a batch's `type_mask` (one descriptor per graph, `GNN_RC_TYPE_ROWS_U8`), its T
`CompositeAdjacencies` and the per-type node lists the model needs (`lookup_type_lists`: no `nonzero` / `bincount` on the type mask) come
out of the same launch.  'composite_average' weights (`:73-103`) are per arc; a batch carries them as one scale per destination row where
every graph of it allows that, as the host's `CSRByDestination.from_coo` decides for the merged batch - the kernels sum the two forms in a
different order, and the same choice keeps results bit-identical (`tests/test_composite_batch_host.py` executes the descriptor plan in
numpy, `tests/test_gpu_composite_batch.py` compares through the launch, the models and every merging path of the sequencer)."""
from __future__ import annotations

import ctypes as C
import weakref
from types import SimpleNamespace

import numpy as np
import torch

from . import _native as nat
from .composite_graph_class import CompositeGraphObject
from .graph_class import GraphObject
from .sparse import CSRByDestination, SparseMatrix, canonical_device


# (set_mask ptr, output_mask ptr, length) -> (out_index, set_mask, output_mask): the model's `nonzero(set & out)` (GNN.py:269,
# one host synchronisation per new batch) answered from the assembly instead.  The masks are kept alive by the entry, so a
# pointer cannot be recycled while it is registered; entries go when their batch is garbage-collected.
_OUT_INDEX = {}


def lookup_out_index(set_mask, output_mask):
    hit = _OUT_INDEX.get((set_mask.data_ptr(), output_mask.data_ptr(), set_mask.shape[0]))
    # an in-place edit of either mask since the assembly (views share the version counter of their base) makes the entry stale:
    # the caller then derives the index from the masks as they are now
    if hit is None or set_mask._version != hit[3] or output_mask._version != hit[4]: return None
    return hit[0]


# (type_mask ptr, shape) -> (type_nodes, host offsets, type_mask, version): the model's per-type node lists (CompositeGNN._type_lists:
# `nonzero` + `bincount(...).cpu()`, one host synchronisation per new batch) answered from the assembly, like the out index above
_TYPE_LISTS = {}


def lookup_type_lists(type_mask):
    """(node ids grouped by type, ascending inside a type: int32 [N] on the device; host offsets [T + 1]) of a (T, N) type mask that came
    from an assembly and has not been edited since - else None."""
    hit = _TYPE_LISTS.get((type_mask.data_ptr(), tuple(type_mask.shape)))
    if hit is None or type_mask._version != hit[3]: return None
    return hit[0], hit[1]


class DeviceBatch:
    """What `GraphTensor` is to the host path: the merged batch, resident in HBM (same attribute names)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return f"graph_tensor(n={self.nodes.shape[0]}, a={self.arcs.shape[0]}, ndim={self.DIM_NODE_LABEL.tolist()}, " \
               f"adim={self.DIM_ARC_LABEL}, tdim={self.DIM_TARGET}, mode={self.aggregation_mode}, assembled on {self.device})"


class DeviceDataset:
    """All graphs of a homogeneous dataset, concatenated, on the device; `assemble(ids)` merges any subset in one launch."""

    MODES = ('sum', 'average', 'normalized')
    GRAPH_TYPE = GraphObject

    def __init__(self, graphs, focus: str, aggregation_mode: str, device):
        if aggregation_mode not in self.MODES:
            raise ValueError(f"device assembly of {self.GRAPH_TYPE.__name__}s supports {', '.join(self.MODES)} aggregation")
        if any(not type(g) is self.GRAPH_TYPE for g in graphs): raise ValueError(f'this device assembly is built for {self.GRAPH_TYPE.__name__}s')
        # graph focus: the assembled NodeGraph pools ONE graph per data-set entry (a column of 1 / n); an entry that is itself a merge of
        # graphs (its NodeGraph has several columns, reference graph_class.py:407) keeps the host path, which block-diagonalises them
        if focus == 'g' and any(g.NodeGraph.shape[1] != 1 for g in graphs):
            raise ValueError('device assembly pools one graph per data-set entry')
        self.focus, self.mode, self.device = focus, aggregation_mode, canonical_device(device)
        self.G = len(graphs)
        L = {g.nodes.shape[1] for g in graphs}; A = {g.arcs.shape[1] for g in graphs}; T = {g.targets.shape[1] for g in graphs}
        if len(L) != 1 or len(A) != 1 or len(T) != 1: raise ValueError('graphs of one dataset must share label / target widths')
        self.L, self.W, self.T = L.pop(), A.pop(), T.pop()                      # W = 2 + dim_arc_label
        n = np.array([g.nodes.shape[0] for g in graphs], dtype=np.int64)
        e = np.array([g.arcs.shape[0] for g in graphs], dtype=np.int64)
        t = np.array([g.targets.shape[0] for g in graphs], dtype=np.int64)
        m = np.array([len(g.set_mask) for g in graphs], dtype=np.int64)          # mask length: nodes, or arcs for arc focus
        self.n, self.e, self.t, self.m = n, e, t, m
        off = lambda c: np.concatenate([[0], np.cumsum(c)]).astype(np.int64)
        self.noff, self.eoff, self.toff, self.moff = off(n), off(e), off(t), off(m)
        N, E = int(n.sum()), int(e.sum())
        # the whole dataset as ONE block-diagonal graph (ids global), then made graph-local again where they are ids
        nodes = np.concatenate([g.nodes for g in graphs]).astype(np.float32)
        arcs = np.concatenate([g.arcs for g in graphs]).astype(np.float32)       # local ids (float, like the reference)
        gid_arc = np.repeat(np.arange(self.G), e)
        src = np.concatenate([g.arc_ids[:, 0] for g in graphs]).astype(np.int64) + self.noff[gid_arc]
        dst = np.concatenate([g.arc_ids[:, 1] for g in graphs]).astype(np.int64) + self.noff[gid_arc]
        # by destination: Adjacency (rows = source nodes) and ArcNode (rows = arc ids); arcs are sorted by (src, dst) inside a
        # graph and graphs are contiguous, so a stable sort by destination keeps ascending source inside a destination
        indeg = np.bincount(dst, minlength=N)
        order = np.argsort(dst, kind='stable')
        rowptr_g = np.concatenate([[0], np.cumsum(indeg)])[:-1]                  # global exclusive prefix
        gid_node = np.repeat(np.arange(self.G), n)
        self._up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        up = self._up
        self.d_nodes, self.d_arcs = up(nodes), up(arcs)
        self.d_targets = up(np.concatenate([g.targets for g in graphs]).astype(np.float32))
        self.d_sw = up(np.concatenate([np.asarray(g.sample_weight, dtype=np.float32).reshape(-1) for g in graphs]))
        self.d_set = up(np.concatenate([g.set_mask for g in graphs]).astype(np.uint8))
        self.d_out = up(np.concatenate([g.output_mask for g in graphs]).astype(np.uint8))
        self.d_rowptr = up((rowptr_g - self.eoff[gid_node]).astype(np.int32))                     # graph-local row pointers
        self.d_adj_src = up((src[order] - self.noff[gid_arc[order]]).astype(np.int32))            # graph-local source ids by destination
        self.d_an_src = up((order - self.eoff[gid_arc[order]]).astype(np.int32))                  # graph-local arc ids by destination
        self.d_scale = None
        if aggregation_mode == 'average':                                        # 1 / in-degree of the destination (graph_class.py:116-121)
            self.d_scale = up(np.where(indeg > 0, 1.0 / np.maximum(indeg, 1), 1.0).astype(np.float32))
        self.d_asrc, self.d_adst = up(src.astype(np.int32) - self.noff[gid_arc].astype(np.int32)), \
            up(dst.astype(np.int32) - self.noff[gid_arc].astype(np.int32))      # arc end points (arc focus: GNN.py:322-325)
        both = np.concatenate([np.logical_and(g.set_mask, g.output_mask) for g in graphs])         # rows the output network sees (GNN.py:269)
        gid_mask = np.repeat(np.arange(self.G), m)
        self.oc = np.bincount(gid_mask[both], minlength=self.G).astype(np.int64)
        self.ooff = off(self.oc)
        self.d_oidx = up((np.flatnonzero(both) - self.moff[gid_mask[both]]).astype(np.int32))    # graph-local positions
        self._host = dict(src=src, dst=dst, indeg=indeg, order=order, gid_arc=gid_arc, gid_node=gid_node)
        self._by_source_ready = False
        self.hub = bool(indeg.max(initial=0) > 512)                              # hub rows need the host-side split (sparse.split_heavy)
        # staging for the descriptor tables
        self._pinned, self._copy_done = None, None

    def _prepare_by_source(self):
        """Adjacency by SOURCE (the transposed aggregate of the backward pass): built on first use."""
        if self._by_source_ready: return
        h, up = self._host, self._up
        N = int(self.n.sum())
        outdeg = np.bincount(h['src'], minlength=N)
        order = np.argsort(h['src'], kind='stable')                               # arcs are already (src, dst)-sorted: identity inside a graph
        rowptr = np.concatenate([[0], np.cumsum(outdeg)])[:-1]
        self.d_t_rowptr = up((rowptr - self.eoff[h['gid_node']]).astype(np.int32))
        self.d_t_dst = up((h['dst'][order] - self.noff[h['gid_arc'][order]]).astype(np.int32))
        w = self._arc_weights()                                                  # not uniform per source: one weight per arc
        self.d_t_w = None if w is None else up(w[order])
        self._by_source_ready = True

    def _arc_weights(self):
        """float32 weight of every arc of the data set (arc order), or None where one scale per batch row says it all."""
        if self.mode != 'average': return None
        return (1.0 / self._host['indeg'][self._host['dst']]).astype(np.float32)     # 1 / in-degree(dst_e)

    # ------------------------------------------------------------------------------------------------------------------
    def _run(self, descs):
        """descs: list of (src tensor | None, src element offset, dst tensor, dst element offset, count, kind, iadd, fval, width)
        given as parallel numpy arrays per array family; executes them in one launch."""
        n = sum(len(d['count']) for d in descs)
        if n == 0: return
        tab = np.zeros(n, dtype=[('src', '<u8'), ('dst', '<u8'), ('count', '<i8'), ('kind', '<i4'), ('iadd', '<i4'), ('fval', '<f4'), ('width', '<i4')])
        assert tab.dtype.itemsize == C.sizeof(nat.RaggedDesc)
        pos = 0
        for d in descs:
            k = len(d['count'])
            sl = tab[pos:pos + k]
            esz = d['esize']
            sl['src'] = 0 if d['src'] is None else np.uint64(d['src'].data_ptr()) + np.asarray(d['src_off']).astype(np.uint64) * np.uint64(esz)
            sl['dst'] = np.uint64(d['dst'].data_ptr()) + np.asarray(d['dst_off']).astype(np.uint64) * np.uint64(esz)
            sl['count'], sl['kind'] = d['count'], d['kind']
            sl['iadd'], sl['fval'], sl['width'] = d.get('iadd', 0), d.get('fval', 0.0), d.get('width', 0)
            pos += k
        tab = tab[tab['count'] > 0]
        n = len(tab)
        if n == 0: return
        blocks = (tab['count'] + nat.RC_CHUNK - 1) // nat.RC_CHUNK
        blk = np.concatenate([[0], np.cumsum(blocks)]).astype(np.int32)
        nbytes = tab.nbytes + blk.nbytes
        if self._copy_done is not None: self._copy_done.synchronize()           # the previous table has left the staging buffer
        if self._pinned is None or self._pinned.numel() < nbytes:
            self._pinned = torch.empty(max(nbytes * 2, 1 << 16), dtype=torch.uint8).pin_memory()
        stage = self._pinned[:nbytes].numpy()
        stage[:tab.nbytes] = tab.view(np.uint8).reshape(-1)
        stage[tab.nbytes:] = blk.view(np.uint8)
        dev = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        dev.copy_(self._pinned[:nbytes], non_blocking=True)
        if self._copy_done is None: self._copy_done = torch.cuda.Event()
        self._copy_done.record(torch.cuda.current_stream(self.device))
        nat.check(nat.lib().gnn_ragged_copy(C.c_void_p(dev.data_ptr()), n, C.c_void_p(dev.data_ptr() + tab.nbytes), int(blk[-1]),
                                            nat.current_stream(self.device)))
        self._keep = dev                              # until the next assemble on this stream (the launch reads it)

    def assemble(self, ids) -> DeviceBatch:
        """The merged batch of graphs `ids` (dataset indices, in batch order)."""
        return self.assemble_many([ids])[0]

    def assemble_many(self, batches) -> list:
        """Every batch of an epoch at once: `batches` = list of lists of dataset indices.  All batches live in epoch-wide arrays
        (a batch is a run of rows of each) filled by ONE descriptor upload and ONE launch; returns the `DeviceBatch` views."""
        if len(batches) == 0: return []
        p = self.plan(batches)
        self._run(p.D)
        return self.batches_of(p)

    def plan(self, batches) -> SimpleNamespace:
        """The epoch-wide arrays (allocated, not filled) and the descriptor families `D` that fill them: what `_run` executes."""
        nb = len(batches)
        sizes = np.array([len(b) for b in batches], dtype=np.int64)
        ids = np.concatenate([np.asarray(b, dtype=np.int64) for b in batches]) if sizes.sum() else np.zeros(0, np.int64)
        bidx = np.repeat(np.arange(nb), sizes)                                   # batch of every graph
        first = np.concatenate([[0], np.cumsum(sizes)])[:-1]                     # position of each batch's first graph
        dev = self.device
        n, e, t, m = self.n[ids], self.e[ids], self.t[ids], self.m[ids]
        excl = lambda c: np.cumsum(c) - c                                        # exclusive prefix over all graphs = offsets in the epoch arrays
        gn, ge, gt, gm = excl(n), excl(e), excl(t), excl(m)
        tot = lambda c: np.add.reduceat(c, first) if len(c) else np.zeros(nb, np.int64)      # per batch totals (every batch has >= 1 graph)
        Nb, Eb, Tb, Mb = tot(n), tot(e), tot(t), tot(m)
        base = lambda g_: g_[first]                                              # epoch offset of each batch
        bN, bE, bT, bM = base(gn), base(ge), base(gt), base(gm)
        ln, le = gn - bN[bidx], ge - bE[bidx]                                    # node / arc offset of every graph INSIDE its batch
        N, E, Tn, Mn = int(n.sum()), int(e.sum()), int(t.sum()), int(m.sum())
        f32 = lambda *s_: torch.empty(s_, dtype=torch.float32, device=dev)
        i32 = lambda *s_: torch.empty(s_, dtype=torch.int32, device=dev)
        nodes, arcs, targets, sw = f32(N, self.L), f32(E, self.W), f32(Tn, self.T), f32(Tn)
        set_mask, out_mask = torch.empty(Mn, dtype=torch.uint8, device=dev), torch.empty(Mn, dtype=torch.uint8, device=dev)
        rowptr, adj_src, an_src = i32(N + nb), i32(E), i32(E)                    # batch b's row pointers start at bN[b] + b
        asrc, adst = (i32(E), i32(E)) if self.focus == 'a' else (None, None)
        scale = None if self.mode == 'sum' else f32(N)
        no, eo, to_, mo = self.noff[ids], self.eoff[ids], self.toff[ids], self.moff[ids]
        K = nat
        oc = self.oc[ids]
        go = excl(oc)
        Ob, bO = tot(oc), base(go)
        out_index = i32(int(oc.sum()))
        lm = gm - bM[bidx]                                                        # mask offset of every graph inside its batch
        D = [dict(src=self.d_nodes, src_off=no * self.L, dst=nodes, dst_off=gn * self.L, count=n * self.L, kind=K.RC_COPY_F32, esize=4),
             dict(src=self.d_arcs, src_off=eo * self.W, dst=arcs, dst_off=ge * self.W, count=e * self.W, kind=K.RC_COPY_ROWS_ADD2,
                  fval=ln.astype(np.float32), width=self.W, esize=4),
             dict(src=self.d_targets, src_off=to_ * self.T, dst=targets, dst_off=gt * self.T, count=t * self.T, kind=K.RC_COPY_F32, esize=4),
             dict(src=self.d_sw, src_off=to_, dst=sw, dst_off=gt, count=t, kind=K.RC_COPY_F32, esize=4),
             dict(src=self.d_set, src_off=mo, dst=set_mask, dst_off=gm, count=m, kind=K.RC_COPY_U8, esize=1),
             dict(src=self.d_out, src_off=mo, dst=out_mask, dst_off=gm, count=m, kind=K.RC_COPY_U8, esize=1),
             dict(src=self.d_rowptr, src_off=no, dst=rowptr, dst_off=gn + bidx, count=n, kind=K.RC_COPY_I32_ADD, iadd=le.astype(np.int32), esize=4),
             dict(src=None, src_off=np.zeros(nb, np.int64), dst=rowptr, dst_off=bN + Nb + np.arange(nb), count=np.ones(nb, np.int64),
                  kind=K.RC_FILL_I32, iadd=Eb.astype(np.int32), esize=4),
             dict(src=self.d_adj_src, src_off=eo, dst=adj_src, dst_off=ge, count=e, kind=K.RC_COPY_I32_ADD, iadd=ln.astype(np.int32), esize=4),
             dict(src=self.d_an_src, src_off=eo, dst=an_src, dst_off=ge, count=e, kind=K.RC_COPY_I32_ADD, iadd=le.astype(np.int32), esize=4)]
        D.append(dict(src=self.d_oidx, src_off=self.ooff[ids], dst=out_index, dst_off=go, count=oc, kind=K.RC_COPY_I32_ADD, iadd=lm.astype(np.int32), esize=4))
        if self.mode == 'average':
            D.append(dict(src=self.d_scale, src_off=no, dst=scale, dst_off=gn, count=n, kind=K.RC_COPY_F32, esize=4))
        elif self.mode == 'normalized':                                           # 1 / #arcs of the merged graph (graph_class.py:110)
            D.append(dict(src=None, src_off=np.zeros(nb, np.int64), dst=scale, dst_off=bN, count=Nb, kind=K.RC_FILL_F32,
                          fval=(np.float32(1.0) / Eb.astype(np.float32)), esize=4))
        if self.focus == 'a':
            D += [dict(src=self.d_asrc, src_off=eo, dst=asrc, dst_off=ge, count=e, kind=K.RC_COPY_I32_ADD, iadd=ln.astype(np.int32), esize=4),
                  dict(src=self.d_adst, src_off=eo, dst=adst, dst_off=ge, count=e, kind=K.RC_COPY_I32_ADD, iadd=ln.astype(np.int32), esize=4)]
        ng_rowptr = ng_src = ng_scale = None
        if self.focus == 'g':                                                     # NodeGraph[n, g] = 1 / |V_g| (graph_class.py:127-138, :407)
            G = len(ids)
            ng_rowptr, ng_src, ng_scale = i32(G + nb), i32(N), f32(G)
            gpos = np.arange(G) + bidx                                            # slot of graph j's row pointer (batch b's start at first[b] + b)
            D += [dict(src=None, src_off=np.zeros(G, np.int64), dst=ng_rowptr, dst_off=gpos, count=np.ones(G, np.int64), kind=K.RC_FILL_I32,
                       iadd=ln.astype(np.int32), esize=4),
                  dict(src=None, src_off=np.zeros(nb, np.int64), dst=ng_rowptr, dst_off=first + sizes + np.arange(nb), count=np.ones(nb, np.int64),
                       kind=K.RC_FILL_I32, iadd=Nb.astype(np.int32), esize=4),
                  dict(src=None, src_off=np.zeros(nb, np.int64), dst=ng_src, dst_off=bN, count=Nb, kind=K.RC_IOTA_I32, iadd=np.zeros(nb, np.int32), esize=4),
                  dict(src=None, src_off=np.zeros(G, np.int64), dst=ng_scale, dst_off=np.arange(G), count=np.ones(G, np.int64), kind=K.RC_FILL_F32,
                       fval=(np.float32(1.0) / n.astype(np.float32)), esize=4)]
        return SimpleNamespace(D=D, nb=nb, sizes=sizes, ids=ids, bidx=bidx, first=first, n=n, e=e, gn=gn, ge=ge, ln=ln, le=le, no=no, eo=eo,
                               N=N, E=E, Nb=Nb, Eb=Eb, Tb=Tb, Mb=Mb, Ob=Ob, bN=bN, bE=bE, bT=bT, bM=bM, bO=bO, nodes=nodes, arcs=arcs,
                               targets=targets, sw=sw, set_mask=set_mask, out_mask=out_mask, rowptr=rowptr, adj_src=adj_src, an_src=an_src,
                               asrc=asrc, adst=adst, scale=scale, out_index=out_index, ng_rowptr=ng_rowptr, ng_src=ng_src, ng_scale=ng_scale,
                               dim_node_label=torch.tensor([self.L], dtype=torch.int32))        # one (read-only) tensor for every batch of the epoch

    def _weight_form(self, p, b, n0, n1, e0, e1):
        """(w, row_scale) of batch b's Adjacency and ArcNode: one weight per entry, or one scale per destination row."""
        return None, (None if p.scale is None else p.scale[n0:n1])

    def _finish_batch(self, p, b, batch):
        """What a subclass adds to batch b."""

    def batches_of(self, p) -> list:
        """The `DeviceBatch` views of a plan whose descriptors have run."""
        dev, nb = self.device, p.nb
        n, e, gn, ge, ln, le, no, eo, bidx, N, E = p.n, p.e, p.gn, p.ge, p.ln, p.le, p.no, p.eo, p.bidx, p.N, p.E
        f32 = lambda *s_: torch.empty(s_, dtype=torch.float32, device=dev)
        i32 = lambda *s_: torch.empty(s_, dtype=torch.int32, device=dev)
        K = nat
        # the by-source operands of the whole epoch, assembled together on the first request (training only)
        epoch = {}

        def by_source_all():
            if 'rowptr' not in epoch:
                self._prepare_by_source()
                t_rowptr, t_dst = i32(N + nb), i32(E)
                t_w = None if self.d_t_w is None else f32(E)
                DD = [dict(src=self.d_t_rowptr, src_off=no, dst=t_rowptr, dst_off=gn + bidx, count=n, kind=K.RC_COPY_I32_ADD, iadd=le.astype(np.int32), esize=4),
                      dict(src=None, src_off=np.zeros(nb, np.int64), dst=t_rowptr, dst_off=p.bN + p.Nb + np.arange(nb), count=np.ones(nb, np.int64),
                           kind=K.RC_FILL_I32, iadd=p.Eb.astype(np.int32), esize=4),
                      dict(src=self.d_t_dst, src_off=eo, dst=t_dst, dst_off=ge, count=e, kind=K.RC_COPY_I32_ADD, iadd=ln.astype(np.int32), esize=4)]
                if t_w is not None:
                    DD.append(dict(src=self.d_t_w, src_off=eo, dst=t_w, dst_off=ge, count=e, kind=K.RC_COPY_F32, esize=4))
                self._run(DD)
                epoch.update(rowptr=t_rowptr, dst=t_dst, w=t_w)
            return epoch

        out = []
        for b in range(nb):
            n0, n1, e0, e1 = int(p.bN[b]), int(p.bN[b] + p.Nb[b]), int(p.bE[b]), int(p.bE[b] + p.Eb[b])
            t0, t1, m0, m1 = int(p.bT[b]), int(p.bT[b] + p.Tb[b]), int(p.bM[b]), int(p.bM[b] + p.Mb[b])
            Nn, Ee, B = n1 - n0, e1 - e0, int(p.sizes[b])
            b_w, b_scale = self._weight_form(p, b, n0, n1, e0, e1)
            b_arcs = p.arcs[e0:e1]
            csr = dict(rowptr=p.rowptr[n0 + b:n1 + b + 1], w=b_w, row_scale=b_scale, n_dst=Nn, nnz=Ee, max_degree=0)

            def adjacency_by_source(b=b, n0=n0, n1=n1, e0=e0, e1=e1, Nn=Nn, Ee=Ee):
                ep = by_source_all()
                sc = None
                if self.mode == 'normalized':
                    sc = torch.full((Nn,), float(np.float32(1.0) / np.float32(Ee)), dtype=torch.float32, device=dev)
                return dict(rowptr=ep['rowptr'][n0 + b:n1 + b + 1], src=ep['dst'][e0:e1], w=None if ep['w'] is None else ep['w'][e0:e1],
                            row_scale=sc, n_src=Nn, n_dst=Nn, nnz=Ee)

            def arcnode_by_source(b_arcs=b_arcs, b_w=b_w, b_scale=b_scale, e0=e0, e1=e1, Nn=Nn, Ee=Ee):       # one entry per arc: its destination, its weight
                dst_of = b_arcs[:, 1].to(torch.int32).contiguous()
                if b_w is not None: w = by_source_all()['w'][e0:e1]            # (arcs are (src, dst)-sorted: by source IS arc order)
                else: w = None if b_scale is None else b_scale[dst_of.long()].contiguous()
                return dict(rowptr=torch.arange(Ee + 1, dtype=torch.int32, device=dev), src=dst_of, w=w, row_scale=None, n_src=Nn, n_dst=Ee, nnz=Ee)

            adjacency = _LazySparse.make((Nn, Nn), dict(csr, src=p.adj_src[e0:e1], n_src=Nn), dev,
                                         endpoints=(p.asrc[e0:e1], p.adst[e0:e1]) if self.focus == 'a' else None, by_source=adjacency_by_source)
            arcnode = _LazySparse.make((Ee, Nn), dict(csr, src=p.an_src[e0:e1], n_src=Ee), dev, by_source=arcnode_by_source)
            g0 = int(p.first[b])
            adjacency._blocks = np.concatenate([[0], np.cumsum(n[g0:g0 + B])]).astype(np.int64)      # one diagonal block per graph
            if self.focus == 'g':
                b_ngs = p.ng_scale[g0:g0 + B]

                def nodegraph_by_source(rp=p.ng_rowptr[g0 + b:g0 + b + B + 1], b_ngs=b_ngs, Nn=Nn, B=B):
                    # graph of every node = the segment of the batch's (device) row pointers it falls into: no host data, no
                    # synchronisation (repeat_interleave with device repeats waits for its output size: 2 x 50 us per training step)
                    gid = torch.bucketize(torch.arange(Nn, dtype=torch.int32, device=dev), rp[1:], right=True)
                    return dict(rowptr=torch.arange(Nn + 1, dtype=torch.int32, device=dev), src=gid.to(torch.int32),
                                w=b_ngs[gid].contiguous(), row_scale=None, n_src=B, n_dst=Nn, nnz=Nn)

                nodegraph = _LazySparse.make((Nn, B), dict(rowptr=p.ng_rowptr[g0 + b:g0 + b + B + 1], src=p.ng_src[n0:n1], w=None, row_scale=b_ngs,
                                                           n_src=Nn, n_dst=B, nnz=Nn, max_degree=0), dev, by_source=nodegraph_by_source)
            else:
                nodegraph = SparseMatrix(np.zeros((0, 2), np.int64), np.zeros(0, np.float32), (1, 0))     # reference: empty matrix
            b_set, b_out = p.set_mask[m0:m1].view(torch.bool), p.out_mask[m0:m1].view(torch.bool)
            key = (b_set.data_ptr(), b_out.data_ptr(), m1 - m0)
            _OUT_INDEX[key] = (p.out_index[int(p.bO[b]):int(p.bO[b] + p.Ob[b])], b_set, b_out, b_set._version, b_out._version)
            out.append(DeviceBatch(nodes=p.nodes[n0:n1], arcs=b_arcs, targets=p.targets[t0:t1], sample_weight=p.sw[t0:t1],
                                   set_mask=b_set, output_mask=b_out,
                                   DIM_NODE_LABEL=p.dim_node_label, DIM_ARC_LABEL=self.W - 2, DIM_TARGET=self.T,
                                   Adjacency=adjacency, ArcNode=arcnode, NodeGraph=nodegraph, aggregation_mode=self.mode, device=dev,
                                   dtype='float32'))
            weakref.finalize(out[-1], _OUT_INDEX.pop, key, None)
            self._finish_batch(p, b, out[-1])
        return out


class _LazySparse(SparseMatrix):
    """Device-only `SparseMatrix` whose by-source form is assembled on first request (training only)."""

    @classmethod
    def make(cls, dense_shape, csr, device, endpoints=None, by_source=None):
        m = cls.device_only(dense_shape, csr, device, endpoints=endpoints)
        m._by_source_thunk = by_source
        return m

    def by_source(self, device):
        key = ('by_source', str(canonical_device(device)))
        if key not in self._dev:
            self._dev[key] = self._by_source_thunk()
        return self._dev[key]


class CompositeDeviceDataset(DeviceDataset):
    """All graphs of a heterogeneous dataset on the device (reference composite_graph_class.py:142-167 `CompositeGraphObject.merge`): on top
    of the homogeneous arrays a type id per node, every type's node list and the by-destination CSR of every composite adjacency CA_t (the
    Adjacency restricted to arcs that leave a node of type t, :57-70), all graph-local; 'composite_average' weights (:73-103) per arc and per
    (type, node).  `assemble_many` returns batches that also carry `type_mask` (T, N), the T `CompositeAdjacencies` and register their type
    lists (`lookup_type_lists`)."""

    MODES = DeviceDataset.MODES + ('composite_average',)
    GRAPH_TYPE = CompositeGraphObject

    def __init__(self, graphs, focus: str, aggregation_mode: str, device):
        if any(not type(g) is CompositeGraphObject for g in graphs): raise ValueError('this device assembly is built for CompositeGraphObjects')
        dims = {tuple(int(d) for d in g.DIM_NODE_LABEL) for g in graphs}
        if len(dims) != 1: raise ValueError('graphs of one dataset must share DIM_NODE_LABEL')
        self.dims = dims.pop()
        T = self.NT = len(self.dims)
        if T > 255: raise ValueError('device assembly keeps a node\'s type in one byte')
        if any(g.type_mask.ndim != 2 or g.type_mask.shape != (g.nodes.shape[0], T) for g in graphs):
            raise ValueError('type_mask must be (n_nodes, n_types)')
        tm = np.concatenate([g.type_mask for g in graphs], axis=0).astype(bool)
        if not np.all(tm.sum(axis=1) == 1): raise ValueError('type_mask must be one-hot: every node needs exactly one type')
        super().__init__(graphs, focus, aggregation_mode, device)
        h, up, G = self._host, self._up, self.G
        N = int(self.n.sum())
        src, dst, order, gid_arc, gid_node = h['src'], h['dst'], h['order'], h['gid_arc'], h['gid_node']
        excl = lambda c: (np.cumsum(c.reshape(-1)) - c.reshape(-1)).reshape(c.shape)
        tid = tm.argmax(axis=1)
        self.d_tid = up(tid.astype(np.uint8))
        # the nodes of every type: type-major, inside a type by graph, inside a graph ascending (graph-local ids)
        bucket = tid * G + gid_node
        by_type = np.argsort(bucket, kind='stable')
        self.d_tl = up((by_type - self.noff[gid_node[by_type]]).astype(np.int32))
        self.tn = np.bincount(bucket, minlength=T * G).reshape(T, G).astype(np.int64)          # nodes of type t in graph g
        self.tloff = excl(self.tn)
        # CA_t by destination: the Adjacency's by-destination entries whose source has type t, type-major
        atype = tid[src]                                                                        # type of every arc's source
        ca_order = order[np.argsort(atype[order], kind='stable')]
        self.d_ca_src = up((src[ca_order] - self.noff[gid_arc[ca_order]]).astype(np.int32))
        self.ce = np.bincount(atype * G + gid_arc, minlength=T * G).reshape(T, G).astype(np.int64)      # arcs that leave type t in graph g
        self.ceoff = excl(self.ce)
        cnt = np.bincount(atype * N + dst, minlength=T * N).reshape(T, N)                      # in-neighbours of type t of every node
        self.d_ca_rowptr = up((excl(cnt) - self.ceoff[:, gid_node]).astype(np.int32))           # [T, N], graph-local
        self.d_ca_scale = self.d_w_dst = self.d_cavg_scale = None
        self.uniform = np.ones(G, dtype=bool)
        if aggregation_mode == 'composite_average':                                             # w_e = 1 / #(in-neighbours of dst_e with the type of src_e)
            w = np.ones(len(src), dtype=np.float32)
            w /= cnt[atype, dst]                                                                # (float32 /= int64, as buildArcNode divides)
            h['w'] = w
            self.d_w_dst = up(w[order])
            self.d_ca_scale = up((np.ones((T, N), dtype=np.float32) / np.maximum(cnt, 1)).astype(np.float32))
            # a graph whose every destination has equal incoming weights can do with one scale per row (CSRByDestination.from_coo)
            indeg = h['indeg']
            row_first = np.ones(N, dtype=np.float32)
            has = indeg > 0
            row_first[has] = w[order][(np.cumsum(indeg) - indeg)[has]]
            uneven = w[order] != row_first[dst[order]]
            self.uniform = np.bincount(gid_arc[order][uneven], minlength=G) == 0
            self.d_cavg_scale = up(row_first)

    def _arc_weights(self):
        return self._host['w'] if self.mode == 'composite_average' else super()._arc_weights()

    def plan(self, batches) -> SimpleNamespace:
        p = super().plan(batches)
        T, K, dev, nb = self.NT, nat, self.device, p.nb
        ids, bidx, first, n, N, E = p.ids, p.bidx, p.first, p.n, p.N, p.E
        Ntot = int(self.n.sum())
        i32 = lambda *s_: torch.empty(s_, dtype=torch.int32, device=dev)
        rows = lambda c: (np.cumsum(c, axis=1) - c)                              # exclusive prefix along every type's row of a [T, graphs] table
        tile = lambda a: np.tile(a, T)
        t_of = np.repeat(np.arange(T), len(ids))
        p.type_mask = torch.empty(T * N, dtype=torch.uint8, device=dev)          # batch b: (T, Nb[b]) at T * bN[b]
        p.type_nodes = i32(N)                                                     # batch b at bN[b]: type 0's nodes, type 1's, ..
        p.ca_rowptr, p.ca_src = i32(T * (N + nb)), i32(E)                         # type t's row pointers at t * (N + nb), batch b's at + bN[b] + b
        tn, ce = self.tn[:, ids], self.ce[:, ids]
        tn_b = np.add.reduceat(tn, first, axis=1) if len(ids) else np.zeros((T, nb), np.int64)       # [T, nb] nodes of type t in batch b
        p.ce_b = np.add.reduceat(ce, first, axis=1) if len(ids) else np.zeros((T, nb), np.int64)     # [T, nb] entries of CA_t in batch b
        p.type_offsets = np.concatenate([np.zeros((1, nb), np.int64), np.cumsum(tn_b, axis=0)])       # [T + 1, nb]
        tpos = rows(tn); tpos = tpos - tpos[:, first][:, bidx] + p.type_offsets[:-1][:, bidx] + p.bN[bidx]      # slot of (type, graph) in type_nodes
        p.ca_pos = (np.cumsum(ce.reshape(-1)) - ce.reshape(-1)).reshape(ce.shape)                     # slot of (type, graph) in ca_src
        ca_local = p.ca_pos - p.ca_pos[:, first][:, bidx]                                             # entries of (type, batch) in front of the graph
        p.D += [dict(src=self.d_tid, src_off=p.no, dst=p.type_mask, dst_off=T * p.bN[bidx] + p.ln, count=n, kind=K.RC_TYPE_ROWS_U8,
                     iadd=p.Nb[bidx].astype(np.int32), width=T, esize=1),
                dict(src=self.d_tl, src_off=self.tloff[:, ids].reshape(-1), dst=p.type_nodes, dst_off=tpos.reshape(-1), count=tn.reshape(-1),
                     kind=K.RC_COPY_I32_ADD, iadd=tile(p.ln).astype(np.int32), esize=4),
                dict(src=self.d_ca_rowptr, src_off=t_of * Ntot + tile(p.no), dst=p.ca_rowptr, dst_off=t_of * (N + nb) + tile(p.gn + bidx), count=tile(n),
                     kind=K.RC_COPY_I32_ADD, iadd=ca_local.reshape(-1).astype(np.int32), esize=4),
                dict(src=None, src_off=np.zeros(T * nb, np.int64), dst=p.ca_rowptr,
                     dst_off=np.repeat(np.arange(T), nb) * (N + nb) + np.tile(p.bN + p.Nb + np.arange(nb), T), count=np.ones(T * nb, np.int64),
                     kind=K.RC_FILL_I32, iadd=p.ce_b.reshape(-1).astype(np.int32), esize=4),
                dict(src=self.d_ca_src, src_off=self.ceoff[:, ids].reshape(-1), dst=p.ca_src, dst_off=p.ca_pos.reshape(-1), count=ce.reshape(-1),
                     kind=K.RC_COPY_I32_ADD, iadd=tile(p.ln).astype(np.int32), esize=4)]
        p.ca_scale = p.w = None
        p.row_scale_form = np.ones(nb, dtype=bool)
        if self.mode == 'composite_average':
            # Adjacency / ArcNode: one scale per row where every graph of the batch allows it, else one weight per entry (the two forms
            # are summed in a different order by the kernels: the host-merged batch makes the same choice, CSRByDestination.from_coo)
            p.row_scale_form = np.logical_and.reduceat(self.uniform[ids], first) if len(ids) else p.row_scale_form
            by_row = p.row_scale_form[bidx]
            p.ca_scale, p.w = torch.empty(T * N, dtype=torch.float32, device=dev), torch.empty(E, dtype=torch.float32, device=dev)
            p.D += [dict(src=self.d_ca_scale, src_off=t_of * Ntot + tile(p.no), dst=p.ca_scale, dst_off=t_of * N + tile(p.gn), count=tile(n),
                         kind=K.RC_COPY_F32, esize=4),
                    dict(src=self.d_cavg_scale, src_off=p.no, dst=p.scale, dst_off=p.gn, count=n * by_row, kind=K.RC_COPY_F32, esize=4),
                    dict(src=self.d_w_dst, src_off=p.eo, dst=p.w, dst_off=p.ge, count=p.e * ~by_row, kind=K.RC_COPY_F32, esize=4)]
        p.dim_node_label = torch.tensor(self.dims, dtype=torch.int32)
        return p

    def _weight_form(self, p, b, n0, n1, e0, e1):
        if self.mode == 'composite_average' and not p.row_scale_form[b]: return p.w[e0:e1], None
        return super()._weight_form(p, b, n0, n1, e0, e1)

    def _finish_batch(self, p, b, batch):
        T, dev, nb, N = self.NT, self.device, p.nb, p.N
        n0, Nn = int(p.bN[b]), int(p.Nb[b])
        g0 = int(p.first[b])
        batch.type_mask = p.type_mask[T * n0:T * (n0 + Nn)].view(torch.bool).view(T, Nn)
        batch.CompositeAdjacencies = []
        for t in range(T):
            c0, nnz, r0 = int(p.ca_pos[t, g0]), int(p.ce_b[t, b]), t * (N + nb) + n0 + b
            if self.mode == 'composite_average': row_scale = p.ca_scale[t * N + n0:t * N + n0 + Nn]       # 1 / #(in-neighbours of type t)
            else: row_scale = None if p.scale is None else p.scale[n0:n0 + Nn]                           # every CA_t row carries the Adjacency's weight
            csr = dict(rowptr=p.ca_rowptr[r0:r0 + Nn + 1], src=p.ca_src[c0:c0 + nnz], w=None, row_scale=row_scale, n_src=Nn, n_dst=Nn, nnz=nnz,
                       max_degree=0)
            batch.CompositeAdjacencies.append(_LazySparse.make((Nn, Nn), csr, dev, by_source=lambda csr=csr: _csr_by_source(csr, dev)))
        key = (batch.type_mask.data_ptr(), (T, Nn))
        _TYPE_LISTS[key] = (p.type_nodes[n0:n0 + Nn], p.type_offsets[:, b].copy(), batch.type_mask, batch.type_mask._version)
        weakref.finalize(batch, _TYPE_LISTS.pop, key, None)


def _csr_by_source(c: dict, device) -> dict:
    """The by-source form of a square by-destination CSR with one scale per row, on the device (a composite adjacency's backward operand:
    only the building-block training path with chained label gradients reads it - torch ops, no launch of the library)."""
    n, nnz = c['n_dst'], c['nnz']
    dst = torch.bucketize(torch.arange(nnz, dtype=torch.int32, device=device), c['rowptr'][1:].contiguous(), right=True)
    perm = torch.sort(c['src'], stable=True).indices                             # entries are by destination: a stable sort keeps them ascending
    rowptr = torch.zeros(n + 1, dtype=torch.int32, device=device)
    rowptr[1:] = torch.cumsum(torch.bincount(c['src'].long(), minlength=n), 0)
    w = None if c['row_scale'] is None else c['row_scale'][dst][perm].contiguous()
    return dict(rowptr=rowptr, src=dst[perm].to(torch.int32).contiguous(), w=w, row_scale=None, n_src=n, n_dst=n, nnz=nnz)
