"""Heterogeneous batches assembled on the device (gnnkeras_amd/device_batch.py `CompositeDeviceDataset`: the data set uploaded once, a
merged batch = one ragged-copy launch) against the host path (numpy `CompositeGraphObject.merge`, reference composite_graph_class.py:142-167):
the same arrays, the same by-destination CSRs of Adjacency / ArcNode / NodeGraph / every composite adjacency, the same per-type node
lists - and therefore bit-identical results through the models, through a training step, and along every path of the sequencer that
merges graphs (epoch reshuffle, merged batches, shards, the grouped CompositeLGNN propagation)."""
import ctypes as C

import numpy as np
import pytest
import torch

from gnnkeras_amd import CompositeGraphObject
from gnnkeras_amd import _native as nat
from gnnkeras_amd.device_batch import lookup_out_index, lookup_type_lists
from gnnkeras_amd.load_MUTAG import load_composite_graphs
from gnnkeras_amd.Models.training import Adam, SGD, LoopTrainer
from gnnkeras_amd.Sequencers.GraphSequencers import CompositeMultiGraphSequencer, CompositeSingleGraphSequencer
from gnnkeras_amd.sparse import SparseMatrix
from test_gpu_parity import TOL, CCLS
from test_gpu_composite_groups import nets
from test_gpu_composite_grouped import typed_graphs, comp_stack, ONE_RUN
from oracle.harness import rel_err

pytestmark = pytest.mark.gpu
MODES = ['sum', 'average', 'normalized', 'composite_average']
DIMS = {1: (14,), 3: (14, 9, 5)}


@pytest.fixture(scope='module')
def composite_mutag():
    return load_composite_graphs(limit=64)


def typed_mutag(graphs, focus, n_types, mode, seed=3):
    """Composite MUTAG graphs with `n_types` node types: 1 as the loader builds them, or 3 - the atom kind (the hot column of the label)
    modulo 3, label widths (14, 9, 5) - with masks, targets and sample weights of their own for node / arc focus (every graph keeps an
    output row)."""
    rng = np.random.default_rng(seed)
    out = []
    for g in graphs:
        n = g.nodes.shape[0]
        types = np.argmax(g.nodes, axis=1) % n_types
        rows = {'n': n, 'a': g.arcs.shape[0], 'g': n}[focus]
        if focus == 'g': sm, om, targets, sw = np.ones(n, bool), np.ones(n, bool), g.targets, 1
        else:
            sm, om = rng.random(rows) < 0.8, rng.random(rows) < 0.7
            sm[0] = om[0] = True
            targets = np.eye(2)[rng.integers(0, 2, int(om.sum()))]
            sw = rng.uniform(0.5, 1.5, len(targets))
        out.append(CompositeGraphObject(nodes=g.nodes, arcs=g.arcs, targets=targets, type_mask=np.eye(n_types, dtype=bool)[types],
                                        dim_node_label=DIMS[n_types], focus=focus, set_mask=sm, output_mask=om, sample_weight=sw,
                                        aggregation_mode=mode))
    return out


def both(graphs, focus, mode, batch_size, **kw):
    return [CompositeMultiGraphSequencer(graphs, focus, mode, batch_size, shuffle=False, assemble=a, **kw) for a in ('host', 'device')]


def eff_scale(c):
    deg = np.diff(c['rowptr'].cpu().numpy())
    if c['w'] is not None: return c['w'].cpu().numpy()
    s = np.ones(c['n_dst'], np.float32) if c['row_scale'] is None else c['row_scale'].cpu().numpy()
    return np.repeat(s, deg)                  # per entry; rows without entries never matter


def same_matrix(th, td, tag):
    """A sparse member of the sequencer tuple: the CSR the kernels walk, the form of its weights, and the COO triple of the reference's
    tuple (rebuilt lazily from the device CSR)."""
    mh, md = SparseMatrix.from_triple(th), SparseMatrix.from_triple(td)
    ch, cd = mh.device_csr('cuda'), md.device_csr('cuda')
    assert (ch['n_dst'], ch['n_src'], ch['nnz']) == (cd['n_dst'], cd['n_src'], cd['nnz']), tag
    assert torch.equal(ch['rowptr'], cd['rowptr']) and torch.equal(ch['src'], cd['src']), tag
    assert np.array_equal(eff_scale(ch), eff_scale(cd)) and (ch['w'] is None) == (cd['w'] is None), tag
    assert np.array_equal(mh.indices, md.indices) and np.array_equal(mh.values, md.values) and mh.shape == md.shape, tag
    (ih, vh, sh), (idd, vd, sd) = th, td
    assert torch.equal(ih.cpu(), idd.cpu()) and torch.equal(vh.cpu(), vd.cpu()) and torch.equal(sh, sd), tag


def same_item(item_h, item_d, focus, tag=''):
    (xh, yh, wh), (xd, yd, wd) = item_h, item_d
    assert len(xh) == len(xd) == 10
    for j in range(6):                       # nodes, arcs, dim_node_label, type_mask, set_mask, output_mask
        assert xh[j].shape == xd[j].shape and xh[j].dtype == xd[j].dtype and torch.equal(xh[j].cpu(), xd[j].cpu()), (tag, j)
    assert torch.equal(yh, yd) and torch.equal(wh, wd), tag
    assert len(xh[6]) == len(xd[6]) == xh[2].shape[0]
    for t, (a, b) in enumerate(zip(xh[6], xd[6])): same_matrix(a, b, (tag, 'CA', t))
    for j in (7, 8) + ((9,) if focus == 'g' else ()): same_matrix(xh[j], xd[j], (tag, j))


def derived_type_lists(tm):
    t_idx, n_idx = torch.nonzero(tm, as_tuple=True)                   # row-major: grouped by type, ascending node id
    counts = torch.bincount(t_idx, minlength=tm.shape[0]).cpu().numpy()
    return n_idx.to(torch.int32), np.concatenate([[0], np.cumsum(counts)])


@pytest.mark.parametrize('focus', ['g', 'n', 'a'])
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('n_types', [3, 1])
def test_device_assembled_composite_batches_equal_host_merged_ones(composite_mutag, n_types, mode, focus):
    gl = typed_mutag(composite_mutag[:40], focus, n_types, mode)
    host, dev = both(gl, focus, mode, 16)
    assert len(host) == len(dev) == 3 and type(dev.graph_tensors[0]).__name__ == 'DeviceBatch' and type(host.graph_tensors[0]).__name__ != 'DeviceBatch'
    forms = []
    for i in range(3):
        same_item(host[i], dev[i], focus, (n_types, mode, focus, i))
        x = dev[i][0]
        tm, sm, om = x[3].squeeze(-1), x[4].squeeze(-1), x[5].squeeze(-1)
        assert tm.is_contiguous() and tuple(tm.shape) == (n_types, x[0].shape[0])
        got, want = lookup_type_lists(tm), derived_type_lists(tm)
        assert got is not None and torch.equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert torch.equal(lookup_out_index(sm, om), torch.nonzero(torch.logical_and(sm, om)).reshape(-1).to(torch.int32))
        forms.append(SparseMatrix.from_triple(x[7]).device_csr('cuda')['w'] is None)
    if mode == 'composite_average': assert all(forms) == (n_types == 1)       # one type: 'average'; three: some atom is entered from two kinds
    tm[0, 0] = ~tm[0, 0]                                                       # an in-place edit: the assembly's lists no longer answer
    assert lookup_type_lists(tm) is None


@pytest.mark.parametrize('focus', ['n', 'a', 'g'])
@pytest.mark.parametrize('mode', ['average', 'composite_average'])
def test_models_and_training_step_agree_on_both_assemblies(composite_mutag, mode, focus):
    gl = typed_mutag(composite_mutag[:40], focus, 3, mode, seed=5)
    host, dev = both(gl, focus, mode, 16)
    d = 16
    ns, no = nets(DIMS[3], d, focus)
    model = CCLS[focus](ns, no, d, 8, 0.0)
    model.compile(optimizer=SGD(0.0), loss='categorical_crossentropy')
    for i in (0, 2):
        s0 = torch.randn(host[i][0][0].shape[0], d, device='cuda') * 0.1
        kh, sth, oh = model.Loop(*model.process_inputs(host[i][0]), state0=s0)
        kd, std, od = model.Loop(*model.process_inputs(dev[i][0]), state0=s0)
        assert float(kh) == float(kd) == 8 and torch.equal(sth, std) and torch.equal(oh, od)
        for native in (True, False):          # both orchestrations of the training step read the by-source operands
            grads = []
            for seq in (host, dev):
                tr = LoopTrainer(model); tr.use_native_step = native
                res = tr.train_step(*seq[i], state0=s0, apply=False)
                grads.append([g.clone() for h in list(tr.gs) + [tr.go] for g in h.gradients()] + [res['loss'].clone()])
            assert len(grads[0]) == len(grads[1]) > 1
            for a, b in zip(*grads):
                assert torch.allclose(a, b, rtol=1e-5, atol=1e-7)       # scatter-add of arc end points uses float atomics


def test_label_gradients_read_the_composite_adjacencies_by_source(composite_mutag):
    """The by-source form of a CA_t (built on request from the batch's CSR) against the one derived from the host COO."""
    from gnnkeras_amd.Models.training import _by_source
    gl = typed_mutag(composite_mutag[:16], 'n', 3, 'composite_average')
    host, dev = both(gl, 'n', 'composite_average', 16)
    x = torch.randn(host[0][0][0].shape[0], 5, device='cuda')
    from gnnkeras_amd import ops
    for th, td in zip(host[0][0][6], dev[0][0][6]):
        a = ops.aggregate(_by_source(SparseMatrix.from_triple(th), torch.device('cuda', 0)), x)
        b = ops.aggregate(_by_source(SparseMatrix.from_triple(td), torch.device('cuda', 0)), x)
        assert torch.allclose(a, b, rtol=1e-6, atol=1e-7)               # (one scale per row on one side, one weight per entry on the other)


def test_epoch_end_merged_batches_predict_and_shards(composite_mutag):
    gl = typed_mutag(composite_mutag[:40], 'g', 3, 'average')
    seq = CompositeMultiGraphSequencer(list(gl), 'g', 'average', 16, shuffle=True)           # 'auto' = device on a GPU box
    assert type(seq.graph_tensors[0]).__name__ == 'DeviceBatch'
    np.random.seed(4)
    seq.on_epoch_end()
    assert [id(g) for g in seq.data] != [id(g) for g in gl] and type(seq.graph_tensors[0]).__name__ == 'DeviceBatch'
    ref = CompositeMultiGraphSequencer(list(seq.data), 'g', 'average', 16, shuffle=False, assemble='host')
    for i in range(len(seq)): same_item(ref[i], seq[i], 'g', ('epoch', i))
    # merged batches (what predict() / evaluate() group) and the shares of two ranks
    (xh, bh), (xd, bd) = ref.merged_batches(0, 2), seq.merged_batches(0, 2)
    assert bh == bd
    same_item((xh, ref[0][1], ref[0][2]), (xd, seq[0][1], seq[0][2]), 'g', 'merged')
    parts = [seq.shard_item(1, r, 2) for r in range(2)]
    for r in range(2): same_item(ref.shard_item(1, r, 2), parts[r], 'g', ('shard', r))
    assert torch.equal(torch.cat([p[0][0] for p in parts]), seq[1][0][0]) and torch.equal(torch.cat([p[1] for p in parts]), seq[1][1])
    assert torch.equal(torch.cat([p[0][3] for p in parts], dim=1), seq[1][0][3])
    # predict(): state_vect_dim = 0, nothing is drawn
    ns, no = nets(DIMS[3], 0, 'g', scale=0.3)
    model = CCLS['g'](ns, no, 0, 6, 0.0)
    model.compile(optimizer='adam', loss='categorical_crossentropy', metrics=['accuracy'])
    model.group_batches = False
    p_host = np.asarray(model.predict(ref))
    assert np.array_equal(np.asarray(model.predict(seq)), p_host)
    model.group_batches = True                                                   # the batches as convergence groups of one launch
    p_grouped = np.asarray(model.predict(seq))
    assert np.array_equal(p_grouped, np.asarray(model.predict(ref))) and rel_err(p_grouped, p_host) <= TOL
    # the single-graph sequencer stays on the host
    assert CompositeSingleGraphSequencer(gl[0], 'n', 4, shuffle=False).assemble == 'host'


def test_grouped_composite_lgnn_propagation_on_both_assemblies():
    rng = np.random.default_rng(17)
    graphs = typed_graphs(rng, rng.integers(6, 60, 12), 100, 'n', absent=1, lonely=2)
    s0 = [torch.from_numpy(rng.normal(0, 0.1, (g.nodes.shape[0], 6)).astype(np.float32)).cuda() for g in graphs]
    got = {}
    for assemble in ('host', 'device'):
        lg = comp_stack('n', 6, 2, 0.0)
        lg.serial_propagation = 'grouped'
        seq_t0 = CompositeMultiGraphSequencer([g.copy() for g in graphs], 'n', 'composite_average', 4, shuffle=False, assemble=assemble)
        seq_now = seq_t0
        for gnn in lg.gnns:
            seq_now, ks = lg._propagate(gnn, seq_now, seq_t0, s0)
            assert lg.last_propagate == ONE_RUN and ks == [5] * 12 and seq_now.assemble == assemble
        assert (type(seq_now.graph_tensors[0]).__name__ == 'DeviceBatch') == (assemble == 'device')
        got[assemble] = [(g.nodes, g.arcs, np.asarray(g.DIM_NODE_LABEL)) for g in seq_now.data]
    for (nh, ah, dh), (nd, ad, dd) in zip(got['host'], got['device']):
        assert nh.shape[1] > 5 and np.array_equal(nh, nd) and np.array_equal(ah, ad) and np.array_equal(dh, dd)


def test_fit_on_device_assembled_composite_batches(composite_mutag):
    gl = typed_mutag(composite_mutag, 'g', 3, 'composite_average')
    seq = CompositeMultiGraphSequencer(gl, 'g', 'composite_average', 16, shuffle=True, assemble='device')
    ns, no = nets(DIMS[3], 8, 'g')
    model = CCLS['g'](ns, no, 8, 5, 0.01)
    model.compile(optimizer=Adam(0.01), loss='categorical_crossentropy', metrics=['accuracy'])
    np.random.seed(2)
    hist = model.fit(seq, epochs=3, verbose=0)
    assert type(seq.graph_tensors[0]).__name__ == 'DeviceBatch' and hist['loss'][-1] < hist['loss'][0]


def test_ragged_copy_refuses_an_unknown_kind():
    src = torch.arange(8, dtype=torch.float32, device='cuda')
    dst = torch.full((16,), -1.0, device='cuda')
    tab = np.zeros(2, dtype=[('src', '<u8'), ('dst', '<u8'), ('count', '<i8'), ('kind', '<i4'), ('iadd', '<i4'), ('fval', '<f4'), ('width', '<i4')])
    assert tab.dtype.itemsize == C.sizeof(nat.RaggedDesc)
    tab['src'], tab['dst'], tab['count'] = src.data_ptr(), [dst.data_ptr(), dst.data_ptr() + 32], 8
    blk = torch.tensor([0, 1, 2], dtype=torch.int32, device='cuda')

    def run(kinds):
        tab['kind'] = kinds
        d_tab = torch.from_numpy(tab.view(np.uint8).copy()).cuda()
        rc = nat.lib().gnn_ragged_copy(C.c_void_p(d_tab.data_ptr()), 2, C.c_void_p(blk.data_ptr()), 2, nat.current_stream(torch.device('cuda', 0)))
        torch.cuda.synchronize()
        return rc
    assert run([nat.RC_COPY_F32, 8]) != 0 and b'unknown kind 8' in nat.lib().gnn_last_error()
    assert bool(torch.all(dst == -1.0))                                       # not even the table's valid descriptor ran
    assert run([nat.RC_COPY_F32, nat.RC_COPY_F32]) == 0 and torch.equal(dst, torch.cat([src, src]))
