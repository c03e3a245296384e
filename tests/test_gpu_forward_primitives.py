"""The FORWARD building blocks (`gnn_aggregate` / `gnn_aggregate_gated`, `gnn_dense` with the row softmax behind it, `gnn_dropout`,
`gnn_gather_rows`), each ALONE against float64 at the edges of its own dispatch, in the manner of test_gpu_train_primitives.py (whose
plumbing is imported): the three kernels of `launch_aggregate` (16-byte pieces in column blocks of 128 .. 4, the general one, the narrow
one from 4096 rows) with the in-degrees around `gather_sum8`'s eight rows per trip and the second trip behind each capped grid; the five
kernels of `launch_segdense` (thin outputs H <= 4 with their vector / scalar segment paths and the bound of `thin_dense_applies`, the
32-column chunks / 64 x 64 tiles of k_segdense<4> and <1> on either side of 16 384 rows, the row-streaming kernels from 32 768 rows and
the calls that miss one of their conditions); k_softmax_rows on both sides of H = 4; the second trips of k_dropout and k_gather_rows.

Reference: `NumpyPrim.dense` / `NumpyPrim.aggregate` (tests/test_data_parallel.py) for the calls `_Prim` expresses; for `addend`,
`addend_rowidx`, `gate`, `gnn_aggregate_gated` and `gnn_gather_rows` the float64 NumPy restatement below, next to a ctypes call on
`nat.DenseArgs` / `nat.lib()`.  Operands as in the training file: every 2-D operand is a column slice of a wider allocation whose spare
columns hold 9, row-index lists are permutations of a larger row pool, outputs start as NaN (or as 7 where a closed gate must leave the
bits alone).  The measure is `oracle.harness.rel_err` through `dist`, the bar the project's own 1e-5.

`test_forward_teeth` (host only) takes the SAME cases and derives wrong results from their float64 reference - the last row / column /
column block past 128 / everything from the second trip on left old, bias / addend / center / row_scale / per-arc w ignored, a segment's
weight row off by one, the last arc of the rows of in-degree 9 and 17 dropped, a closed gate ignored, a softmax without the max
subtraction - and requires each to miss the bar by a factor of 100."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from gnnkeras_amd import _native as nat
from gnnkeras_amd.Models.training import _Prim
from oracle.torch_train import dropout_keep_mask, mix32
from test_data_parallel import NumpyPrim, _act
from test_gpu_train_primitives import (BAR, CAP, TEETH, Case, _last_col_old, _tail_old, dist, flat, index, outputs, plain_errs, reference, reference_side, run_case,
                                       wide)

ACT = nat.ACTIVATIONS
NAIVE_SOFTMAX = -1              # reference only (a mutant): exp / sum in float32 without the max subtraction


def _dev():
    return torch.device('cuda', 0)


def _rng(*key):
    return np.random.default_rng([1000] + [int(k) for k in key])


def _f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def wide_at(a, dev, pad, col0):
    """`a` as the columns [col0, col0 + width) of a [rows, width + pad] allocation: col0 = 1 moves the base pointer off 16 bytes."""
    a = np.asarray(a, dtype=np.float32)
    full = np.full((a.shape[0], a.shape[1] + pad), 9.0, dtype=np.float32)
    full[:, col0:col0 + a.shape[1]] = a
    return torch.from_numpy(full).to(dev)[:, col0:col0 + a.shape[1]]


def spare_columns_keep_9(t):
    """The columns of the wide allocation outside the slice `t` (a device tensor made by `wide` / `wide_at`)."""
    full = t._base.cpu().numpy()
    col0 = t.storage_offset() % full.shape[1]
    mask = np.ones(full.shape[1], dtype=bool)
    mask[col0:col0 + t.shape[1]] = False
    return bool(np.all(full[:, mask] == 9.0))


def _set(pos, fn):
    def pre(args):
        args[pos] = fn(args[pos])
        return args
    return pre


def kept_bits_errs(got, ref):
    """A closed gate: the output keeps its bits (the reference left it alone) - nothing short of equality passes."""
    return {i: 0.0 if np.array_equal(g, r) else float('inf') for i, (g, r) in enumerate(zip(got, ref))}


def _rows_old(rows):
    def post(outs, old):
        res = []
        for o, p in zip(outs, old):
            o = o.copy()
            o[rows] = p[rows]
            res.append(o)
        return res
    return post


def _cols_from_old(c0):
    def post(outs, old):
        res = []
        for o, p in zip(outs, old):
            o = o.copy()
            o[:, c0:] = p[:, c0:]
            res.append(o)
        return res
    return post


# ----------------------------------------------------------------------------------------------------------------------
# aggregate
# ----------------------------------------------------------------------------------------------------------------------
def dev_aggregate(csr, X, F, out, gate=None):
    if gate is None: return _Prim(_dev()).aggregate(csr, X, F, out)
    c = nat.make_csr(csr)
    nat.check(nat.lib().gnn_aggregate_gated(C.byref(c), nat.ptr(X), X.stride(0), F, nat.ptr(out), out.stride(0), nat.ptr(gate),
                                            nat.current_stream(_dev())))


def ref_aggregate(csr, X, F, out, gate=None):
    if gate is not None and int(gate[0]) == 0: return           # a closed gate: the output keeps its bits
    NumpyPrim(None).aggregate(csr, X, F, out)


AGG = (dev_aggregate, ref_aggregate)


def _agg_degrees(kind, n_dst):
    """'edges': 70 rows with the in-degrees 0, 1, 7, 8, 9, 16, 17 around gather_sum8's eight rows per trip and one row of 300 (the last row: 9).
    'thr': the rows of the narrow kernel's threshold pair (the same for 4095 and 4096 rows), with 16, 17 and 33 for its sixteen arcs per trip.
    'trip': average in-degree 2, the last row 3."""
    rng = _rng(20, len(kind))
    if kind == 'edges':
        deg = rng.integers(0, 13, 70)
        deg[[3, 10, 20, 30, 40, 50, 60, 69]] = [0, 1, 7, 8, 16, 300, 17, 9]
        assert n_dst == 70
    elif kind == 'thr':
        deg = rng.integers(0, 6, 4096)
        deg[[5, 6, 7, 4094, 4095]] = [16, 17, 33, 9, 17]
    else:
        deg = rng.integers(0, 5, n_dst)
        deg[-1] = 3
    return deg[:n_dst]


def _agg_build(kind, n_dst, n_src, F, weights, pad, col0, gate, dev):
    """X = +-(0.5 + |normal|); the LAST source row is 4 x as large, and it is the source of the last arc of every row of in-degree 9 and 17
    ('trip': of every arc of the last row): one arc more or less shows, one row more or less shows.  Arcs are not sorted by source."""
    deg = _agg_degrees(kind, n_dst)
    rng = _rng(21, len(kind), n_src, F)                  # (not keyed by n_dst: the threshold pair shares its rows)
    nnz_all = int(_agg_degrees(kind, 4096 if kind == 'thr' else n_dst).sum())
    src_all, w_all = rng.integers(0, n_src - 1, nnz_all), rng.uniform(0.5, 1.5, nnz_all)
    rs_all = rng.uniform(0.75, 1.25, 4096 if kind == 'thr' else n_dst)
    x = rng.normal(size=(n_src, F))
    x = np.sign(x) * (0.5 + np.abs(x))
    x[-1] *= 4
    rowptr = np.concatenate([[0], np.cumsum(deg)])
    nnz = int(rowptr[-1])
    src, w = src_all[:nnz].copy(), w_all[:nnz].copy()
    last = rowptr[1:][np.isin(deg, (9, 17))] - 1
    src[last], w[last] = n_src - 1, 2.0
    if kind == 'trip': src[rowptr[-2]:] = n_src - 1
    csr = {'n_dst': n_dst, 'n_src': n_src, 'nnz': nnz, 'rowptr': index(rowptr, dev), 'src': index(src, dev),
           'w': flat(w, dev) if weights in ('w', 'both') else None, 'row_scale': flat(rs_all[:n_dst], dev) if weights in ('rs', 'both') else None}
    fill = np.full((n_dst, F), np.nan if gate is None else 7.0)
    args = [csr, wide_at(x, dev, pad, col0), F, wide(fill, dev, pad=pad)]
    if gate is not None: args.append(torch.tensor([gate], dtype=torch.int32, device=dev))
    return args, [3]


def _csr_keep(csr, keep):
    rp = csr['rowptr'].numpy().astype(np.int64)
    dst = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    deg = np.bincount(dst[keep], minlength=len(rp) - 1)
    new = dict(csr)
    new['rowptr'] = torch.from_numpy(np.concatenate([[0], np.cumsum(deg)]).astype(np.int32))
    new['src'] = csr['src'][torch.from_numpy(keep)]
    if csr['w'] is not None: new['w'] = csr['w'][torch.from_numpy(keep)]
    new['nnz'] = int(keep.sum())
    return new


def _drop_last_arc_of_9_17(args):
    rp = args[0]['rowptr'].numpy().astype(np.int64)
    deg = np.diff(rp)
    keep = np.ones(rp[-1], dtype=bool)
    keep[rp[1:][np.isin(deg, (9, 17))] - 1] = False
    if keep.all(): return None
    args[0] = _csr_keep(args[0], keep)
    return args


def _drop_arcs_of_last_row(args):
    rp = args[0]['rowptr'].numpy().astype(np.int64)
    keep = np.ones(rp[-1], dtype=bool)
    keep[rp[-2]:] = False
    if keep.all(): return None
    args[0] = _csr_keep(args[0], keep)
    return args


def _without(key):
    def pre(args):
        args[0] = dict(args[0])
        args[0][key] = None
        return args
    return pre


def _agg_case(block, kind, n_dst, n_src, F, weights, pad=4, col0=0, gate=None, trip_rows=None):
    name = f'{kind}-N{n_dst}-F{F}-{weights}-ld{F + pad}' + (f'-col{col0}' if col0 else '') + ('' if gate is None else f'-gate{gate}')
    if gate == 0:
        mut = [('gate_ignored', _set(4, lambda g: None), None)]
    else:
        mut = [('last_row_old', None, _rows_old([-1])), ('last_col_old', None, _last_col_old), ('arcs_of_the_last_row_dropped', _drop_arcs_of_last_row, None),
               ('last_arc_of_in_degree_9_and_17_dropped', _drop_last_arc_of_9_17, None)]
        if weights in ('w', 'both'): mut.append(('w_ignored', _without('w'), None))
        if weights in ('rs', 'both'): mut.append(('row_scale_ignored', _without('row_scale'), None))
        if F > 128: mut.append(('column_block_past_128_old', None, _cols_from_old(128)))
        if trip_rows: mut.append((f'rows_from_{trip_rows}_old', None, functools.partial(_tail_old, start=trip_rows * F)))
    return Case(block, name, AGG, functools.partial(_agg_build, kind, n_dst, n_src, F, weights, pad, col0, gate),
                kept_bits_errs if gate == 0 else plain_errs, mut)


W4 = ('none', 'w', 'rs', 'both')
AGG_VEC = [_agg_case('aggregate_vec', 'edges', 70, 90, F, wt) for F in (16, 32, 64, 128, 132, 200, 252) for wt in W4]
AGG_UNALIGNED = [_agg_case('aggregate_unaligned', 'edges', 70, 90, F, 'both', pad=pad, col0=col0) for F in (32, 132) for pad, col0 in ((3, 0), (4, 1))]
AGG_GENERAL = [_agg_case('aggregate_general', 'edges', 70, 90, F, W4[i % 4]) for i, F in enumerate((1, 4, 5, 17, 63, 65, 70, 130))]
# (F = 16 on 16-byte rows would be the vec kernel's: ld = 19 keeps it on k_aggregate<16> / k_aggregate_narrow<16>)
AGG_THRESHOLD = [_agg_case('aggregate_narrow_threshold', 'thr', n, 500, F, 'both', pad=3) for F in (3, 16) for n in (4095, 4096)]
AGG_TRIP = [_agg_case('aggregate_second_trip', 'trip', n, 1000, F, wt, trip_rows=n - 1)
            for n, F, wt in ((32769, 128, 'both'), (65537, 64, 'none'), (16385, 70, 'w'), (65537, 14, 'rs'))]
AGG_GATED = [_agg_case('aggregate_gated', 'edges', 70, 90, F, 'both', gate=g) for F in (32, 5) for g in (1, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize('case', AGG_VEC + AGG_UNALIGNED + AGG_GENERAL + AGG_THRESHOLD + AGG_TRIP + AGG_GATED, ids=repr)
def test_aggregate(case):
    """k_aggregate_vec (F in 16 .. 128 and the column blocks above), k_aggregate<G> (any F; 16-byte-unaligned operands), k_aggregate_narrow
    (G <= 16 from 4096 rows), the second trip behind each 4096-workgroup grid, and the gate word of gnn_aggregate_gated."""
    run_case(case)


@pytest.mark.gpu
@pytest.mark.parametrize('F', [3, 16])
def test_aggregate_agrees_across_the_narrow_threshold(F):
    """4095 rows (k_aggregate) and 4096 rows (k_aggregate_narrow) share their first 4095 rows: the two kernels agree on them."""
    outs = []
    for case in AGG_THRESHOLD:
        if f'-F{F}-' not in case.name: continue
        args, _ = case.build(_dev())
        dev_aggregate(*args)
        torch.cuda.synchronize()
        outs.append(args[3].cpu().numpy())
    assert [o.shape[0] for o in outs] == [4095, 4096]
    e = dist(outs[1][:4095], outs[0])
    print(f'PRIM_ERR aggregate_narrow_threshold F{F}-4096-against-4095 out {e:.3e}')
    assert e <= BAR


# ----------------------------------------------------------------------------------------------------------------------
# dense
# ----------------------------------------------------------------------------------------------------------------------
# argument positions of dev_dense / ref_dense
SEGS, WEIGHTS, NOUT, BIAS, ACTIVATION, OUT, WROWS, OUT_ROWIDX, CENTER, ADDEND, ADDEND_ROWIDX, GATE = range(12)


def dev_dense(segs, W, H, bias, act, Y, wrows, out_rowidx, center, addend, addend_rowidx, gate):
    if addend is None and gate is None: return _Prim(_dev()).dense(segs, W, H, bias, act, Y, wrows, out_rowidx, center)
    d = nat.DenseArgs()
    d.M, d.H, d.n_segments = (Y.shape[0] if out_rowidx is None else len(out_rowidx)), H, len(segs)
    for i, (x, ridx) in enumerate(segs):
        d.seg_ptr[i], d.seg_rowidx[i] = x.data_ptr(), (0 if ridx is None else ridx.data_ptr())
        d.seg_ld[i], d.seg_width[i], d.seg_wrow[i] = x.stride(0), x.shape[1], wrows[i]
    d.W, d.ldw, d.bias = W.data_ptr(), W.stride(0), (0 if bias is None else bias.data_ptr())
    if addend is not None:
        d.addend, d.ld_addend = addend.data_ptr(), addend.stride(0)
        d.addend_rowidx = 0 if addend_rowidx is None else addend_rowidx.data_ptr()
    d.activation, d.Y, d.ldy = act, Y.data_ptr(), Y.stride(0)
    d.out_rowidx = 0 if out_rowidx is None else out_rowidx.data_ptr()
    d.gate = 0 if gate is None else gate.data_ptr()
    d.in_center = 0 if center is None else center.data_ptr()
    d.stream = nat.current_stream(_dev())
    nat.check(nat.lib().gnn_dense(C.byref(d)))


def ref_dense(segs, W, H, bias, act, Y, wrows, out_rowidx, center, addend, addend_rowidx, gate):
    """include/gnnloop.h, gnn_dense: Y[orow(m), :H] = act(sum_s (X_s[row_s(m)] - center[wrow_s ..]) . W[wrow_s .., :H] + bias + addend[arow(m), :H])
    when *gate != 0, in float64."""
    if gate is not None and int(gate[0]) == 0: return
    if addend is None and act != NAIVE_SOFTMAX: return NumpyPrim(None).dense(segs, W, H, bias, act, Y, wrows, out_rowidx, center)
    M = Y.shape[0] if out_rowidx is None else len(out_rowidx)
    Wn, z = _f64(W), np.zeros((M, H))
    for (x, ridx), r0 in zip(segs, wrows):
        rows, w = (_f64(x)[:M] if ridx is None else _f64(x)[ridx.numpy().astype(np.int64)]), x.shape[1]
        if center is not None: rows = rows - _f64(center)[r0:r0 + w]
        z += rows @ Wn[r0:r0 + w, :H]
    if bias is not None: z += _f64(bias)[:H]
    if addend is not None: z += (_f64(addend)[:M] if addend_rowidx is None else _f64(addend)[addend_rowidx.numpy().astype(np.int64)])[:, :H]
    if act == NAIVE_SOFTMAX:
        with np.errstate(all='ignore'):
            e = np.exp(z.astype(np.float32))
            y = e / e.sum(1, keepdims=True)
    else:
        y = _act(act, z)
    Y[torch.arange(M) if out_rowidx is None else out_rowidx.long(), :H] = torch.from_numpy(y).to(torch.float32)


DENSE = (dev_dense, ref_dense)


def _spec(M, H, segs, act='linear', wrows=None, bias=True, center=False, out_idx=False, addend=None, gate=None, Mgen=None, key=0,
          kernel='normal', logits=None, trip_rows=None, ypad=3, wscale=None):
    """segs: [(width, pad of its allocation, through a row index?)]; wrows: weight row of each segment (None: one after the other);
    addend: None / 'rows' / 'idx'; Mgen: the rows the inputs are drawn for (a pair of cases with different M shares its first rows);
    kernel = 'eye' + logits: the input IS the logit matrix (the softmax cases)."""
    if wrows is None: wrows = list(np.cumsum([0] + [s[0] for s in segs[:-1]]))
    return dict(M=M, H=H, segs=list(segs), act=act, wrows=[int(r) for r in wrows], bias=bias, center=center, out_idx=out_idx, addend=addend, gate=gate,
                Mgen=Mgen or M, key=key, kernel=kernel, logits=logits, trip_rows=trip_rows, ypad=ypad, wscale=wscale)


def _out_rows(sp):
    """The output rows of the case (a permutation into a Y of Mgen + 13 rows), or None."""
    if not sp['out_idx']: return None
    return _rng(30, sp['Mgen'], sp['key']).permutation(sp['Mgen'] + 13)[:sp['M']]


def _logits(kind, M, H, rng):
    if kind == 'equal': return np.full((M, H), 3.0)
    z = rng.normal(size=(M, H))
    rows = np.arange(0, M, 50)
    z[rows, (rows // 50) % H] = np.where((rows // 50) % 3 == 2, -200.0, 200.0)        # (row 0: + 200)
    return z


def _dense_build(sp, dev):
    M, H, Mgen = sp['M'], sp['H'], sp['Mgen']
    rng = _rng(31, Mgen, H, sp['key'], len(sp['segs']), sum(s[0] for s in sp['segs']))
    K = sum(s[0] for s in sp['segs'])
    w_rows = max(r + s[0] for r, s in zip(sp['wrows'], sp['segs'])) + 1            # (+ 1: the mutant `wrow + 1` stays inside W)
    segs = []
    for width, pad, use_idx in sp['segs']:
        pool = Mgen + 11 if use_idx else Mgen
        x = rng.normal(size=(pool, width)) + (2.0 if sp['center'] else 0.0)
        if sp['logits']: x = _logits(sp['logits'], pool, width, rng)
        rows = rng.permutation(pool)[:Mgen]
        segs.append((wide(x if use_idx else x[:M], dev, pad=pad), index(rows[:M], dev) if use_idx else None))
    Wn = rng.normal(size=(w_rows, H)) * (sp['wscale'] or 1.0 / np.sqrt(K))
    if sp['kernel'] == 'eye': Wn = np.eye(w_rows, H)
    bias = flat(rng.normal(size=H), dev) if sp['bias'] else None
    center = flat(2.0 + 0.1 * rng.normal(size=w_rows), dev) if sp['center'] else None
    addend = addend_rowidx = None
    if sp['addend']:
        pool = Mgen + 17 if sp['addend'] == 'idx' else Mgen
        a = rng.normal(size=(pool, H))
        rows = rng.permutation(pool)[:Mgen]
        addend = wide(a if sp['addend'] == 'idx' else a[:M], dev, pad=4)
        if sp['addend'] == 'idx': addend_rowidx = index(rows[:M], dev)
    orows = _out_rows(sp)
    Y = wide(np.full((M if orows is None else Mgen + 13, H), 7.0 if sp['gate'] == 0 else np.nan), dev, pad=sp['ypad'])
    gate = None if sp['gate'] is None else torch.tensor([sp['gate']], dtype=torch.int32, device=dev)
    return [segs, wide(Wn, dev), H, bias, ACT[sp['act']], Y, list(sp['wrows']), None if orows is None else index(orows, dev), center,
            addend, addend_rowidx, gate], [OUT]


def _dense_case(block, sp, extra=''):
    K = sum(s[0] for s in sp['segs'])
    name = f'M{sp["M"]}-K{K}-H{sp["H"]}-{len(sp["segs"])}seg-{sp["act"]}' + ('' if sp['bias'] else '-nobias') + ('-center' if sp['center'] else '') + \
        ('-outidx' if sp['out_idx'] else '') + (f'-addend_{sp["addend"]}' if sp['addend'] else '') + ('' if sp['gate'] is None else f'-gate{sp["gate"]}') + \
        (f'-{sp["logits"]}' if sp['logits'] else '') + extra
    if sp['gate'] == 0:
        mut = [('gate_ignored', _set(GATE, lambda g: None), None)]
    else:
        orows = _out_rows(sp)
        mut = [('last_row_old', None, _rows_old([-1] if orows is None else [int(orows[-1])])), ('last_col_old', None, _last_col_old)]
        if not (sp['act'] == 'softmax' and (sp['H'] == 1 or sp['logits'])):      # (one class: the softmax is 1 whatever goes in; fixed logits: nothing else does)
            mut.append(('last_wrow_off_by_one', _set(WROWS, lambda w: w[:-1] + [w[-1] + 1]), None))
            if sp['bias']: mut.append(('bias_ignored', _set(BIAS, lambda b: None), None))
            if sp['center']: mut.append(('center_ignored', _set(CENTER, lambda c: None), None))
            if sp['addend']: mut.append(('addend_ignored', _set(ADDEND, lambda a: None), None))
        if sp['logits'] == 'big': mut.append(('softmax_without_the_max_subtraction', _set(ACTIVATION, lambda a: NAIVE_SOFTMAX), None))
        if sp['trip_rows']: mut.append((f'rows_from_{sp["trip_rows"]}_old', None, functools.partial(_tail_old, start=sp['trip_rows'] * sp['H'])))
    return Case(block, name, DENSE, functools.partial(_dense_build, sp), kept_bits_errs if sp['gate'] == 0 else plain_errs, mut)


# ---- thin outputs (k_thin_dense<H>) ----
# a vector-eligible segment (width 8, ld 12) at weight row 6 (no multiple of 4: the centres are read from there), a scalar one (width 5),
# one through a row index (width 4, ld 8: vector-eligible too); weight rows 14 .. 16 are a gap
THIN_SEGS, THIN_WROWS = [(8, 4, False), (5, 3, False), (4, 4, True)], [6, 0, 17]


def _thin_cases():
    cases = []
    for hi, H in enumerate((1, 2, 3, 4)):
        for mi, M in enumerate((1, 7, 8, 9, 129)):
            i = hi * 5 + mi
            sp = _spec(M, H, THIN_SEGS, act=('linear', 'sigmoid', 'softmax')[(hi + mi) % 3], wrows=THIN_WROWS, bias=bool((i // 2) % 2), center=bool(i % 2),
                       out_idx=bool((i // 3) % 2), addend='idx' if i % 4 == 1 else None)
            cases.append(_dense_case('dense_thin', sp))
    for act in ('linear', 'sigmoid', 'softmax'):            # every option at once, per activation
        cases.append(_dense_case('dense_thin', _spec(9, 3, THIN_SEGS, act=act, wrows=THIN_WROWS, center=True, out_idx=True, addend='idx', key=1)))
    cases.append(_dense_case('dense_thin', _spec(9, 2, THIN_SEGS, wrows=THIN_WROWS, addend='rows', gate=0, key=2)))
    # 2048 workgroups x 128 rows = 262 144 rows per trip: the non-softmax second trip
    cases.append(_dense_case('dense_thin', _spec(262145, 3, THIN_SEGS, act='tanh', wrows=THIN_WROWS, center=True, trip_rows=262144)))
    return cases


DENSE_THIN = _thin_cases()


# ---- the bound of the thin kernel (gnnloop.hip, thin_dense_applies) ----
def thin_applies(K, H):
    """`thin_dense_applies`: the weights within 48 KB and the dynamic LDS (weights in whole 16-byte pieces + K centres + a pad) within 64 KB."""
    lds = (((K * H + 3) & ~3) + K + 4) * 4
    return H <= 4 and K * H * 4 <= 48 * 1024 and lds <= 64 * 1024


def thin_boundary(H):
    K = 1
    while thin_applies(K + 1, H): K += 1
    return K


THIN_EDGE = {H: thin_boundary(H) for H in (1, 2, 3)}
# (M = 9, weights 1 / sqrt(K) by `_dense_build`'s default; the pad makes ld a multiple of 4: K % 4 == 0 takes the thin kernel's vector path)
DENSE_THIN_EDGE = [_dense_case('dense_thin_boundary', _spec(9, H, [(K, 3 + (-(K + 3)) % 4, False)], act=act), '-thin' if thin_applies(K, H) else '-segdense')
                   for H in (1, 2, 3) for K in (THIN_EDGE[H], THIN_EDGE[H] + 1) for act in ('linear', 'softmax')]


def test_thin_boundary_is_where_the_dynamic_lds_reaches_64_kb():
    """Host: the K on either side of the rule, recomputed from its formula - at H <= 3 it is the LDS bound that ends the thin kernel, not
    the 48 KB of weights (the launcher once repeated only the latter)."""
    assert THIN_EDGE == {1: 8188, 2: 5460, 3: 4094}
    for H, K in THIN_EDGE.items():
        assert thin_applies(K, H) and not thin_applies(K + 1, H) and (K + 1) * H * 4 <= 48 * 1024


# ---- k_segdense<4> / k_segdense<1> ----
def _six(K):
    """Six segments of K columns in all whose borders do not fall on the 32-column chunks (K >= 97: 14 | 14 | 3 | 64 | 1 | K - 96)."""
    widths = [14, 14, 3, 64, 1, K - 96] if K >= 97 else [5, 9, 3, 1, 7, K - 25]
    assert min(widths) >= 1 and sum(widths) == K
    return [(w, 3, s in (1, 4)) for s, w in enumerate(widths)]


def _six_wrows(K):
    """The segments' weight rows in another order than the segments, with a gap of 2 rows in front of the last."""
    widths = [s[0] for s in _six(K)]
    order, at, pos = (3, 0, 5, 1, 4, 2), {}, 0
    for s in order:
        if s == order[-1]: pos += 2
        at[s] = pos
        pos += widths[s]
    return [at[s] for s in range(6)]


SEG_K, SEG_HM = (31, 32, 33, 127, 128, 129, 160), [(H, M) for H in (5, 63, 64, 65, 129) for M in (1, 63, 64, 65)]
SEG_ACTS = ['linear', 'relu', 'selu', 'tanh', 'sigmoid', 'elu', 'softplus', 'softmax']


def _segdense_cases():
    ks = [(K, six) for K in SEG_K for six in (False, True)]
    cases = []
    for i, (H, M) in enumerate(SEG_HM):                     # H x M in full, K x segments in full (14 pairs over 20 cases), the options in turn
        K, six = ks[i % len(ks)]
        sp = _spec(M, H, _six(K) if six else [(K, 3, False)], act=SEG_ACTS[i % 7], wrows=_six_wrows(K) if six else [1], bias=i % 3 != 0, center=i % 2 == 1,
                   out_idx=i % 4 >= 2, addend=(None, 'idx', 'rows')[i % 3])
        cases.append(_dense_case('dense_segdense', sp))
    cases.append(_dense_case('dense_segdense', _spec(65, 65, _six(129), wrows=_six_wrows(129), center=True, out_idx=True, addend='idx', gate=0, key=1)))
    cases.append(_dense_case('dense_segdense', _spec(65, 65, _six(129), wrows=_six_wrows(129), center=True, out_idx=True, addend='idx', gate=1, key=1)))
    for act in SEG_ACTS:                                    # all eight at one shape; softmax: k_segdense + k_softmax_rows
        cases.append(_dense_case('dense_segdense', _spec(65, 65, _six(33), act=act, wrows=_six_wrows(33), key=2)))
    for M in (16384, 16385):                                # k_segdense<4> | k_segdense<1>
        cases.append(_dense_case('dense_segdense', _spec(M, 5, _six(33), act='tanh', wrows=_six_wrows(33), center=True, addend='idx', Mgen=16385, key=3)))
    return cases


DENSE_SEG = _segdense_cases()


# ---- k_rowdense / k_rowdense_wide from 32 768 rows, and the calls one condition off ----
def _rowdense_cases():
    R = 32768
    cases = [_dense_case('dense_rowdense', _spec(M, 24, [(48, 4, False)], act='tanh', Mgen=R, ypad=4), '-pair') for M in (R - 1, R)]
    cases += [_dense_case('dense_rowdense', _spec(R, 24, [(50, 2, False)], act='tanh', ypad=4), '-width50'),
              _dense_case('dense_rowdense', _spec(R, 24, [(48, 3, False)], act='tanh', ypad=4), '-ld51'),
              _dense_case('dense_rowdense', _spec(R, 24, [(48, 4, True)], act='tanh', ypad=4), '-rowidx'),
              _dense_case('dense_rowdense', _spec(R, 66, [(48, 4, False)], act='tanh', ypad=2), '-H66')]
    for H in (68, 132):
        for addend in (None, 'rows'):
            cases.append(_dense_case('dense_rowdense_wide', _spec(R, H, [(64, 4, False), (20, 4, False)], act='tanh', addend=addend, ypad=4)))
    return cases


DENSE_ROW = _rowdense_cases()


# ---- softmax rows: the thin kernel's own (H <= 4) and k_softmax_rows ----
SOFTMAX = [_dense_case('softmax_rows', _spec(M, H, [(H, 3, False)], act='softmax', bias=False, out_idx=out_idx, kernel='eye', logits=logits))
           for H in (1, 2, 4, 5, 70) for M in (1, 257) for logits, out_idx in (('big', False), ('big', True), ('equal', False))]

ALL_DENSE = DENSE_THIN + DENSE_THIN_EDGE + DENSE_SEG + DENSE_ROW + SOFTMAX


@pytest.mark.gpu
@pytest.mark.parametrize('case', ALL_DENSE, ids=repr)
def test_dense(case):
    """gnn_dense on k_thin_dense<1 .. 4> (and on either side of its bound), k_segdense<4> / <1>, k_rowdense, k_rowdense_wide and the calls
    that miss one of their conditions, the softmax finished in the thin kernel or by k_softmax_rows.  A call the library refuses fails
    here: `nat.check` raises on a status other than 0."""
    run_case(case)


def _device_result(case):
    args, _ = case.build(_dev())
    dev_dense(*args)
    torch.cuda.synchronize()
    return args[OUT].cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize('block,tag,M', [('dense_segdense', '-addend_idx', 16384), ('dense_rowdense', '-pair', 32767)])
def test_dense_agrees_across_a_kernel_switch(block, tag, M):
    """The same rows on either side of M = 16 384 (k_segdense<4> | <1>) and of M = 32 768 (k_segdense<1> | k_rowdense)."""
    pair = [c for c in ALL_DENSE if c.block == block and c.name.startswith((f'M{M}-', f'M{M + 1}-')) and tag in c.name]
    assert len(pair) == 2
    small, large = (_device_result(c) for c in pair)
    assert small.shape[0] == M and large.shape[0] == M + 1
    e = dist(large[:M], small)
    print(f'PRIM_ERR {block} M{M + 1}-against-M{M} Y {e:.3e}')
    assert e <= BAR


# ----------------------------------------------------------------------------------------------------------------------
# dropout
# ----------------------------------------------------------------------------------------------------------------------
ALPHA_P = -1.6732632423543772 * 1.0507009873554805


def _dropout_want(x, keep, rate, alpha, backward):
    r, x = float(np.float32(rate)), x.astype(np.float64)
    if not alpha: return np.where(keep, x / (1 - r), 0.0)
    a = ((1 - r) * (1 + r * ALPHA_P ** 2)) ** -0.5
    return np.where(keep, x * a, 0.0) if backward else a * np.where(keep, x, ALPHA_P) + (-a * ALPHA_P * r)


@pytest.mark.gpu
@pytest.mark.parametrize('alpha', [0, 1])
@pytest.mark.parametrize('backward', [0, 1])
def test_dropout_second_trip(alpha, backward):
    """k_dropout at M * H = 1 048 576 + 257 elements (the grid-stride loop's second trip), ld > H, out of place and in place, against
    `oracle.torch_train.dropout_keep_mask`; the spare columns keep their 9."""
    dev, H, rate = _dev(), 9, 0.3
    M = (CAP + 257) // H
    assert M * H == CAP + 257
    x = _rng(40).normal(size=(M, H)).astype(np.float32)
    key = mix32(7, alpha, backward, M)
    want = _dropout_want(x, dropout_keep_mask(key, M, H, rate), rate, alpha, backward)
    xd, out, inplace = wide(x, dev), wide(np.full((M, H), np.nan), dev), wide(x, dev)
    p = _Prim(dev)
    p.dropout(xd, out, rate, key, alpha, backward)
    p.dropout(inplace, inplace, rate, key, alpha, backward)
    torch.cuda.synchronize()
    errs = {'out': dist(out.cpu().numpy(), want), 'inplace': dist(inplace.cpu().numpy(), want),
            'tail_out': dist(out.cpu().numpy().reshape(-1)[CAP:], want.reshape(-1)[CAP:])}
    for k, e in errs.items(): print(f'PRIM_ERR dropout alpha{alpha}-backward{backward}-M{M}-H{H} {k} {e:.3e}')
    assert all(e <= BAR for e in errs.values()), errs
    assert np.array_equal(xd.cpu().numpy(), x) and all(spare_columns_keep_9(t) for t in (xd, out, inplace))


@pytest.mark.gpu
@pytest.mark.parametrize('alpha', [0, 1])
def test_dropout_rate_0_is_the_identity(alpha):
    dev = _dev()
    x = _rng(41).normal(size=(257, 5)).astype(np.float32)
    for backward in (0, 1):
        out = wide(np.full(x.shape, np.nan), dev)
        _Prim(dev).dropout(wide(x, dev), out, 0.0, mix32(3, alpha), alpha, backward)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), x) and spare_columns_keep_9(out)


# ----------------------------------------------------------------------------------------------------------------------
# gather_rows
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('M,width,pad', [(1, 1, 3), (300, 1, 3), (1, 5, 3), (300, 5, 3), (1, 64, 4), (300, 64, 4), (300, 64, 3), (1, 130, 3), (300, 130, 2),
                                         ((CAP + 3) // 7, 7, 1), (CAP // 16 + 1, 64, 4)])
def test_gather_rows(M, width, pad):
    """k_gather_rows: 16 bytes per lane (width and both leading dimensions multiples of 4) or element by element, an index list with
    repeats, the second trip of either form (M * width = 1 048 576 + 3; M * width / 4 = 1 048 576 + 16): the bits of NumPy's fancy
    indexing, and the destination's spare columns keep their 9."""
    dev = _dev()
    rng = _rng(42, M, width)
    pool = min(M, 1000) + 17
    src = rng.normal(size=(pool, width)).astype(np.float32)
    idx = rng.integers(0, pool, M)
    if M > 1: idx[1] = idx[0]
    s, d, i = wide(src, dev, pad=pad), wide(np.full((M, width), np.nan), dev, pad=pad), index(idx, dev)
    nat.check(nat.lib().gnn_gather_rows(nat.ptr(s), s.stride(0), nat.ptr(i), M, width, nat.ptr(d), d.stride(0), nat.current_stream(dev)))
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), src[idx]) and spare_columns_keep_9(d) and np.array_equal(s.cpu().numpy(), src)


# ----------------------------------------------------------------------------------------------------------------------
# teeth (host only)
# ----------------------------------------------------------------------------------------------------------------------
FORWARD_CASES = AGG_VEC + AGG_UNALIGNED + AGG_GENERAL + AGG_THRESHOLD + AGG_TRIP + AGG_GATED + ALL_DENSE


def test_forward_case_names_are_unique():
    assert len({repr(c) for c in FORWARD_CASES}) == len(FORWARD_CASES)


@pytest.mark.parametrize('case', FORWARD_CASES, ids=repr)
def test_forward_teeth(case):
    """Every aggregate / dense / softmax case tells a wrong kernel from a right one: each mutant derived from its float64 reference
    misses the bar by a factor of 100 under the case's own measure.  A case without an applicable mutant fails here."""
    ref, old = reference(case)
    assert case.mutants
    applied = 0
    for name, pre, post in case.mutants:
        if pre is not None:
            args, outs = case.build('cpu')
            args = pre(list(args))
            if args is None: continue
            reference_side(case.method)(*args)
            mutant = outputs(args, outs)
        else:
            mutant = [r.copy() for r in ref]
        if post is not None: mutant = post(mutant, old)
        worst = max(case.errs(mutant, ref).values())
        assert worst >= TEETH * BAR, (name, worst)
        applied += 1
    assert applied > 0
