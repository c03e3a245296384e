"""The training building blocks (include/gnnloop.h "training building blocks", csrc/train_api.hpp, driven by `training._Prim`), each
ALONE against float64 at the boundaries of its own kernel: the row counts at which `gnn_colstats` changes kernel (8192) and chunk size
(65536), the 64-wide K / H tiles of the weight-gradient GEMM, the 64-lane stride of `k_first_layer_param_grads`, the second trip of
every grid-stride loop behind a capped grid (4096 workgroups of 256 threads = 1 048 576 elements), the two launches and the
1024-workgroup cap of `gnn_adam_multi`, the clip edges of the losses.  The whole-step gradient tests (test_gpu_training.py, the
training fuzz) reach none of them: they run at MUTAG-like shapes.

Reference: `tests/test_data_parallel.py::NumpyPrim`, every `_Prim` method restated in float64 NumPy.  `both()` runs the two on the same
float32 inputs.  Every 2-D operand with a leading dimension is a column slice of a wider allocation (ld > width) whose spare columns
hold 9; row indices are permutations of a larger row pool.  The measure is `oracle.harness.rel_err`, the bar the project's own 1e-5
(`BAR`); nothing here needed a wider one.

`test_teeth` (host only) takes the SAME cases and derives wrong results from the reference - the last row dropped, the last column
left at its old value, `accumulate` / `center` / `centered` taken the other way, everything from row 8192 / 65536 on dropped, elements
from 1 048 576 on left unwritten - and requires each to miss the bar by a factor of 100 under the case's own measure: the inputs are
shaped so that they do (outlier last rows, outputs pre-filled with values that cannot pass for a result)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from gnnkeras_amd import _native as nat
from gnnkeras_amd.Models.MLP import BN_EPSILON, BN_MOMENTUM
from gnnkeras_amd.Models.training import _Prim
from oracle import torch_train
from oracle.harness import rel_err
from test_data_parallel import NumpyPrim, _act

BAR = 1e-5                      # check_step, test_piecewise_ops_match_oracle, test_dense_entry_large_batches
TEETH = 100.0                   # a mutant must miss the bar by this factor
CAP = 256 * 16 * 256            # elements one trip of a capped grid-stride launch covers (train_api.hpp)
ACT = nat.ACTIVATIONS


def _dev():
    return torch.device('cuda', 0)


# ----------------------------------------------------------------------------------------------------------------------
# plumbing
# ----------------------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def wide(a, dev, pad=3):
    """`a` [rows, width] as a column slice of a [rows, width + pad] allocation on `dev` (spare columns = 9)."""
    a = np.asarray(a, dtype=np.float32)
    full = np.full((a.shape[0], a.shape[1] + pad), 9.0, dtype=np.float32)
    full[:, :a.shape[1]] = a
    return torch.from_numpy(full).to(dev)[:, :a.shape[1]]


def flat(a, dev):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).to(dev)


def index(a, dev):
    return torch.from_numpy(np.asarray(a, dtype=np.int32)).to(dev)


def _map(fn, a):
    if isinstance(a, torch.Tensor): return fn(a)
    if isinstance(a, tuple): return tuple(_map(fn, t) for t in a)
    if isinstance(a, list): return [_map(fn, t) for t in a]
    if isinstance(a, dict): return {k: _map(fn, t) for k, t in a.items()}
    return a


def device_side(method):
    """`method`: the name of a `_Prim` method, or a pair of callables (device call, float64 reference) for what `_Prim` does not express."""
    return method[0] if isinstance(method, tuple) else getattr(_Prim(_dev()), method)


def reference_side(method):
    return method[1] if isinstance(method, tuple) else getattr(NumpyPrim(None), method)


def both(method, *args):
    """`_Prim(cuda).method(*args)` on the device tensors and `NumpyPrim(None).method` on CPU clones of the same float32 inputs (taken
    before the device call: an output's old value is an input; one clone per tensor object, so aliases stay aliases).  Returns both
    argument lists afterwards, tensors as NumPy arrays.  `method` may be a pair of callables (`device_side`)."""
    memo = {}

    def clone(t):
        if id(t) not in memo: memo[id(t)] = t.detach().cpu().clone()
        return memo[id(t)]
    ref_args = [_map(clone, a) for a in args]
    device_side(method)(*args)
    torch.cuda.synchronize()
    reference_side(method)(*ref_args)
    out = lambda t: t.detach().cpu().numpy()
    return [_map(out, a) for a in args], [_map(out, a) for a in ref_args]


def dist(a, b):
    """rel_err, infinite where one side is not finite and the other is (an unwritten NaN can never pass)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isfinite(a), np.isfinite(b)): return float('inf')
    ok = np.isfinite(b)
    return rel_err(a[ok], b[ok])


def plain_errs(got, ref):
    return {i: dist(g, r) for i, (g, r) in enumerate(zip(got, ref))}


class Case:
    """One call of one building block.  `build(dev)` -> (args, indices of the output arguments); `errs(got, ref)` -> {name: error} over
    the output arrays; `mutants`: [(name, pre(args) -> args | None, post(outs, old outs) -> outs | None)] for `test_teeth`."""

    def __init__(self, block, name, method, build, errs=plain_errs, mutants=()):
        self.block, self.name, self.method, self.build, self.errs, self.mutants = block, name, method, build, errs, list(mutants)

    def __repr__(self):
        return f'{self.block}-{self.name}'


def outputs(args, outs):
    return [np.array(args[i].detach().cpu().numpy() if isinstance(args[i], torch.Tensor) else args[i]) for i in outs]


def run_case(case):
    """The device against the reference; prints the figures (`PRIM_ERR block case output error`) before it asserts."""
    args, outs = case.build(_dev())
    got, ref = both(case.method, *args)
    errs = case.errs([got[i] for i in outs], [ref[i] for i in outs])
    for k, e in errs.items(): print(f'PRIM_ERR {case.block} {case.name} {k} {e:.3e}')
    assert errs and all(e <= BAR for e in errs.values()), errs


def reference(case, pre=None):
    args, outs = case.build('cpu')
    old = outputs(args, outs)
    if pre is not None: args = pre(list(args))
    reference_side(case.method)(*args)
    return outputs(args, outs), old


def _last_col_old(outs, old):
    res = []
    for o, p in zip(outs, old):
        o = o.copy()
        o[..., -1] = p[..., -1]
        res.append(o)
    return res


def _tail_old(outs, old, start=CAP):
    """Elements from `start` on (in the order the kernel numbers them: row-major over the logical [M, width]) keep their old value."""
    res = []
    for o, p in zip(outs, old):
        o = o.copy()
        o.reshape(-1)[start:] = p.reshape(-1)[start:]
        res.append(o)
    return res


# ----------------------------------------------------------------------------------------------------------------------
# colstats
# ----------------------------------------------------------------------------------------------------------------------
def _colstats_input(M, K, use_idx):
    """Column 0 = 50 + 0.05 normal (a one-pass variance loses it), column 1 = the constant 3.25, the rest normal.  The LAST row is an
    outlier in column 0 (50 + 5: still 0.1 sigma^2 .. sigma^2 of variance against a mean of 50) - one row more or less shows."""
    rng = _rng(1, M, K, use_idx)
    pool = M + 37 if use_idx else M
    x = rng.normal(size=(pool, K))
    x[:, 0] = 50 + 0.05 * rng.normal(size=pool)
    if K > 1: x[:, 1] = 3.25
    rows = rng.permutation(pool)[:M] if use_idx else np.arange(M)
    x[rows[-1], 0] = 55.0
    return x, rows


def _colstats_build(M, K, use_idx, dev):
    x, rows = _colstats_input(M, K, use_idx)
    mean, var = flat(np.full(K, 7.0), dev), flat(np.full(K, 7.0), dev)
    return (wide(x, dev), index(rows, dev) if use_idx else None, M, mean, var), [3, 4]


def _colstats_errs(got, ref):
    """mean by rel_err; 1 / sqrt(var + eps) column by column: what every consumer of the statistics forms."""
    rs = lambda v: 1.0 / np.sqrt(np.asarray(v, dtype=np.float64) + BN_EPSILON)
    return {'mean': dist(got[0], ref[0]),
            'rstd': max(dist(rs(got[1])[k:k + 1], rs(ref[1])[k:k + 1]) for k in range(len(ref[1])))}


def _drop_rows_from(pos_x, pos_idx, pos_M, extra, at):
    """pre(): the rows from `at` on are not there (x by position or through the index; `extra`: further per-row operands)."""
    def pre(args):
        M = args[pos_M]
        keep = M + at if at < 0 else at
        if not 0 <= keep < M: return None
        if args[pos_idx] is not None: args[pos_idx] = args[pos_idx][:keep]
        for e in extra: args[e] = args[e][:keep]
        args[pos_M] = keep
        return args
    return pre


def _colstats_cases():
    shapes = [(M, 65) for M in (1, 255, 256, 257, 8191, 8192, 8193, 65537)]
    shapes += [(M, K) for M in (257, 8193) for K in (1, 63, 64, 130)]
    cases = []
    for M, K in shapes:
        for use_idx in (False, True):
            mut = [('last_col_old', None, _last_col_old)]
            if M > 1: mut.append(('last_row_dropped', _drop_rows_from(0, 1, 2, (), -1), None))
            for edge in (8192, 65536):
                if M > edge: mut.append((f'from_row_{edge}_dropped', _drop_rows_from(0, 1, 2, (), edge), None))
            cases.append(Case('colstats', f'M{M}-K{K}-{"idx" if use_idx else "rows"}', 'colstats',
                              functools.partial(_colstats_build, M, K, use_idx), _colstats_errs, mut))
    return cases


COLSTATS = _colstats_cases()


@pytest.mark.gpu
@pytest.mark.parametrize('case', COLSTATS, ids=repr)
def test_colstats(case):
    """k_colstats_small (M <= 8192, 32 rows per thread in registers) / the two-pass partial path (64-row chunks, 128 above 65536 rows)."""
    run_case(case)


@pytest.mark.gpu
@pytest.mark.parametrize('M', [8192, 8193])
def test_colstats_moving_statistics(M):
    """`gnn_colstats` with moving statistics (the call of `_Prim.colstats` + the moving pair), once on each side of M = 8192: the pair
    follows m * 0.99 + batch * 0.01; with a gate word of 0 it keeps its bits while mean / var are still written."""
    dev, K = _dev(), 65
    (x, _, _, mean, var), _ = _colstats_build(M, K, False, dev)
    rng = _rng(2, M)
    mm0, mv0 = rng.normal(size=K).astype(np.float32), rng.uniform(0.5, 2.0, K).astype(np.float32)
    ref_mean, ref_var = torch.zeros(K), torch.zeros(K)
    NumpyPrim(None).colstats(x.cpu(), None, M, ref_mean, ref_var)
    lib, p = nat.lib(), _Prim(dev)
    nb = lib.gnn_colstats_workspace_bytes(K, M)
    ws = p.ws(nb)
    for gate_val in (None, 1, 0):
        gate = None if gate_val is None else torch.tensor([gate_val], dtype=torch.int32, device=dev)
        mm, mv = flat(mm0, dev), flat(mv0, dev)
        mean.fill_(float('nan')); var.fill_(float('nan'))
        nat.check(lib.gnn_colstats(nat.ptr(x), x.stride(0), None, K, M, nat.ptr(mean), nat.ptr(var), nat.ptr(mm), nat.ptr(mv),
                                   BN_MOMENTUM, nat.ptr(gate), nat.ptr(ws), ws.numel(), p.stream()))
        torch.cuda.synchronize()
        errs = _colstats_errs([mean.cpu().numpy(), var.cpu().numpy()], [ref_mean.numpy(), ref_var.numpy()])
        if gate_val == 0:
            assert np.array_equal(mm.cpu().numpy(), mm0) and np.array_equal(mv.cpu().numpy(), mv0)
        else:
            errs['moving_mean'] = dist(mm.cpu().numpy(), mm0.astype(np.float64) * 0.99 + ref_mean.numpy().astype(np.float64) * 0.01)
            errs['moving_var'] = dist(mv.cpu().numpy(), mv0.astype(np.float64) * 0.99 + ref_var.numpy().astype(np.float64) * 0.01)
        for k, e in errs.items(): print(f'PRIM_ERR colstats_moving M{M}-gate{gate_val} {k} {e:.3e}')
        assert all(e <= BAR for e in errs.values()), (gate_val, errs)


# ----------------------------------------------------------------------------------------------------------------------
# dense_grad
# ----------------------------------------------------------------------------------------------------------------------
def _dense_grad_build(K, H, M, accumulate, with_q, center, use_idx, dev):
    """P and q start as normals (accumulate = 0 must overwrite them, 1 must add to them).  The last row of x and dZ is 4 x as large as
    the others: one row among 65 537 still moves the largest entry of P by more than 1e-3 of it."""
    rng = _rng(3, K, H, M, accumulate, with_q, center, use_idx)
    pool = M + 29 if use_idx else M
    x = rng.normal(size=(pool, K)) + (2.0 if center else 0.0)
    dz = rng.normal(size=(M, H))
    rows = rng.permutation(pool)[:M] if use_idx else np.arange(M)
    if M > 0: x[rows[-1]] *= 4; dz[-1] *= 4
    cen = flat(2.0 + 0.1 * rng.normal(size=K), dev) if center else None
    P, q = flat(rng.normal(size=(K, H)), dev), (flat(rng.normal(size=H), dev) if with_q else None)
    return (wide(x, dev), index(rows, dev) if use_idx else None, wide(dz, dev), M, P, q, accumulate, cen), ([4, 5] if with_q else [4])


def _set(pos, fn):
    def pre(args):
        args[pos] = fn(args[pos])
        return args
    return pre


def _dense_grad_cases():
    specs = [(K, H, 65, 0, True, False, False) for K, H in ((1, 1), (63, 65), (64, 64), (65, 63), (130, 37))]
    specs += [(65, 63, M, 0, True, False, False) for M in (0, 1, 63, 64, 4097, 65537)]
    specs += [(130, 37, 4097, a, q, c, i) for a, q, c, i in ((0, True, False, False), (1, True, False, False), (0, False, False, False),
                                                              (1, False, False, False), (0, True, True, False), (1, True, True, True),
                                                              (0, True, False, True))]
    specs += [(65, 63, 0, 1, True, False, False), (130, 37, 0, 0, False, False, False)]
    cases = []
    for K, H, M, acc, with_q, center, use_idx in specs:
        mut = [('accumulate_taken_the_other_way', _set(6, lambda a: 1 - a), None)]
        if M > 0 or not acc: mut.append(('last_col_old', None, _last_col_old))          # (M = 0, accumulate = 1: the old value IS the result)
        if M > 0: mut.append(('last_row_dropped', _drop_rows_from(0, 1, 3, (2,), -1), None))
        if center: mut.append(('center_ignored', _set(7, lambda c: None), None))
        for edge in (8192, 65536):
            if M > edge: mut.append((f'from_row_{edge}_dropped', _drop_rows_from(0, 1, 3, (2,), edge), None))
        name = f'K{K}-H{H}-M{M}-acc{acc}' + ('' if with_q else '-noq') + ('-center' if center else '') + ('-idx' if use_idx else '')
        cases.append(Case('dense_grad', name, 'dense_grad', functools.partial(_dense_grad_build, K, H, M, acc, with_q, center, use_idx),
                          plain_errs, mut))
    return cases


DENSE_GRAD = _dense_grad_cases()


@pytest.mark.gpu
@pytest.mark.parametrize('case', DENSE_GRAD, ids=repr)
def test_dense_grad(case):
    """k_dense_grad_partial (64 x 64 tiles of K x H, q from the blocks with blockIdx.y == 0) + k_reduce_partials (q == NULL: the entries
    past n1 are skipped); M = 0 zeroes P and q (accumulate = 0) or leaves them alone (accumulate = 1)."""
    run_case(case)


# ----------------------------------------------------------------------------------------------------------------------
# first_layer_param_grads (+ bn_input_grad on its m1 / m2), fold
# ----------------------------------------------------------------------------------------------------------------------
KH = [(1, 130), (64, 1), (65, 63), (130, 64), (64, 65)]        # K in {1, 64, 65, 130} x H in {1, 63, 64, 65, 130}: every value once
BN_ROWS = 300


def _bn_operands(rng, K, dev):
    return ((flat(1 + 0.3 * rng.normal(size=K), dev), flat(0.3 * rng.normal(size=K), dev)), flat(0.5 * rng.normal(size=K), dev),
            flat(rng.uniform(0.1, 2.0, K), dev))


def _flpg_build(K, H, bn_on, accumulate, centered, dev):
    rng = _rng(4, K, H, bn_on, accumulate, centered)
    tall = np.where(np.arange(H) == H - 1, 4.0, 1.0)        # the last output column weighs 16 x in S1 / S2: one lane's term shows among 130
    qn = rng.normal(size=H)
    qn = np.sign(qn) * (0.5 + np.abs(qn))                   # (H = 1: q is ONE number, and every term `centered` moves is a multiple of it)
    P, q, W = flat(rng.normal(size=(K, H)) * tall, dev), flat(qn * tall, dev), flat(0.3 * rng.normal(size=(K, H)) * tall, dev)
    bn, mean, var = _bn_operands(rng, K, dev) if bn_on else (None, None, None)
    dW, db = flat(rng.normal(size=(K, H)), dev), flat(rng.normal(size=H), dev)
    dg, dbe = (flat(rng.normal(size=K), dev), flat(rng.normal(size=K), dev)) if bn_on else (None, None)
    m1, m2 = (flat(np.full(K, 7.0), dev), flat(np.full(K, 7.0), dev)) if bn_on else (None, None)
    return (P, q, W, bn, mean, var, BN_ROWS, dW, db, dg, dbe, m1, m2, accumulate, centered), ([7, 8, 9, 10, 11, 12] if bn_on else [7, 8])


def _zero_last_col(w):
    w = w.clone()
    w[:, -1] = 0
    return w


def _flpg_cases():
    cases = []
    for K, H in KH:
        for bn_on, acc, cen in [(False, 0, False), (False, 1, False)] + [(True, a, c) for a in (0, 1) for c in (False, True)]:
            mut = [('last_col_old', None, _last_col_old), ('accumulate_taken_the_other_way', _set(13, lambda a: 1 - a), None)]
            if bn_on:
                mut += [('centered_taken_the_other_way', _set(14, lambda c: not c), None),
                        ('last_column_left_out_of_S1_S2', _set(2, _zero_last_col), None)]
            name = f'K{K}-H{H}-' + ('bn' if bn_on else 'plain') + f'-acc{acc}' + ('-centered' if cen else '')
            cases.append(Case('first_layer_param_grads', name, 'first_layer_param_grads', functools.partial(_flpg_build, K, H, bn_on, acc, cen),
                              plain_errs, mut))
    return cases


FLPG = _flpg_cases()


def _bn_input_grad_args(K, M, bn, mean, var, m1, m2, dev):
    """A column block [k0, k0 + width) with k0 > 0 (K = 1: the only column), x through a row index."""
    rng = _rng(5, K, M)
    k0 = min(2, K - 1)
    width = K - k0
    x = rng.normal(size=(M + 31, width)) + 0.5
    return (wide(rng.normal(size=(M, width)), dev), wide(x, dev), index(rng.permutation(M + 31)[:M], dev), M, k0, bn, mean, var, m1, m2,
            wide(np.full((M, width), np.nan), dev))


@pytest.mark.gpu
@pytest.mark.parametrize('case', FLPG, ids=repr)
def test_first_layer_param_grads_then_bn_input_grad(case):
    """k_first_layer_param_grads (64 lanes stride over H, S1 / S2 through a shuffle tree), then k_bn_input_grad on the m1 / m2 it wrote
    (without BatchNormalization: the plain copy dx = dy)."""
    dev = _dev()
    args, outs = case.build(dev)
    got, ref = both(case.method, *args)
    errs = case.errs([got[i] for i in outs], [ref[i] for i in outs])
    K = args[2].shape[0]
    b_args = _bn_input_grad_args(K, BN_ROWS, args[3], args[4], args[5], args[11], args[12], dev)
    got, ref = both('bn_input_grad', *b_args)
    errs['dx'] = dist(got[10], ref[10])
    for k, e in errs.items(): print(f'PRIM_ERR {case.block} {case.name} {k} {e:.3e}')
    assert all(e <= BAR for e in errs.values()), errs


def _bn_big_build(dev):
    """M * width = 8200 * 128 > 1 048 576: the grid-stride loop of k_bn_input_grad takes a second trip."""
    K, M = 130, 8200
    rng = _rng(6)
    bn, mean, var = _bn_operands(rng, K, dev)
    m1, m2 = flat(0.1 * rng.normal(size=K), dev), flat(0.1 * rng.normal(size=K), dev)
    return _bn_input_grad_args(K, M, bn, mean, var, m1, m2, dev), [10]


BN_BIG = Case('bn_input_grad', 'M8200-width128', 'bn_input_grad', _bn_big_build, plain_errs, [('from_element_1048576_unwritten', None, _tail_old)])


@pytest.mark.gpu
def test_bn_input_grad_second_trip():
    run_case(BN_BIG)


def _fold_build(K, H, mode, dev):
    rng = _rng(7, K, H, len(mode))
    W, b = flat(0.3 * rng.normal(size=(K, H)), dev), flat(rng.normal(size=H), dev)
    bn, mean, var = _bn_operands(rng, K, dev) if mode != 'plain' else (None, None, None)
    return (W, b, bn, mean, var, flat(np.full((K, H), np.nan), dev), flat(np.full(H, np.nan), dev), mode == 'centred'), [5, 6]


def _zero_last_row(w):
    w = w.clone()
    w[-1] = 0
    return w


def _fold_cases():
    cases = []
    for K, H in KH:
        for mode in ('plain', 'bn', 'centred'):
            mut = [('last_col_old', None, _last_col_old)]
            if mode != 'plain':
                mut += [('centred_taken_the_other_way', _set(7, lambda c: not c), None),
                        ('last_row_left_out_of_the_shift', _set(0, _zero_last_row), None)]
            cases.append(Case('fold', f'K{K}-H{H}-{mode}', 'fold', functools.partial(_fold_build, K, H, mode), plain_errs, mut))
    return cases


FOLD = _fold_cases()


@pytest.mark.gpu
@pytest.mark.parametrize('case', FOLD, ids=repr)
def test_fold(case):
    """k_fold_bn through gnn_fold_bn: one workgroup per output column, 128 threads stride over K."""
    run_case(case)


# ----------------------------------------------------------------------------------------------------------------------
# act_grad
# ----------------------------------------------------------------------------------------------------------------------
ACT_NAMES = ['linear', 'relu', 'selu', 'tanh', 'sigmoid', 'elu', 'softplus', 'softmax']


def _act_grad_build(act, M, H, inplace, dev):
    """Y is a real output of the activation; an out-of-place dZ starts as NaN: a row that is not written cannot pass."""
    rng = _rng(8, ACT[act], M % 1000, H, inplace)
    Y = wide(_act(ACT[act], rng.normal(size=(M, H))), dev, pad=1)
    G = wide(rng.normal(size=(M, H)), dev, pad=1)
    dZ = G if inplace else wide(np.full((M, H), np.nan), dev, pad=1)
    return (G, Y, dZ, ACT[act]), [2]


def _act_case(act, M, H, inplace, mutants=()):
    return Case('act_grad', f'{act}-M{M}-H{H}-' + ('inplace' if inplace else 'out'), 'act_grad',
                functools.partial(_act_grad_build, act, M, H, inplace), plain_errs, mutants)


ACT_GRAD = [_act_case(a, M, H, ip) for a in ACT_NAMES for H in (1, 3, 64, 65) for M in (1, 257) for ip in (False, True)]
ACT_GRAD_BIG = [_act_case('tanh', 20000, 64, False, [('from_element_1048576_unwritten', None, _tail_old)]),
                _act_case('tanh', 20000, 64, True, [('from_element_1048576_unwritten', None, _tail_old)]),
                # one row per thread: rows from 1 048 576 on (here: the last one)
                _act_case('softmax', CAP + 1, 2, False, [('from_row_1048576_unwritten', None, functools.partial(_tail_old, start=2 * CAP))])]


@pytest.mark.gpu
@pytest.mark.parametrize('case', ACT_GRAD + ACT_GRAD_BIG, ids=repr)
def test_act_grad(case):
    """k_act_grad: all eight activations from the layer OUTPUT, in place and out of place; M * H > 1 048 576 element-wise and
    M = 1 048 577 softmax rows (one row per thread behind the same capped grid)."""
    run_case(case)


def _dense_softmax_build(H, dev):
    rng = _rng(9, H)
    M, K = CAP + 1, 3
    x = wide(rng.normal(size=(M, K)), dev, pad=1)
    W, b = flat(rng.normal(size=(K, H)), dev), flat(rng.normal(size=H), dev)
    return ([(x, None)], W, H, b, ACT['softmax'], wide(np.full((M, H), np.nan), dev, pad=1)), [5]


@pytest.mark.gpu
@pytest.mark.parametrize('H', [2, 5])
def test_dense_softmax_forward_past_a_million_rows(H):
    """The forward direction of the same shape: `_Prim.dense` with a softmax activation at M = 1 048 577, on the thin-output kernel
    (H = 2: softmax finished in the same launch) and on k_segdense + k_softmax_rows (H = 5: thin_dense_applies is false)."""
    args, outs = _dense_softmax_build(H, _dev())
    x, W, b, Y = args[0][0][0], args[1], args[3], args[5]
    ref = torch.full((x.shape[0], H), float('nan'))
    _Prim(_dev()).dense(*args)
    torch.cuda.synchronize()
    NumpyPrim(None).dense([(x.cpu(), None)], W.cpu(), H, b.cpu(), ACT['softmax'], ref)
    e = dist(Y.cpu().numpy(), ref.numpy())
    print(f'PRIM_ERR dense_softmax M{x.shape[0]}-H{H} Y {e:.3e}')
    assert e <= BAR


# ----------------------------------------------------------------------------------------------------------------------
# scatter_add_rows, axpby
# ----------------------------------------------------------------------------------------------------------------------
def _scatter_build(M, width, kind, dev):
    """G is not zero beforehand.  'few': 8 distinct targets for every row; 'perm': a permutation into a larger pool; 'random': repeats."""
    rng = _rng(10, M, width, len(kind))
    pool = M + 100
    idx = {'few': lambda: rng.permutation(pool)[:8][rng.integers(0, 8, M)], 'perm': lambda: rng.permutation(pool)[:M],
           'random': lambda: rng.integers(0, pool, M)}[kind]()
    return (wide(rng.normal(size=(M, width)), dev), index(idx, dev), wide(rng.normal(size=(pool, width)), dev)), [2]


def _scatter_drop_last(args):
    args[0], args[1] = args[0][:-1], args[1][:-1]
    return args


def _scatter_drop_tail(args):
    """The elements from 1 048 576 on are not added: the whole rows in front of it, then the first columns of the row it falls in."""
    D, idx, G = args
    w = D.shape[1]
    r, c = CAP // w, CAP % w
    D = D.clone()
    D[r, c:] = 0
    args[0], args[1] = D[:r + 1], idx[:r + 1]
    return args


SCATTER = [Case('scatter_add_rows', 'M5000-w7-8targets', 'scatter_add_rows', functools.partial(_scatter_build, 5000, 7, 'few'), plain_errs,
                [('last_row_dropped', _scatter_drop_last, None)]),
           Case('scatter_add_rows', 'M300-w5-perm', 'scatter_add_rows', functools.partial(_scatter_build, 300, 5, 'perm'), plain_errs,
                [('last_row_dropped', _scatter_drop_last, None)]),
           Case('scatter_add_rows', 'M8200-w130-random', 'scatter_add_rows', functools.partial(_scatter_build, 8200, 130, 'random'), plain_errs,
                [('last_row_dropped', _scatter_drop_last, None), ('from_element_1048576_not_added', _scatter_drop_tail, None)])]


@pytest.mark.gpu
@pytest.mark.parametrize('case', SCATTER, ids=repr)
def test_scatter_add_rows(case):
    """k_scatter_add_rows: float atomics, so the order of the additions is free - the bar holds, bit equality is not claimed."""
    run_case(case)


def _axpby_build(n, alias, dev):
    rng = _rng(11, n, alias)
    x, y = flat(rng.normal(size=n), dev), flat(rng.normal(size=n), dev)
    return (0.75, x, -1.25, y, x if alias else flat(np.full(n, np.nan), dev)), [4]


AXPBY = [Case('axpby', f'n{n}-' + ('alias' if alias else 'out'), 'axpby', functools.partial(_axpby_build, n, alias), plain_errs,
              [('from_element_1048576_unwritten', None, _tail_old)] if n > CAP else [])
         for n in (1, 255, 257, CAP + 1) for alias in (False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize('case', AXPBY, ids=repr)
def test_axpby(case):
    run_case(case)


# ----------------------------------------------------------------------------------------------------------------------
# converged_gated
# ----------------------------------------------------------------------------------------------------------------------
CONV_THR = 0.01


def _converge_input(N, over_row, with_old):
    """Every row moves by half the threshold (relative to its old norm), row `over_row` (if any) by 1.5 x the threshold."""
    rng = _rng(12, N, 0 if over_row is None else over_row + 1, with_old)
    dim = 5
    old = rng.normal(size=(N, dim)) + 3.0 if with_old else np.ones((N, dim))
    step = rng.normal(size=(N, dim))
    step /= np.sqrt((step ** 2).sum(1, keepdims=True))
    scale = np.full(N, 0.5)
    if over_row is not None: scale[over_row] = 1.5
    new = old + step * (scale * CONV_THR * np.sqrt((old ** 2).sum(1)))[:, None]
    return new.astype(np.float32), old.astype(np.float32)


CONVERGE = [(N, over, old, gate) for N, over in ((1000, 617), (1000, None), (70001, 70000)) for old in (True, False) for gate in (1, 0, None)]


def test_converge_inputs_are_decided_alike_in_float32_and_float64():
    """Host: the rows of the convergence cases are far enough from the threshold that float32 and float64 arithmetic agree on each."""
    for N, over, old, _ in CONVERGE:
        new, prev = _converge_input(N, over, old)
        for dt in (np.float32, np.float64):
            s, o = new.astype(dt), prev.astype(dt)
            ratio = np.sqrt(((s - o) ** 2).sum(1, dtype=dt)) / (dt(CONV_THR) * np.sqrt((o ** 2).sum(1, dtype=dt)))
            moving = ratio > 1
            assert np.all(np.abs(ratio - 1) > 0.25)
            assert moving.sum() == (0 if over is None else 1) and (over is None or moving[over])


@pytest.mark.gpu
@pytest.mark.parametrize('N,over,with_old,gate_val', CONVERGE)
def test_converged_gated(N, over, with_old, gate_val):
    """k_converge through gnn_converged_gated (ld > dim; N > 65536: the probe over the first rows + the pass over the rest): the flag is
    raised by exactly one moving row, k is recorded, and a closed gate leaves both alone."""
    dev = _dev()
    new, prev = _converge_input(N, over, with_old)
    gate = None if gate_val is None else torch.tensor([gate_val], dtype=torch.int32, device=dev)
    flag, k_dev = torch.zeros(1, dtype=torch.int32, device=dev), torch.full((1,), -1.0, device=dev)
    got, ref = both('converged_gated', wide(new, dev), wide(prev, dev) if with_old else None, CONV_THR, gate, flag, k_dev, 3.0)
    want_flag = 0 if (gate_val == 0 or over is None) else 1
    assert int(ref[4][0]) == want_flag and float(ref[5][0]) == (-1.0 if gate_val == 0 else 3.0)
    assert int(got[4][0]) == int(ref[4][0]) and float(got[5][0]) == float(ref[5][0])


# ----------------------------------------------------------------------------------------------------------------------
# loss_grad
# ----------------------------------------------------------------------------------------------------------------------
F32_BELOW_ONE = float(np.nextafter(np.float32(1), np.float32(0)))                  # 1 - 6e-8: clipped in float32 and in float64
F32_ONE_MINUS_EPS = float(np.float32(1) - np.float32(1e-7))                        # 1 - 1.19e-7: inside the clip range in both
EDGES = [0.0, 1e-10, 1e-9, 1.0, 1 - 1e-9, F32_BELOW_ONE, F32_ONE_MINUS_EPS]


def _loss_input(kind, M, T):
    """Predictions with exact 0 and 1, values within 1e-9 of each, and the float32 neighbours of 1 - nothing between float32(1e-7) and
    float64(1e-7) or their mirror images at 1, where the two precisions clip differently by right.  BCE: a prediction the clip moves
    down from 1 gets the target 1 - its (1 - y) log(1 - p) term would be log(1 - (1 - eps)), which is log(1.19e-7) in float32 and
    log(1e-7) in float64 by the number format alone.  CCE: the edge values sit in rows of their own next to ordinary entries, so
    that p / sum(p) stays where it is put.  The edge rows start at row 1: a row whose only loss term is -log(1 - eps) holds 1.19e-7 in
    float32 and 1e-7 in float64 (1 - 1e-7 is not a float32), 2e-8 apart and 19 % of each other, so it must not be the ONLY row (M = 1)
    of a max-norm comparison.  MAE: every fifth row has p == y."""
    rng = _rng(13, kind, M, T)
    if kind == 0:
        y = np.eye(T)[rng.integers(0, T, M)]
        p = rng.uniform(0.05, 1.0, (M, T))
        for m in range(1, M, 3):
            e = EDGES[(m // 3) % len(EDGES)]
            if e < 0.5: p[m, 0] = e                             # p / sum = 0 or ~1e-10 .. 1e-8 next to ordinary entries
            else: p[m] = 0.0; p[m, (m // 3) % T] = 1.0          # p / sum = exactly 1 and exactly 0
    elif kind == 1:
        y = rng.integers(0, 2, (M, T)).astype(np.float64)
        p = rng.uniform(0.02, 0.98, (M, T))
        for m in range(1, M, 2):
            p[m, m % T] = EDGES[(m // 2) % len(EDGES)]
        y[p > 0.999] = 1.0
    else:
        y = rng.normal(size=(M, T))
        p = y + rng.normal(size=(M, T))
        if kind == 3: p[::5] = y[::5]
    sw = rng.uniform(0.5, 1.5, M)
    return y.astype(np.float32), p.astype(np.float32), sw.astype(np.float32)


LOSS = [(kind, M, T) for kind in range(4) for M in (1, 255, 256, 257, 1000) for T in (1, 2, 5) if not (kind == 0 and T < 2)]


@pytest.mark.gpu
@pytest.mark.parametrize('kind,M,T', LOSS)
def test_loss_grad(kind, M, T):
    """k_loss_grad, all four losses, with and without sample weights: the per-row loss and d loss / d prediction (zero where the clip
    is active) against `oracle/torch_train.py::keras_loss` under float64 autograd."""
    dev = _dev()
    y, p, sw = _loss_input(kind, M, T)
    for weighted in (False, True):
        got, ref = both('loss_grad', kind, flat(y, dev), flat(p, dev), flat(sw, dev) if weighted else None,
                        flat(np.full((M, T), np.nan), dev), flat(np.full(M, np.nan), dev))
        errs = {'dpred': dist(got[4], ref[4]), 'loss_rows': dist(got[5], ref[5])}
        for k, e in errs.items(): print(f'PRIM_ERR loss_grad kind{kind}-M{M}-T{T}-sw{int(weighted)} {k} {e:.3e}')
        assert all(e <= BAR for e in errs.values()), (weighted, errs)


def test_numpy_reference_losses_match_their_formulas():
    """Host: the BCE / MAE additions of NumpyPrim.loss_grad against the formulas written out, clip edges included."""
    for kind in (1, 3):
        y, p, sw = _loss_input(kind, 257, 5)
        dp, rows = torch.zeros(257, 5), torch.zeros(257)
        NumpyPrim(None).loss_grad(kind, torch.from_numpy(y), torch.from_numpy(p), torch.from_numpy(sw), dp, rows)
        y64, p64, w = y.astype(np.float64), p.astype(np.float64), sw.astype(np.float64)
        if kind == 1:
            pc = np.clip(p64, 1e-7, 1 - 1e-7)
            inside = (p64 >= 1e-7) & (p64 <= 1 - 1e-7)
            want_rows = -(y64 * np.log(pc) + (1 - y64) * np.log(1 - pc)).mean(1) * w
            want_dp = np.where(inside, -(y64 / pc) + (1 - y64) / (1 - pc), 0.0) * w[:, None] / 5 / 257
            assert (~inside).sum() > 20
        else:
            want_rows = np.abs(p64 - y64).mean(1) * w
            want_dp = np.sign(p64 - y64) * w[:, None] / 5 / 257
            assert (p64 == y64).sum() > 100
        assert rel_err(rows.numpy(), want_rows) <= 1e-6 and rel_err(dp.numpy(), want_dp) <= 1e-6


# ----------------------------------------------------------------------------------------------------------------------
# optimizers
# ----------------------------------------------------------------------------------------------------------------------
OPT_SIZES = [0, 1, 255, 256, 257, 4097, 262145 + 3]          # the last one: 1025 workgroups of 256 > gnn_adam_multi's 1024 per variable


def _grad(rng, n):
    """|g| >= 1e-3: Adam's m / (sqrt(v) + eps) is a sign function near zero - a tiny gradient says nothing about the kernel."""
    g = rng.normal(size=n)
    return (np.sign(g) * (1e-3 + np.abs(g))).astype(np.float32)


@pytest.mark.gpu
def test_adam_multi_and_adam_step_against_float64():
    """gnn_adam_multi on 40 variables (two launches of at most 32; sizes 0 .. 262 148: the 1024-workgroup cap per variable), three steps
    with fresh gradients: parameters, m and v against float64 `torch_train.adam_update`, and bit-equal to gnn_adam_step per variable."""
    dev, lib = _dev(), nat.lib()
    st = nat.current_stream(dev)
    rng = _rng(14)
    sizes = [OPT_SIZES[i % len(OPT_SIZES)] for i in range(40)]
    p0 = [rng.normal(size=n).astype(np.float32) for n in sizes]
    # the ABI takes the hyper-parameters as float: the reference gets the SAME numbers (float32(0.999) is 0.99900001..., and 1 - beta_2
    # is then 1.29e-5 off 0.001 - with the double 0.999 on the reference's side alone, v measured 1.295e-5 here for that reason only)
    lr, b1, b2, eps = (float(np.float32(h)) for h in (0.01, 0.9, 0.999, 1e-7))
    multi = [[flat(a, dev) for a in p0], None, [flat(np.zeros(n), dev) for n in sizes], [flat(np.zeros(n), dev) for n in sizes]]
    single = [[flat(a, dev) for a in p0], None, [flat(np.zeros(n), dev) for n in sizes], [flat(np.zeros(n), dev) for n in sizes]]
    ref = [[a.astype(np.float64) for a in p0], None, [np.zeros(n) for n in sizes], [np.zeros(n) for n in sizes]]
    n_vars = len(sizes)
    arr = lambda ts: (C.c_void_p * n_vars)(*[t.data_ptr() for t in ts])
    for step in (1, 2, 3):
        grads = [_grad(rng, n) for n in sizes]
        g_dev = [flat(g, dev) for g in grads]
        nat.check(lib.gnn_adam_multi(arr(multi[0]), arr(g_dev), arr(multi[2]), arr(multi[3]), (C.c_size_t * n_vars)(*sizes), n_vars,
                                     lr, b1, b2, eps, step, None, st))
        for j, n in enumerate(sizes):
            nat.check(lib.gnn_adam_step(nat.ptr(single[0][j]), nat.ptr(g_dev[j]), nat.ptr(single[2][j]), nat.ptr(single[3][j]), n,
                                        lr, b1, b2, eps, step, None, st))
            ref[0][j], ref[2][j], ref[3][j] = torch_train.adam_update(ref[0][j], grads[j].astype(np.float64), ref[2][j], ref[3][j], step,
                                                                      lr, b1, b2, eps)
        torch.cuda.synchronize()
    worst = {}
    for slot, name in ((0, 'p'), (2, 'm'), (3, 'v')):
        for j, n in enumerate(sizes):
            a, b = multi[slot][j].cpu().numpy(), single[slot][j].cpu().numpy()
            assert np.array_equal(a, b), (name, j, n)
            worst[name] = max(worst.get(name, 0.0), dist(a, ref[slot][j]))
    for k, e in worst.items(): print(f'PRIM_ERR adam 40vars-3steps {k} {e:.3e}')
    assert all(e <= BAR for e in worst.values()), worst


@pytest.mark.gpu
@pytest.mark.parametrize('momentum', [0.0, 0.9])
def test_sgd_step_against_float64(momentum):
    """gnn_sgd_step (momentum 0: no velocity array), three steps, against the same recurrence in float64; 1 048 577 elements: the
    grid-stride loop behind the capped grid takes a second trip."""
    dev, lib = _dev(), nat.lib()
    st = nat.current_stream(dev)
    rng = _rng(15, int(momentum * 10))
    lr, worst = 0.05, {}
    for n in (1, 255, 257, CAP + 1):
        p0 = rng.normal(size=n).astype(np.float32)
        p, vel = flat(p0, dev), (flat(np.zeros(n), dev) if momentum else None)
        rp, rv = p0.astype(np.float64), np.zeros(n)
        for _ in range(3):
            g = _grad(rng, n)
            g_dev = flat(g, dev)
            nat.check(lib.gnn_sgd_step(nat.ptr(p), nat.ptr(g_dev), nat.ptr(vel), n, lr, momentum, None, st))
            torch.cuda.synchronize()
            if momentum:
                rv = momentum * rv - lr * g.astype(np.float64)
                rp = rp + rv
            else:
                rp = rp - lr * g.astype(np.float64)
        worst['p'] = max(worst.get('p', 0.0), dist(p.cpu().numpy(), rp))
        if momentum: worst['velocity'] = max(worst.get('velocity', 0.0), dist(vel.cpu().numpy(), rv))
    for k, e in worst.items(): print(f'PRIM_ERR sgd momentum{momentum} {k} {e:.3e}')
    assert all(e <= BAR for e in worst.values()), worst


# ----------------------------------------------------------------------------------------------------------------------
# teeth (host only)
# ----------------------------------------------------------------------------------------------------------------------
TEETH_CASES = COLSTATS + DENSE_GRAD + FLPG + FOLD + [BN_BIG] + ACT_GRAD_BIG + SCATTER + [c for c in AXPBY if c.mutants]


@pytest.mark.parametrize('case', TEETH_CASES, ids=repr)
def test_teeth(case):
    """Every reduction case (and every case whose point is a second grid-stride trip) tells a wrong kernel from a right one: each
    mutant derived from the float64 reference misses the bar by a factor of 100 under the case's own measure.  No case is exempt:
    one without an applicable mutant fails here."""
    ref, old = reference(case)
    assert case.mutants
    applied = 0
    for name, pre, post in case.mutants:
        if pre is not None:
            args, outs = case.build('cpu')
            args = pre(list(args))
            if args is None: continue
            getattr(NumpyPrim(None), case.method)(*args)
            mutant = outputs(args, outs)
        else:
            mutant = [r.copy() for r in ref]
        if post is not None: mutant = post(mutant, old)
        worst = max(case.errs(mutant, ref).values())
        assert worst >= TEETH * BAR, (name, worst)
        applied += 1
    assert applied > 0
