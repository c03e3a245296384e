"""Seeded training fuzz on EVERY route of `gnn_train_step`, homogeneous and composite, against the float64 autograd oracle.

tests/test_gpu_fuzz.py::test_fuzz_training_gradients runs each seed on whatever route the plan picks.  Here every seed names the routes
that cover it - a route is (name, how to force it, the exact `gnn_last_kernel_name()` it must produce) - and runs ALL of them against ONE
oracle result, at the project's own bars (k exact, loss 1e-5, `Y_PRED_BAR`, `BARS` with the kink allowance of `grad_rows`, moving
statistics 1e-5: `check_step` of tests/test_gpu_training.py, `composite_compare` of tests/test_gpu_round6.py).  The eligibility rule is
restated in Python (`homogeneous_plan`, `composite_plan`) from csrc/train_loop.hpp (`homogeneous_train_path`) and
csrc/train_composite.hpp / train_composite_big.hpp (`composite_train_path`, `composite_big_applies`); a wrong restatement cannot hide,
because every run asserts the kernel name.

Three parts: 1. the configuration generator (`homogeneous_case`, `composite_case`: pure functions of the seed) and `test_route_census`,
which needs no GPU and asserts that the committed seed ranges reach every route and every corner listed there; 2.
`test_fuzz_homogeneous_routes`; 3. `test_fuzz_composite_routes`.

The draws are stratified, not uniform (j = seed // 4; HOM_SEEDS = 48):
  seed % 4 == 0  one Dense of a state width the row-streaming kernels have (16 / 32 / 64; `ROW_WIDTHS`: d = 0 with 16 / 32 label columns
                 reaches Kc = 0 and the arc-labels-only constants line, d = 32 with L = 14, A = 4 reaches Kc = 32), activation j % 7,
                 loss j % 4
  seed % 4 == 1  Dense(H) - Dense(S): H <= the padded width (three seeds of four), or wider than that (general kernels only)
  seed % 4 == 2  one Dense of any width: d in {3, 8, 16, 24, 32, 40, 64} or d = 0
  seed % 4 == 3  Dropout / AlphaDropout behind the Dense layers of the state network, one layer (j even) or Dense(H) - Dense(S) (j odd)
  every family   focus j % 3 x batch size class (j // 3) % 4: under 16 rows in all, 16 .. 63, over 128, free
With L in 1 .. 14 and A in 0 .. 4 a network with a state reads 2 L + A <= 32 constant columns: Kc > 32 is out of reach of these ranges.
A one-column target takes no softmax head (softmax of one column is the constant 1: every gradient is exactly zero).

Threshold: 0 in four seeds of five; there the case is accepted when the float32 and the float64 oracle stop at the same k (threshold 0
stops at an exact fixed point only).  A positive threshold (seed % 5 == 2) is accepted when the float64 oracle's k is at least 1 and
does not change with the threshold moved by 1e-3 (relative) either way - no executed evaluation's worst ratio lies within 1e-3 of it,
the rule of tests/test_gpu_train_dropout_small.py.  Otherwise the case takes its next sub-seed.  Decided once, on the CPU.

Census of the committed seed ranges (`python -m pytest tests/test_gpu_train_route_fuzz.py -m "not gpu" -s` prints it):

homogeneous, seeds 0 .. 47
route                                 seeds     selu     tanh     relu  sigmoid   linear      elu softplus      cce      mse      bce      mae        n        a        g
default                                  48        6        8        6        7        8        4        9        7       12       17       12       16       16       16
dropout form                              6        1        2        1        0        0        0        2        0        1        3        2        2        2        2
general                                  48        6        8        6        7        8        4        9        7       12       17       12       16       16       16
hidden-layer dropout form                 6        1        0        3        0        0        1        1        1        0        1        4        2        2        2
hidden-layer form                         9        0        4        0        2        1        0        2        1        4        3        1        3        3        3
persistent, tiled                        24        4        2        2        4        6        2        4        5        6        8        5        8        8        8
persistent, untiled                      24        4        2        2        4        6        2        4        5        6        8        5        8        8        8
row-streaming                            14        2        2        2        2        3        2        1        3        4        4        3        5        4        5
composite, seeds 0 .. 23 (an activation counts once per seed that has it on a type with nodes)
route                                 seeds     selu     tanh     relu  sigmoid   linear      elu softplus      cce      mse      bce      mae        n        a        g
default -> general                       10        4        2        3        4        3        5        3        3        3        2        2        7        2        1
default -> persistent small-graph        14        8        3        7        4        4        5        2        2        4        4        4        1        6        7
general -> general                       24       12        5       10        8        7       10        5        5        7        6        6        8        8        8
type ranges -> general                   12        5        2        4        4        2        5        3        2        2        4        4        4        4        4
type ranges -> row-streaming             12        7        3        6        4        5        5        2        3        5        2        2        4        4        4
"""
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

from gnnkeras_amd import _native as nat
from gnnkeras_amd import GraphObject, CompositeGraphObject
from gnnkeras_amd.Models.MLP import MLP, get_inout_dims
from gnnkeras_amd.Models.GNN import GNNnodeBased, GNNarcBased, GNNgraphBased
from gnnkeras_amd.Models.CompositeGNN import CompositeGNNnodeBased, CompositeGNNarcBased, CompositeGNNgraphBased
from gnnkeras_amd.Models.training import LoopTrainer, SGD
from gnnkeras_amd.Sequencers.GraphSequencers import MultiGraphSequencer, CompositeMultiGraphSequencer
import test_gpu_training as tt
from test_gpu_training import cached_oracle, check_step, oracle_step
from test_gpu_fuzz import ACTS, random_arcs
from test_gpu_round6 import composite_compare, composite_oracle_step, composite_weights, set_composite_weights

FUZZ_SCALE = int(os.environ.get('GNN_FUZZ_SCALE', '1'))      # GNN_FUZZ_SCALE=10 runs ten times as many seeds (offline soak)
HOM_SEEDS, COMP_SEEDS = 48, 24
FOCI = ['n', 'a', 'g']
LOSSES = [('categorical_crossentropy', 'softmax'), ('mse', 'linear'), ('binary_crossentropy', 'sigmoid'), ('mae', 'tanh')]
KNOBS = ('GNN_TRAIN_SMALL', 'GNN_TRAIN_BIG_MIN_NODES', 'GNN_TRAIN_COMPOSITE_BIG', 'GNN_TRAIN_TAPE_MB')
HID, DROP = nat.FLAG_TRAIN_HIDDEN_SMALL, nat.FLAG_TRAIN_DROPOUT_SMALL

GENERAL = 'train_step: general kernels'
SMALL = 'train_step: persistent small-graph kernels'
HIDDEN = SMALL + ' (hidden layer)'
DROPPED = SMALL + ' (dropout)'
HIDDEN_DROPPED = SMALL + ' (hidden layer, dropout)'
BIG = 'train_step: row-streaming kernels (kernels_train_big.hpp)'
C_GENERAL = 'train_step composite: general kernels (one launch per layer, type and iteration)'
C_SMALL = 'train_step composite: persistent small-graph kernels'
C_BIG = 'train_step composite: row-streaming kernels on type ranges'

# name; env for monkeypatch.setenv; LoopTrainer.use_tiles (None: as it is); native_flags; the kernel name; composite row-streaming: XT
Route = namedtuple('Route', 'name env use_tiles flags expected xt', defaults=(None,))


def route_matches(route, name):
    if route.xt is None: return name == route.expected
    return name.startswith(route.expected) and f'XT={route.xt}>' in name


def padded(S):
    return 16 if S <= 16 else 32 if S <= 32 else 64


# ---- 1a. the rule, restated ------------------------------------------------------------------------------------------------------------------
def homogeneous_plan(c, flags=0, small_on=True, big_min=32768):
    """`homogeneous_train_path` (csrc/train_loop.hpp) at these sizes: every tile is resident and every tape within its budget."""
    S, SPs, Kc, K, N, units = c['S'], padded(c['S']), c['Kc'], c['K'], c['N'], c['units']
    pos = c['drop']['pos'] if c['drop'] else []
    one = len(units) == 1 and units[0] == S                                              # one_dense_of_state_width (no softmax state here)
    hid_ok = SPs <= 32 and len(units) == 2 and units[1] == S and 1 <= units[0] <= SPs    # hidden_dense_of_state_width
    small_fits = small_on and N < big_min and S <= 64                                    # train_small_fits
    if pos and flags & DROP and K >= 1 and Kc <= 32:
        hid = bool(flags & HID) and hid_ok
        form = SPs <= 32 and 1 <= len(pos) <= len(units) and all(1 <= q <= len(units) for q in pos) and \
            all(a < b for a, b in zip(pos, pos[1:]))                                     # dropout_small_form
        if (hid or one) and form and small_fits: return HIDDEN_DROPPED if hid else DROPPED
    if flags & HID and hid_ok and not pos and K >= 1 and Kc <= 32 and small_fits: return HIDDEN
    if not one or pos or K <= 0 or Kc > 32: return GENERAL
    if N >= big_min: return BIG if S in (16, 32, 64) else GENERAL
    return SMALL if small_fits else GENERAL


def composite_plan(c, small_on=True, big_min=32768):
    """`composite_train_path` / `composite_big_applies`: (the kernel name, XT of the row-streaming kernels or None)."""
    S, N = c['D'], c['N']
    bns = {bool(b) for b, n in zip(c['bn'], c['counts']) if n > 0}                       # every non-empty type with or every one without
    n_wg = sum(-(-n // 64) for n in c['counts'])
    if len(bns) == 1 and small_on and N < big_min and S <= 64 and 1 <= n_wg <= 256: return C_SMALL, None
    kc = [d_t + sum(c['dims']) + c['A'] for d_t in c['dims']]                            # (every type, the empty ones too)
    if N >= big_min and S in (32, 64) and max(kc) <= 63: return C_BIG, 2 if max(kc) > 31 else 1
    return C_GENERAL, None


def homogeneous_routes(c):
    small_off, big0 = {'GNN_TRAIN_SMALL': '0'}, {'GNN_TRAIN_BIG_MIN_NODES': '0'}
    routes = [Route('default', {}, None, 0, homogeneous_plan(c)), Route('general', small_off, None, 0, homogeneous_plan(c, small_on=False))]
    if homogeneous_plan(c) == SMALL:           # (every graph has at most 60 nodes: the batch is handed over in tiles when use_tiles says so)
        routes += [Route('persistent, tiled', {}, True, 0, SMALL), Route('persistent, untiled', {}, False, 0, SMALL)]
    tiles = c['seed'] % 2 == 0                 # the flagged forms: tiles cut at graph boundaries (even seeds), 64 consecutive nodes (odd)
    if homogeneous_plan(c, HID) == HIDDEN: routes.append(Route('hidden-layer form', {}, tiles, HID, HIDDEN))
    flags = DROP | (HID if len(c['units']) == 2 else 0)
    name = homogeneous_plan(c, flags)
    if name == DROPPED: routes.append(Route('dropout form', {}, tiles, flags, DROPPED))
    if name == HIDDEN_DROPPED: routes.append(Route('hidden-layer dropout form', {}, tiles, flags, HIDDEN_DROPPED))
    if homogeneous_plan(c, big_min=0) == BIG: routes.append(Route('row-streaming', big0, None, 0, BIG))
    return routes


def composite_routes(c):
    (default, _), (off, _), (ranges, xt) = composite_plan(c), composite_plan(c, small_on=False), composite_plan(c, big_min=0)
    return [Route('default', {}, None, 0, default), Route('general', {'GNN_TRAIN_SMALL': '0'}, None, 0, off),
            Route('type ranges', {'GNN_TRAIN_BIG_MIN_NODES': '0'}, None, 0, ranges, xt)]


# ---- 1b. the draws ---------------------------------------------------------------------------------------------------------------------------
# (d, L, A) of the seeds that are cut for the row-streaming kernels; None: drawn (L in 1 .. 14, A in 0 .. 4)
ROW_WIDTHS = [(0, 16, 0), (32, 14, 4), (64, None, None), (0, 32, 2), (16, None, None), (0, 16, 2), (64, None, None), (32, None, None),
              (16, None, None), (0, 32, 0), (64, None, None), (16, None, None)]
SIZE_CLASSES = ['tiny', 'mid', 'large', 'free']


def batch_sizes(rng, cls):
    """2 - 5 graphs of 3 - 60 nodes whose total lands under 16 rows ('tiny': less than one 16-row tile), in 16 .. 63 ('mid': less than one
    64-row step), over 128 ('large': several tiles) or anywhere ('free')."""
    while True:
        if cls == 'tiny': sizes = rng.integers(3, 7, int(rng.integers(2, 4)))
        elif cls == 'mid': sizes = rng.integers(3, 30, int(rng.integers(2, 5)))
        elif cls == 'large': sizes = rng.integers(20, 61, int(rng.integers(3, 6)))
        else: sizes = rng.integers(3, 61, int(rng.integers(2, 6)))
        tot = int(sizes.sum())
        if {'tiny': tot < 16, 'mid': 16 <= tot <= 63, 'large': tot > 128, 'free': True}[cls]: return [int(v) for v in sizes]


def threshold_of(seed, rng):
    return float(rng.choice([0.05, 0.15, 0.4])) if seed % 5 == 2 else 0.0


def draw_homogeneous(seed, rng):
    fam, j = seed % 4, seed // 4
    c = dict(seed=seed, focus=FOCI[j % 3], size_class=SIZE_CLASSES[(j // 3) % 4], drop=None)
    d = L = A = None
    if fam == 0:
        d, L, A = ROW_WIDTHS[j % len(ROW_WIDTHS)]
        act, (loss, out_act) = ACTS[j % 7], LOSSES[j % 4]
    else:
        narrow = fam == 3 or (fam == 1 and j % 4 != 3)                    # the forms of the persistent kernels with a second set of accumulators
        if fam != 2 and rng.random() < 0.2: d, L, A = 0, int(rng.choice([16, 32])), int(rng.choice([0, 2]))
        elif narrow: d = int(rng.choice([3, 8, 16, 24, 32]))
        else: d = int(rng.choice([3, 8, 16, 24, 32, 40, 64], p=[.2, .2, .05, .2, .05, .2, .1]))      # (family 0 has the widths 16 / 32 / 64)
        act, (loss, out_act) = ACTS[int(rng.integers(0, 7))], LOSSES[int(rng.integers(0, 4))]
    if L is None: L, A = int(rng.integers(1, 15)), int(rng.integers(0, 5))
    T = int(rng.integers(1, 5))
    if T == 1 and out_act == 'softmax': loss, out_act = LOSSES[1 + j % 3]
    S = d if d else L
    units = [S]
    if fam == 1 and j % 4 == 3: units = [padded(S) + int(rng.integers(1, 20)), S]
    elif fam == 1 or (fam == 3 and j % 2 == 1): units = [int(rng.choice([1, 5, padded(S) // 2, padded(S) - 1, padded(S)])), S]
    if fam == 3:
        pos = [1] if len(units) == 1 else [[1], [2], [1, 2]][int(rng.integers(0, 3))]
        alpha = rng.random() < 0.34
        c['drop'] = dict(rate=float(rng.choice([0.1, 0.2, 0.3])), pos=pos, alpha=alpha, seed=5 + seed)
        if alpha: act = 'selu'
    thr = threshold_of(seed, rng)
    c.update(d=d, L=L, A=A, T=T, S=S, Kc=(2 * L if d else 0) + A, units=units, act=act, loss=loss, out_act=out_act,
             mode=['sum', 'average', 'normalized'][int(rng.integers(0, 3))], bn=bool(rng.integers(0, 2)), avg=bool(rng.integers(0, 2)),
             K=6 if thr > 0 else int(rng.integers(1, 7)), thr=thr, out_hidden=[6] if rng.random() < 0.4 else None,
             sizes=batch_sizes(rng, c['size_class']))
    c['N'] = sum(c['sizes'])
    return c


def build_homogeneous(c, rng):
    focus, L, A, T, d, mode = c['focus'], c['L'], c['A'], c['T'], c['d'], c['mode']
    graphs = []
    for n in c['sizes']:
        arcs = random_arcs(rng, n, int(rng.integers(2, 3 * n)), A)
        cnt = {'n': n, 'a': len(arcs), 'g': n}[focus]
        om = rng.random(cnt) < 0.7 if focus != 'g' else np.ones(n, bool)      # masks as in tests/test_gpu_fuzz.py
        om[0] = True
        sm = rng.random(cnt) < 0.8 if focus != 'g' else np.ones(n, bool)
        sm[0] = True
        nt = int(om.sum()) if focus != 'g' else 1
        t = rng.random((nt, T)); t = t / t.sum(1, keepdims=True)
        graphs.append(GraphObject(rng.normal(size=(n, L)), arcs, t, focus=focus, set_mask=sm, output_mask=om,
                                  sample_weight=rng.uniform(0.5, 1.5, nt), aggregation_mode=mode))
    x, y, sw = MultiGraphSequencer(graphs, focus, mode, len(graphs), shuffle=False)[0]
    inp, lay = get_inout_dims('state', L, A, T, focus, d, hidden_units=c['units'][:-1] or None)
    assert lay == c['units']
    ns = MLP(inp[0], lay, c['act'], 'lecun_normal', 'lecun_normal', rng=c['seed'], batch_normalization=c['bn'])
    ns.set_weights([w * 0.3 if w.ndim == 2 else w for w in ns.get_weights()])
    if c['drop']:       # as `drop_nets` of tests/test_gpu_train_dropout_small.py
        ns.dropout_rate, ns.dropout_pos, ns.alphadropout = [c['drop']['rate']] * len(c['drop']['pos']), list(c['drop']['pos']), c['drop']['alpha']
    inp, lay = get_inout_dims('output', L, A, T, focus, d, hidden_units=c['out_hidden'])
    no = MLP(inp[0], lay, ['tanh'] * (len(lay) - 1) + [c['out_act']], 'glorot_normal', 'glorot_normal', rng=c['seed'] + 1,
             batch_normalization=c['bn'])
    for n_ in (ns, no):
        if c['bn']:
            w = n_.get_weights()
            w[0] = rng.uniform(.7, 1.3, w[0].shape).astype(np.float32); w[1] = rng.normal(0, .2, w[1].shape).astype(np.float32)
            n_.set_weights(w)
    model = {'n': GNNnodeBased, 'a': GNNarcBased, 'g': GNNgraphBased}[focus](ns, no, d, c['K'], c['thr'])
    assert x[0].shape[0] == c['N']
    s0 = rng.normal(0, 0.2, (c['N'], d)).astype(np.float32) if d else None
    return dict(model=model, x=x, y=y, sw=sw, s0=s0, seed=c['drop']['seed'] if c['drop'] else None)


def stable_k(c, model, oracle):
    """Whether float32 cannot flip the loop's k (`oracle(dtype)`: the oracle's result with the model as it stands): see the module docstring."""
    k = oracle(torch.float64)['k']
    if c['thr'] == 0.0: return oracle(torch.float32)['k'] == k
    ks = []
    for f in (1 - 1e-3, 1 + 1e-3):
        model.state_threshold = c['thr'] * f
        ks.append(oracle(torch.float64)['k'])
    model.state_threshold = c['thr']
    return k >= 1 and ks[0] == k == ks[1]


def draw_composite(seed, rng):
    Tt, D = 2 + (seed // 3) % 3, [32, 4, 64, 16][(seed // 2) % 4]
    A = int(rng.integers(0, 4))
    while True:          # kc = d_t + (sum of the widths + A): at most 31 on even seeds (XT = 1), 32 .. 63 on odd ones (XT = 2)
        dims = [int(v) for v in (rng.integers(5, 15, Tt) if seed % 2 else rng.integers(0, 9, Tt))]
        if seed % 4 == 2: dims[int(rng.integers(0, Tt))] = 0          # a type without labels of its own
        kc = max(dims) + sum(dims) + A
        if max(dims) >= 1 and (32 <= kc <= 63 if seed % 2 else kc <= 31): break
    T = int(rng.integers(1, 5))
    loss, out_act = LOSSES[(seed // 3) % 4]
    if T == 1 and out_act == 'softmax': loss, out_act = LOSSES[1 + seed % 3]
    bn = [[True] * Tt, [False] * Tt, [bool(t % 2) for t in range(Tt)]][int(rng.choice(3, p=[0.4, 0.3, 0.3]))]
    thr = threshold_of(seed, rng)
    c = dict(seed=seed, focus=FOCI[seed % 3], D=D, dims=dims, A=A, T=T, loss=loss, out_act=out_act, bn=bn, out_bn=bool(rng.integers(0, 2)),
             acts=[ACTS[int(rng.integers(0, 7))] for _ in range(Tt)], avg=bool(rng.integers(0, 2)), thr=thr,
             K=6 if thr > 0 else int(rng.integers(1, 6)), mode=['sum', 'average', 'normalized', 'composite_average'][int(rng.integers(0, 4))],
             empty=int(rng.integers(0, Tt)) if seed % 6 == 4 else None, drop=None)
    # 1 - 4 graphs; graph focus: at least two.  One graph pooled by its mean behind a BatchNormalization + linear head has a CONSTANT prediction
    # (the normalised columns have mean zero over the graph's rows): every gradient in front of the head is exactly zero - nothing to compare
    n_graphs = max(int(rng.integers(1, 5)), 2 if c['focus'] == 'g' else 1)
    c['sizes'] = [int(rng.integers(Tt + 1, 13)) if rng.random() < 0.5 else int(rng.integers(13, 81)) for _ in range(n_graphs)]
    c['types'] = []
    for n in c['sizes']:
        types = rng.integers(0, Tt, n); types[:Tt] = np.arange(Tt)
        if c['empty'] is not None: types[types == c['empty']] = (c['empty'] + 1) % Tt
        c['types'].append(types)
    c['N'] = sum(c['sizes'])
    c['counts'] = [int(sum(int((t_ == t).sum()) for t_ in c['types'])) for t in range(Tt)]
    return c


def build_composite(c, rng):
    focus, dims, A, T, D, mode, Tt = c['focus'], c['dims'], c['A'], c['T'], c['D'], c['mode'], len(c['dims'])
    graphs = []
    for n, types in zip(c['sizes'], c['types']):
        arcs = random_arcs(rng, n, int(rng.integers(1, 4 * n)), A)
        tm = np.zeros((n, Tt), bool); tm[np.arange(n), types] = True
        cnt = {'n': n, 'a': len(arcs), 'g': n}[focus]
        om = rng.random(cnt) < 0.7 if focus != 'g' else np.ones(n, bool)
        om[0] = True
        nt = int(om.sum()) if focus != 'g' else 1
        t = rng.random((nt, T)); t = t / t.sum(1, keepdims=True)
        graphs.append(CompositeGraphObject(rng.normal(size=(n, max(dims))), arcs, t, type_mask=tm, dim_node_label=tuple(dims), focus=focus,
                                           output_mask=om, sample_weight=rng.uniform(0.5, 1.5, nt), aggregation_mode=mode))
    x, y, sw = CompositeMultiGraphSequencer(graphs, focus, mode, len(graphs), shuffle=False)[0]
    inp, lay = get_inout_dims('state', tuple(dims), A, T, focus, D)
    ns = [MLP(i, lay, c['acts'][t], 'lecun_normal', 'lecun_normal', rng=c['seed'] + t, batch_normalization=c['bn'][t]) for t, i in enumerate(inp)]
    for n_ in ns: n_.set_weights([w * 0.4 if w.ndim == 2 else w for w in n_.get_weights()])
    inp, lay = get_inout_dims('output', tuple(dims), A, T, focus, D)
    no = MLP(inp[0], lay, c['out_act'], 'glorot_normal', 'glorot_normal', rng=c['seed'] + 50, batch_normalization=c['out_bn'])
    for n_ in ns + [no]:
        if n_.batch_normalization:
            w = n_.get_weights()
            w[0] = rng.uniform(.7, 1.3, w[0].shape).astype(np.float32); w[1] = rng.normal(0, .2, w[1].shape).astype(np.float32)
            n_.set_weights(w)
    model = {'n': CompositeGNNnodeBased, 'a': CompositeGNNarcBased, 'g': CompositeGNNgraphBased}[focus](ns, no, D, c['K'], c['thr'])
    assert x[0].shape[0] == c['N']
    return dict(model=model, x=x, y=y, sw=sw, s0=rng.normal(0, 0.2, (c['N'], D)).astype(np.float32))


def _case(kind, seed):
    """The first sub-seed of `seed` whose k float32 cannot flip: (configuration, what was built from it, the oracle key)."""
    draw, build = (draw_homogeneous, build_homogeneous) if kind == 'homogeneous' else (draw_composite, build_composite)
    for sub in range(8):
        rng = np.random.default_rng([77000 if kind == 'homogeneous' else 88000, seed, sub])
        c = draw(seed, rng)
        b = build(c, rng)
        c['sub'], b['key'] = sub, ('train_route_fuzz', kind, seed, sub)
        m = b['model']
        if kind == 'homogeneous':
            oracle = lambda dt: oracle_step(m, b['x'], b['y'], b['sw'], b['s0'], c['loss'], c['avg'], dtype=dt, seed=b['seed'])
        else:       # (the composite oracle is float64 only: threshold 0 is taken as it is, as in tests/test_gpu_fuzz.py::test_fuzz_composite)
            oracle = lambda dt: composite_oracle_step(m, b['x'], b['y'], b['sw'], b['s0'], loss=c['loss'], avg=c['avg'])
        if (kind == 'composite' and c['thr'] == 0.0) or stable_k(c, m, oracle):
            cached_oracle(b['key'], lambda: oracle(torch.float64))
            return c, b
    raise AssertionError(f'{kind} seed {seed}: no sub-seed with a stable k')


# (built afresh by whoever asks: nothing of a case - its model, its batch on the device - outlives the test that ran it; only the oracle's
# result, host arrays, stays with `cached_oracle`)
def _homogeneous(seed):
    c, b = _case('homogeneous', seed)
    return c, homogeneous_routes(c), b


def _composite(seed):
    c, b = _case('composite', seed)
    return c, composite_routes(c), b


def homogeneous_case(seed):
    """(configuration, routes that cover it) - a pure function of the seed."""
    return _homogeneous(seed)[:2]


def composite_case(seed):
    return _composite(seed)[:2]


# ---- 1c. the census --------------------------------------------------------------------------------------------------------------------------
FLOOR = 6
LOSS_SHORT = {'categorical_crossentropy': 'cce', 'mse': 'mse', 'binary_crossentropy': 'bce', 'mae': 'mae'}


def census(cases, composite):
    """{route, as it is named by what it forces and what runs: {column: seeds}} and the table of it."""
    cols = ACTS + list(LOSS_SHORT.values()) + FOCI
    table = {}
    for c, routes in cases:
        acts = {a for a, n in zip(c['acts'], c['counts']) if n > 0} if composite else {c['act']}
        for r in routes:
            key = r.name if not composite else f"{r.name} -> {r.expected.split(': ')[1].split(' kernels')[0]}"
            row = table.setdefault(key, dict.fromkeys(['seeds'] + cols, 0))
            row['seeds'] += 1
            for col in list(acts) + [LOSS_SHORT[c['loss']], c['focus']]: row[col] += 1
    head = f"{'route':<34}" + ''.join(f'{h:>9}' for h in ['seeds'] + cols)
    lines = [head] + [f'{k:<34}' + ''.join(f'{row[h]:>9}' for h in ['seeds'] + cols) for k, row in sorted(table.items())]
    return table, '\n'.join(lines)


def test_route_census():
    """The committed seed ranges reach every route often enough, and the row-streaming routes every corner the hand-picked tests leave out."""
    hom = [homogeneous_case(s) for s in range(HOM_SEEDS)]
    comp = [composite_case(s) for s in range(COMP_SEEDS)]
    t_hom, text_hom = census(hom, False)
    t_comp, text_comp = census(comp, True)
    print(f'\nhomogeneous, seeds 0 .. {HOM_SEEDS - 1}\n{text_hom}\ncomposite, seeds 0 .. {COMP_SEEDS - 1} (an activation counts once per seed that has it on a type with nodes)\n{text_comp}')
    for name in ('default', 'general', 'persistent, tiled', 'persistent, untiled', 'hidden-layer form', 'dropout form', 'hidden-layer dropout form',
                 'row-streaming'):
        assert t_hom.get(name, {'seeds': 0})['seeds'] >= FLOOR, (name, t_hom.get(name))
    for c, routes in hom:
        by_name = {r.name: r for r in routes}
        assert by_name['general'].expected == GENERAL                 # GNN_TRAIN_SMALL=0 leaves nothing else below the large-graph threshold
        assert all(n <= 60 for n in c['sizes']) and 2 <= len(c['sizes']) <= 5
    totals = {cls: [c['N'] for c, _ in hom if c['size_class'] == cls] for cls in SIZE_CLASSES}
    assert max(totals['tiny']) < 16 and 16 <= min(totals['mid']) and max(totals['mid']) <= 63 and min(totals['large']) > 128
    for want in (GENERAL, SMALL):              # what the default route predicts
        assert sum(1 for c, routes in hom if routes[0].expected == want) >= FLOOR, want
    assert sum(1 for c, routes in hom if len(c['units']) == 1 and not c['drop'] and c['S'] not in (16, 32, 64)) >= FLOOR   # general kernels, one layer of any width
    big = [c for c, routes in hom if any(r.name == 'row-streaming' for r in routes)]
    row = t_hom['row-streaming']
    assert all(row[a] >= 1 for a in ACTS) and all(row[l] >= 1 for l in LOSS_SHORT.values()) and all(row[f] >= 1 for f in FOCI), row
    assert {c['S'] for c in big} == {16, 32, 64}
    assert any(c['Kc'] == 0 for c in big) and any(c['Kc'] == 32 for c in big)
    assert any(c['d'] == 0 and c['A'] > 0 for c in big)                                   # a constants line that holds arc labels only
    assert any(c['focus'] == 'a' and c['S'] != 16 for c in big) and any(c['mode'] != 'average' and c['S'] == 16 for c in big)
    assert any(c['N'] < 16 for c in big) and any(16 <= c['N'] < 64 for c in big)
    for prefix in ('default -> persistent', 'default -> general', 'general -> general', 'type ranges -> row-streaming', 'type ranges -> general'):
        assert sum(row['seeds'] for k, row in t_comp.items() if k.startswith(prefix)) >= FLOOR, (prefix, sorted(t_comp))
    ranges = [(c, r) for c, routes in comp for r in routes if r.expected == C_BIG]
    assert {r.xt for _, r in ranges} == {1, 2}
    assert any(0 in c['counts'] for c, _ in ranges) and any(c['focus'] == 'a' for c, _ in ranges)
    assert any(0 < n < 16 for c, _ in ranges for n in c['counts'])                        # a type range shorter than one tile
    assert any(0 in c['dims'] for c, _ in comp) and {LOSS_SHORT[c['loss']] for c, _ in comp} == set(LOSS_SHORT.values())
    assert any(len(set(c['bn'])) == 2 for c, _ in comp)
    # the persistent kernels with a FIRST type that has no node and no BatchNormalization in front of types that have both (seed 10: the launch
    # took its one BatchNormalization epsilon from the first network - 0 without BatchNormalization - until composite_small_eps)
    assert any(c['counts'][0] == 0 and not c['bn'][0] and any(c['bn'][1:]) and routes[0].expected == C_SMALL for c, routes in comp)
    for cases, n in ((hom, HOM_SEEDS), (comp, COMP_SEEDS)):
        assert sum(1 for c, _ in cases if c['sub'] > 0) <= n // 8, [(c['seed'], c['sub']) for c, _ in cases if c['sub'] > 0]
        assert 0 < sum(1 for c, _ in cases if c['thr'] > 0) < n // 2


# ---- 2. homogeneous routes on the GPU --------------------------------------------------------------------------------------------------------
def last_name():
    return nat.lib().gnn_last_kernel_name().decode()


BLOCKS = Route('building blocks', {}, None, 0, None)      # the Python orchestration of the device primitives: no route of the library


def forced(mp, route, model):
    """Everything a route forces, through `mp` (a monkeypatch context: undone when the route has run); the per-tensor errors that the
    comparison helpers append to $GNN_TEST_ERRLOG carry the route's name."""
    for name in KNOBS: mp.delenv(name, raising=False)
    for name, value in route.env.items(): mp.setenv(name, value)
    if route.use_tiles is not None: mp.setattr(LoopTrainer, 'use_tiles', route.use_tiles)
    mp.setattr(model, 'native_flags', route.flags)
    log = tt.log_rows
    mp.setattr(tt, 'log_rows', lambda tag, rows, **extra: log(tag, rows, route=route.name, **extra))


@pytest.mark.gpu
@pytest.mark.parametrize('seed', range(HOM_SEEDS * FUZZ_SCALE))
def test_fuzz_homogeneous_routes(seed, monkeypatch):
    """One float64 oracle result per seed; the building blocks once, then the in-library step on every route that covers the seed, each
    with the kernel name it must report."""
    c, routes, b = _homogeneous(seed)
    model, nets = b['model'], (b['model'].net_state, b['model'].net_output)
    start = [[w.copy() for w in n.get_weights()] for n in nets]
    print(f"\nseed {seed}.{c['sub']}: " + ', '.join(f'{k}={c[k]}' for k in ('focus', 'd', 'L', 'A', 'T', 'units', 'act', 'loss', 'mode', 'bn', 'K', 'thr', 'drop', 'sizes')))
    try:
        for route in [BLOCKS] + routes:
            for n, w in zip(nets, start): n.set_weights([a.copy() for a in w])      # (a pass moves the BatchNormalization moving statistics)
            with monkeypatch.context() as mp:
                forced(mp, route, model)
                res, want = check_step(model, b['x'], b['y'], b['sw'], b['s0'], loss=c['loss'], avg=c['avg'], native=route is not BLOCKS, seed=b['seed'],
                                       oracle_key=b['key'])
                if route is not BLOCKS: assert last_name() == route.expected, (seed, route.name, last_name())
                print(f"  {route.name:<26} k = {res['k']}  {route.expected or ''}")
    finally:
        for n, w in zip(nets, start): n.set_weights(w)


# ---- 3. composite routes on the GPU ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('seed', range(COMP_SEEDS * FUZZ_SCALE))
def test_fuzz_composite_routes(seed, monkeypatch):
    """The same for heterogeneous models: k, loss, predictions, the final state in the caller's node order, every network's gradients and
    the moving statistics (`composite_compare`), on the building blocks and on the three routes of the in-library step."""
    c, routes, b = _composite(seed)
    model = b['model']
    model.compile(optimizer=SGD(0.0), loss=c['loss'], average_st_grads=c['avg'])
    want = cached_oracle(b['key'], lambda: composite_oracle_step(model, b['x'], b['y'], b['sw'], b['s0'], loss=c['loss'], avg=c['avg']))
    start = composite_weights(model)
    print(f"\nseed {seed}.{c['sub']}: " + ', '.join(f'{k}={c[k]}' for k in ('focus', 'D', 'dims', 'A', 'T', 'acts', 'bn', 'loss', 'mode', 'K', 'thr', 'counts', 'sizes')))
    try:
        for route in [BLOCKS] + routes:
            set_composite_weights(model, start)
            with monkeypatch.context() as mp:
                forced(mp, route, model)
                summary, _ = composite_compare(model, b['x'], b['y'], b['sw'], b['s0'], want, route is not BLOCKS,
                                               tag=os.environ.get('PYTEST_CURRENT_TEST', ''))
                if route is not BLOCKS: assert route_matches(route, last_name()), (seed, route.name, last_name())
                print(f"  {route.name:<16} k = {want['k']}  {last_name() if route is not BLOCKS else ''}\n      {summary}")
    finally:
        set_composite_weights(model, start)
