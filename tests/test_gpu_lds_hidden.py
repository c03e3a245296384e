"""The hidden-layer form of the one-CU-per-group inference kernels (csrc/kernel_state_lds.hpp `LdsHidden`; opt-in: `model.native_flags |=
nat.FLAG_LDS_HIDDEN`): convergence groups of models whose state network is Dense(H) - Dense(state width), homogeneous
(`k_state_lds<.., hidden>`) and composite (`k_state_lds_types<.., hidden>`, H and both activations per type), and predict() / evaluate()
through the unchanged planners - against the float64 oracle batch by batch, with the conventions of tests/test_gpu_composite_groups.py:
TOL = 1e-5 on rel_err = max|a - b| / max|b|, k exact, and with a threshold the float64 k first asserted not to move at threshold x (1 +- 1e-3)
(`oracle_k_is_firm`; the seeds below were chosen on the CPU so that it holds).

Groups are a handful of graphs of 1 .. 60 nodes (one case: a single ~700-node group, the single-buffered form at width 32)."""
import numpy as np
import pytest
import torch

from gnnkeras_amd import GraphObject
from gnnkeras_amd import _native as nat
from gnnkeras_amd.Models.MLP import MLP
from gnnkeras_amd.Sequencers.GraphSequencers import CompositeMultiGraphSequencer, MultiGraphSequencer
from oracle.harness import oracle_loop, rel_err
from test_gpu_parity import TOL, CLS, CCLS, dev, _graph_with_long_rows, _last_kernel, _random_graph, _with_arc_weights
from test_gpu_composite_groups import K_MARGIN, case_graphs, oracle_k_is_firm, run_groups, states0, with_mode
from test_gpu_composite_grouped import typed_graphs

pytestmark = pytest.mark.gpu
L, A, T = 5, 3, 2


# ---- models ----------------------------------------------------------------------------------------------------------------------------------------
def hidden_model(focus, d, H, acts=('tanh', 'tanh'), max_it=5, thr=0.0, scale=0.5, labels=L, seed=0, flag=True):
    """A homogeneous model with state network Dense(H, acts[0]) - Dense(S, acts[1]) (S = d, or the label width for d = 0)."""
    S = d or labels
    ns = MLP((2 * S + 2 * labels + A if d else 2 * S + A,), [H, S], list(acts), 'lecun_normal', 'lecun_normal', rng=seed + 10)
    ns.set_weights([w * scale if w.ndim == 2 else w + 0.05 for w in ns.get_weights()])             # (biases off zero: b2 must arrive)
    node_part = S + labels if d else S
    no = MLP((2 * node_part + A if focus == 'a' else node_part,), [T], 'softmax', 'glorot_normal', 'glorot_normal', rng=seed + 11)
    model = CLS[focus](ns, no, d, max_it, thr)
    model.native_flags = nat.FLAG_LDS_HIDDEN if flag else 0
    return model


def composite_hidden_model(focus, dims, d, hidden, acts=None, max_it=5, thr=0.0, scale=0.5, seed=0, flag=True):
    """A composite model, type t's state network Dense(hidden[t], acts[t][0]) - Dense(S, acts[t][1])."""
    S = d if d > 0 else max(dims)
    ns = []
    for t, dt in enumerate(dims):
        n_ = MLP((dt + 2 * S + sum(dims) + A,), [hidden[t], S], list(acts[t]) if acts else ['tanh', 'tanh'], 'lecun_normal', 'lecun_normal', rng=seed + 30 + t)
        n_.set_weights([w * scale if w.ndim == 2 else w + 0.05 for w in n_.get_weights()])
        ns.append(n_)
    no = MLP((2 * S + A if focus == 'a' else S,), [T], 'softmax', 'glorot_normal', 'glorot_normal', rng=seed + 50)
    model = CCLS[focus](ns, no, d, max_it, thr)
    model.native_flags = nat.FLAG_LDS_HIDDEN if flag else 0
    return model


def firm_k(model, x, s0):
    """The float64 oracle's (k, state, out) of a homogeneous batch, k asserted not to move with the threshold by +- K_MARGIN."""
    k64, st64, o64 = oracle_loop(model, x, s0, np.float64)
    thr = model.state_threshold
    if thr > 0:
        try:
            for f in (1 - K_MARGIN, 1 + K_MARGIN):
                model.state_threshold = thr * f
                assert float(oracle_loop(model, x, s0, np.float64)[0]) == float(k64), 'borderline k in float64: choose another seed'
        finally:
            model.state_threshold = thr
    return float(k64), st64, o64


def kernel_name(model, S, weights=False, db=True, typed=False):
    sp = 16 if S <= 16 else 32
    return f'k_state_lds{"_types" if typed else ""}<{sp},{"true" if weights else "false"},{"true" if db else "false"},hidden>'


def run_hidden(model, xs, x_merged, begin, s0s, tag, db=True, weights=False, group_sets=None, fine=None, check_alone=True):
    """ONE `Loop(groups=...)` over the merged batches `xs` against the float64 oracle and the call on every batch alone."""
    d = model.state_vect_dim
    S = d or int(xs[0][0].shape[1])
    s0 = dev(np.concatenate(s0s)) if d else None
    kw = {} if group_sets is None else {'group_sets': group_sets}
    k, st, o = model.Loop(*model.process_inputs(x_merged), state0=s0, groups=begin if fine is None else fine, **kw)
    name = _last_kernel()
    torch.cuda.synchronize()
    assert name == kernel_name(model, S, weights, db), (tag, name)
    assert k.shape == (len(xs),), (tag, k.shape)
    k, st, o = k.cpu().numpy(), st.cpu().numpy(), o.cpu().numpy()
    assert np.all(np.isfinite(st)) and np.all(np.isfinite(o))
    r0, ks = 0, []
    for j, xb in enumerate(xs):
        k64, st64, o64 = firm_k(model, xb, s0s[j] if d else None)
        rows = o64.shape[0]
        e_st, e_o = rel_err(st[begin[j]:begin[j + 1]], st64), rel_err(o[r0:r0 + rows], o64)
        print(f'{tag} batch {j}: n = {begin[j + 1] - begin[j]}, k = {k[j]} (float64 {k64}), rel_err state {e_st:.2e} out {e_o:.2e}')
        assert float(k[j]) == k64, (tag, j, float(k[j]), k64)
        assert e_st <= TOL and e_o <= TOL, (tag, j, e_st, e_o)
        if check_alone:                             # `Loop()` on the batch alone: no group table, so none of the group kernels
            kb, stb, ob = model.Loop(*model.process_inputs(xb), state0=dev(s0s[j]) if d else None)
            assert not _last_kernel().startswith('k_state_lds'), _last_kernel()
            assert float(kb) == float(k[j]), (tag, j, float(kb), float(k[j]))
            assert rel_err(st[begin[j]:begin[j + 1]], stb.cpu().numpy()) <= TOL and rel_err(o[r0:r0 + rows], ob.cpu().numpy()) <= TOL
        r0 += rows
        ks.append(float(k[j]))
    assert r0 == o.shape[0]
    return ks


def one_node_graph(rng, focus):
    return GraphObject(nodes=rng.normal(size=(1, L)), arcs=np.zeros((0, 2 + A)), targets=rng.normal(size=(0 if focus == 'a' else 1, 2)), focus=focus)


def graphs_of(rng, sizes, focus='n', mode='average', labels=L):
    return [one_node_graph(rng, focus) if n == 1 and labels == L else _random_graph(rng, n, 3 * n, labels, A, focus=focus, mode=mode) for n in sizes]


def batches_of(gl, focus, mode, per_batch=1):
    seq = MultiGraphSequencer(gl, focus, mode, per_batch, shuffle=False)
    x, begin = seq.merged_batches(0, len(seq))
    return seq, [seq[i][0] for i in range(len(seq))], x, begin


def draw_s0(rng, xs, d, spread=False):
    return [rng.normal(0, 0.1 * (1 + i if spread else 1), (x[0].shape[0], d)).astype(np.float32) if d else None for i, x in enumerate(xs)]


# ---- 1. homogeneous models: tiles, widths, H edges, activations, iteration limits ------------------------------------------------------------------
TILES = (1, 15, 16, 17, 33)                  # groups of 1 node without arcs, and on either side of one and two 16-row tiles
HOMOGENEOUS = {
    # focus, mode, d, H, (hidden activation, last activation), threshold, max_iteration, sizes
    'tiles_w16_H16_S6':      ('n', 'average', 6, 16, ('tanh', 'tanh'), 0.0, 5, TILES),            # H = 16 with S = 6: H = SP
    'tiles_w32_H32':         ('n', 'sum', 32, 32, ('tanh', 'tanh'), 0.0, 5, TILES),               # H = SP at width 32
    'H1_w16':                ('n', 'average', 6, 1, ('tanh', 'tanh'), 0.0, 5, (9, 33, 20)),
    'H5_w32_graph':          ('g', 'average', 20, 5, ('tanh', 'tanh'), 0.0, 5, (9, 33, 20)),
    'H1_w32_arc':            ('a', 'average', 20, 1, ('selu', 'tanh'), 0.0, 5, (9, 33, 20)),
    'sigmoid_H5_w16':        ('n', 'average', 6, 5, ('sigmoid', 'tanh'), 0.0, 5, (17, 40)),       # act(0) = 0.5 on the pad hidden columns
    'softplus_H9_w32':       ('n', 'average', 20, 9, ('softplus', 'tanh'), 0.0, 5, (17, 40)),     # act(0) = log 2
    'softplus_sigmoid_w16':  ('n', 'sum', 12, 9, ('softplus', 'sigmoid'), 0.0, 5, (17, 40)),      # ... and on the pad STATE columns
    'selu_relu_w32':         ('n', 'average', 20, 20, ('selu', 'relu'), 0.0, 5, (17, 40)),
    'relu_linear_w16':       ('n', 'average', 16, 12, ('relu', 'linear'), 0.0, 4, (17, 40)),
    'tanh_linear_w32':       ('g', 'average', 32, 20, ('tanh', 'linear'), 0.0, 4, (17, 40)),
    'elu_selu_w16':          ('n', 'average', 6, 16, ('elu', 'selu'), 0.0, 5, (17, 40)),
    'd0_labels14_H9':        ('g', 'average', 0, 9, ('tanh', 'tanh'), 0.0, 5, (12, 30, 7)),       # the starter shape with a hidden layer
    'max_iteration_1':       ('n', 'average', 20, 20, ('tanh', 'tanh'), 0.0, 1, (17, 40, 5)),
    'thr_w16':               ('n', 'average', 6, 9, ('tanh', 'tanh'), 0.01, 30, (12, 30, 7, 55, 21, 40)),
    'thr_w32':               ('g', 'average', 32, 20, ('tanh', 'selu'), 0.01, 30, (12, 30, 7, 55, 21, 40)),
}


def homogeneous_case(case):
    focus, mode, d, H, acts, thr, max_it, sizes = HOMOGENEOUS[case]
    rng = np.random.default_rng(sum(map(ord, case)))
    labels = 14 if d == 0 else L
    gl = graphs_of(rng, sizes, focus, mode, labels)
    # (weight scales of the threshold cases: contractions under which the float64 k is firm and differs between the groups)
    model = hidden_model(focus, d, H, acts, max_it, thr, scale={'thr_w16': 0.35, 'thr_w32': 0.6}.get(case, 0.5), labels=labels)
    return model, gl, rng


@pytest.mark.parametrize('case', list(HOMOGENEOUS))
def test_homogeneous_groups_match_float64_oracle(case):
    focus, mode, d, H, acts, thr, max_it, sizes = HOMOGENEOUS[case]
    model, gl, rng = homogeneous_case(case)
    seq, xs, x, begin = batches_of(gl, focus, mode)
    ks = run_hidden(model, xs, x, begin, draw_s0(rng, xs, d, spread=thr > 0), case)
    if thr == 0: assert ks == [float(max_it)] * len(sizes)
    else: assert len(set(ks)) > 1 and max(ks) < max_it, ('the groups were meant to stop early, at different k', ks)


# ---- 2. long CSR rows, per-arc weights against row scale, the single-buffered form ------------------------------------------------------------------
LONG_ROWS = {
    # mode (row scale: 'average'; none: 'sum'), per-arc weights, d, H, threshold, max_iteration, sizes, double-buffered
    'avg_w16':          ('average', False, 6, 9, 0.0, 5, (20, 45), True),
    'sum_w32':          ('sum', False, 20, 5, 0.0, 5, (20, 45), True),
    'weights_w16':      ('sum', True, 6, 16, 0.0, 5, (20, 45), True),
    'weights_w32_thr':  ('sum', True, 20, 20, 0.02, 12, (20, 60, 45), True),
    'single_w32':       ('average', False, 32, 20, 0.0, 3, (20, 700, 45), False),       # 700 nodes do not fit LDS twice at 32-wide rows
    'single_w32_weights': ('sum', True, 20, 9, 0.0, 3, (700, 33), False),
}


def long_rows_case(case):
    mode, weights, d, H, thr, max_it, sizes, db = LONG_ROWS[case]
    rng = np.random.default_rng(sum(map(ord, case)))
    gl = [_graph_with_long_rows(rng, n, L, A) for n in sizes]           # rows of in-degree 5 .. 8 and 9 .. 12 in every group
    for g in gl: g.setAggregation(mode)
    ws = [rng.uniform(0.2, 1.0, g.arcs.shape[0]) / (4.0 if thr > 0 else 1.0) for g in gl] if weights else None
    s0s = [rng.normal(0, 0.1 * (1 + i), (n, d)).astype(np.float32) for i, n in enumerate(sizes)]
    model = hidden_model('n', d, H, ('tanh', 'tanh'), max_it, thr, scale=0.3)
    return model, gl, ws, s0s


@pytest.mark.parametrize('case', list(LONG_ROWS))
def test_long_rows_arc_weights_and_the_single_buffered_form(case):
    mode, weights, d, H, thr, max_it, sizes, db = LONG_ROWS[case]
    model, gl, ws, s0s = long_rows_case(case)
    begin = [0] + [int(v) for v in np.cumsum(sizes)]
    if weights:
        m = GraphObject.merge(gl, 'n', 'sum')
        x, xs = _with_arc_weights(m, np.concatenate(ws)), [_with_arc_weights(g, w) for g, w in zip(gl, ws)]
    else:
        seq, xs, x, begin_seq = batches_of(gl, 'n', mode)
        assert begin_seq == begin
    ks = run_hidden(model, xs, x, begin, s0s, case, db=db, weights=weights, check_alone=max(sizes) < 100)
    if thr == 0: assert ks == [float(max_it)] * len(sizes)
    else: assert min(ks) < max_it, ks


# ---- 3. a batch cut into parts (group sets) -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('thr', [0.0, 0.01])
def test_group_sets_report_one_k_per_cut_batch(thr, monkeypatch):
    """Batch 0 (4 graphs) cut into three parts, batch 1 into two: five groups, two sets; every part reports the k of its set, which is the
    k of the uncut batch."""
    import gnnkeras_amd.Models.GNN as G
    rng = np.random.default_rng(11)
    sizes = [30, 45, 12, 60, 25, 18, 50, 33]
    gl = graphs_of(rng, sizes)
    model = hidden_model('n', 20, 9, ('tanh', 'tanh'), 12, thr, scale=0.35 if thr > 0 else 0.5)
    seq, xs, x, begin = batches_of(gl, 'n', 'average', per_batch=4)
    n = sizes
    fine = [0, n[0] + n[1], n[0] + n[1] + n[2], sum(n[:4]), sum(n[:7]), sum(n)]
    seen = {}
    fold = G.fold_sets
    monkeypatch.setattr(G, 'fold_sets', lambda k, set_id, n_sets: (seen.__setitem__('k', k.cpu().numpy()), fold(k, set_id, n_sets))[1])
    ks = run_hidden(model, xs, x, begin, draw_s0(rng, xs, 20), f'sets thr {thr}', group_sets=[0, 3, 5], fine=fine)
    assert seen['k'].shape == (5,) and np.all(seen['k'][:3] == ks[0]) and np.all(seen['k'][3:] == ks[1]), (seen['k'], ks)
    if thr == 0: assert ks == [12.0, 12.0]


# ---- 4. composite models -----------------------------------------------------------------------------------------------------------------------------------
ACTS3 = (('sigmoid', 'tanh'), ('relu', 'linear'), ('softplus', 'selu'))
COMPOSITE = {
    # focus, mode, dims, d, H per type, activations per type, threshold, max_iteration
    'n_3types_w16':      ('n', 'composite_average', (5, 3, 4), 6, (5, 16, 9), ACTS3, 0.0, 5),
    'a_3types_w32':      ('a', 'average', (5, 3, 4), 20, (5, 16, 9), ACTS3, 0.0, 4),
    'g_3types_w16_thr':  ('g', 'sum', (5, 3, 4), 6, (5, 16, 9), None, 0.01, 12),
    'n_3types_w32_thr':  ('n', 'composite_average', (5, 3, 4), 32, (5, 16, 9), None, 0.01, 12),
    'g_3types_d0':       ('g', 'average', (6, 6, 6), 0, (5, 16, 9), ACTS3, 0.0, 5),
    'n_1type_thr':       ('n', 'average', (7,), 10, (5,), None, 0.01, 10),
    'n_8types_w16':      ('n', 'composite_average', (3, 2, 4, 3, 2, 4, 3, 2), 12, (5, 16, 9, 5, 16, 9, 5, 16), ACTS3 * 3, 0.0, 5),
    'a_8types_w32_thr':  ('a', 'sum', (3, 2, 4, 3, 2, 4, 3, 2), 20, (5, 16, 9, 5, 16, 9, 5, 16), None, 0.01, 10),
}


def composite_case(case):
    focus, mode, dims, d, hidden, acts, thr, max_it = COMPOSITE[case]
    rng = np.random.default_rng(sum(map(ord, case)))
    gl = with_mode(case_graphs(rng, focus, dims)[:6], mode)            # 14, 9, 30 nodes, ONE node, 150 and 22 nodes; some lack a type
    model = composite_hidden_model(focus, dims, d, hidden, [acts[t] for t in range(len(dims))] if acts else None, max_it, thr,
                                   scale=0.3 if thr > 0 else 0.5)
    return model, gl, rng


@pytest.mark.parametrize('case', list(COMPOSITE))
def test_composite_groups_match_float64_oracle(case):
    focus, mode, dims, d, hidden, acts, thr, max_it = COMPOSITE[case]
    model, gl, rng = composite_case(case)
    seq = CompositeMultiGraphSequencer(gl, focus, mode, 1, shuffle=False)
    ks = run_groups(model, seq, list(range(len(seq))), states0(rng, seq, d), case, name_end=',true,hidden>')
    if thr == 0: assert ks == [float(max_it)] * len(seq)
    else: assert min(ks) >= 1
    seq2 = CompositeMultiGraphSequencer(gl, focus, mode, 2, shuffle=False)          # larger groups: three batches of two graphs
    run_groups(model, seq2, [0, 1, 2], states0(rng, seq2, d), case + ' x2', name_end=',true,hidden>')


def test_composite_group_sets_and_the_single_buffered_form():
    dims, d = (5, 3, 4), 20
    rng = np.random.default_rng(5)
    gl = with_mode(typed_graphs(rng, [30, 45, 12, 60, 25, 18, 50, 33], 900, 'n', absent=2, lonely=5, dims=dims), 'composite_average')
    seq = CompositeMultiGraphSequencer(gl, 'n', 'composite_average', 4, shuffle=False)
    model = composite_hidden_model('n', dims, d, (5, 16, 9), ACTS3, 12, 0.0)
    n = [g.nodes.shape[0] for g in gl]
    fine = [0, n[0] + n[1], n[0] + n[1] + n[2], sum(n[:4]), sum(n[:7]), sum(n)]
    ks = run_groups(model, seq, [0, 1], states0(rng, seq, d), 'composite sets', group_sets=[0, 3, 5], fine=fine, name_end=',true,hidden>')
    assert ks == [12.0, 12.0]
    # one group above what fits LDS twice at width 32 with three types (533 nodes without the hidden form's three 4 KB blocks)
    gl = with_mode(typed_graphs(rng, [35, 640, 20], 1500, 'n', absent=2, dims=dims), 'sum')
    seq = CompositeMultiGraphSequencer(gl, 'n', 'sum', 1, shuffle=False)
    model = composite_hidden_model('n', dims, d, (5, 16, 9), ACTS3, 3, 0.0, scale=0.3)
    ks = run_groups(model, seq, [0, 1, 2], states0(rng, seq, d), 'composite single-buffered', check_alone=False, name_end=',false,hidden>')
    assert ks == [3.0] * 3


# ---- 5. determinism ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_same_launch_twice_is_bit_identical():
    rng = np.random.default_rng(2)
    for d, H, sizes in ((6, 9, (30, 55, 7)), (32, 20, (40, 17, 60))):
        gl = graphs_of(rng, sizes)
        model = hidden_model('n', d, H, ('softplus', 'tanh'), 10, 0.01, scale=0.35)
        seq, xs, x, begin = batches_of(gl, 'n', 'average')
        s0 = dev(rng.normal(0, 0.1, (begin[-1], d)).astype(np.float32))
        r1 = model.Loop(*model.process_inputs(x), state0=s0, groups=begin)
        name = _last_kernel()
        r2 = model.Loop(*model.process_inputs(x), state0=s0, groups=begin)
        torch.cuda.synchronize()
        assert name == kernel_name(model, d), name
        for a, b in zip(r1, r2): assert torch.equal(a, b)
    dims = (5, 3, 4)
    gl = with_mode(typed_graphs(rng, [30, 60, 7, 44], 1400, 'n', absent=0, dims=dims), 'composite_average')
    seq = CompositeMultiGraphSequencer(gl, 'n', 'composite_average', 1, shuffle=False)
    model = composite_hidden_model('n', dims, 20, (5, 16, 9), ACTS3, 10, 0.01, scale=0.3)
    x, begin = seq.merged_batches(0, len(seq))
    s0 = dev(rng.normal(0, 0.1, (begin[-1], 20)).astype(np.float32))
    r1 = model.Loop(*model.process_inputs(x), state0=s0, groups=begin)
    name = _last_kernel()
    r2 = model.Loop(*model.process_inputs(x), state0=s0, groups=begin)
    torch.cuda.synchronize()
    assert name == 'k_state_lds_types<32,true,true,hidden>', name          # ('composite_average' carries per-arc weights)
    for a, b in zip(r1, r2): assert torch.equal(a, b)


# ---- 6. predict() / evaluate() through the unchanged planners ----------------------------------------------------------------------------------------------
def _walks(model, seq, n_rows):
    """(predictions, evaluation, the kernel of the last launch of predict()) with the model's flags as they are."""
    model.group_batches = True
    p = model.predict(seq); name = _last_kernel(); e = model.evaluate(seq, return_dict=True)
    assert p.shape == (n_rows, T)
    return p, e, name


def test_predict_and_evaluate_of_a_two_layer_model_run_resident_launches():
    """state_vect_dim = 0 keeps the forward deterministic (the state starts from the labels: 20 columns, the 32-wide kernels).  Without
    the flag the planner groups the batches on the spread form; with it every batch is a group of ONE resident launch."""
    rng = np.random.default_rng(4)
    gl = []
    for i in range(96):
        n = int(rng.integers(5, 40))
        g = _random_graph(rng, n, 3 * n, 20, A, focus='g')
        gl.append(GraphObject(nodes=g.nodes, arcs=g.arcs, targets=np.eye(T)[rng.integers(0, T, 1)], focus='g'))
    seq = MultiGraphSequencer(gl, 'g', 'average', 8, shuffle=False)
    model = hidden_model('g', 0, 12, ('tanh', 'tanh'), 15, 0.005, scale=0.3, labels=20)
    model.compile(optimizer='adam', loss='categorical_crossentropy', metrics=['accuracy'])
    dev_ = torch.device('cuda', 0)
    plan = model._group_plan(seq, dev_)
    assert plan is not None and len(plan) == 1 and plan[0].resident and sorted(plan[0]) == list(range(len(seq))), plan
    p1, e1, name = _walks(model, seq, 96)
    assert name == 'k_state_lds<32,false,true,hidden>', name
    model.native_flags = 0
    plan0 = model._group_plan(seq, dev_)
    assert plan0 is not None and not any(bs.resident for bs in plan0), plan0               # (the spread form: what ran before the flag)
    p0, e0, name0 = _walks(model, seq, 96)
    assert name0.startswith('k_state_small'), name0
    print(f'predict rel_err flag on / off {rel_err(p1, p0):.2e}; loss {e1["loss"]:.8f} / {e0["loss"]:.8f}')
    assert rel_err(p1, p0) <= TOL
    assert abs(e1['loss'] - e0['loss']) <= 1e-5 and abs(e1['accuracy'] - e0['accuracy']) <= 1e-6
    model.native_flags = nat.FLAG_LDS_HIDDEN
    for b in (0, len(seq) - 1):                                                           # ... and against the oracle
        k64, st64, o64 = firm_k(model, seq[b][0], None)
        assert rel_err(p1[8 * b:8 * b + o64.shape[0]], o64) <= TOL, b


def test_predict_and_evaluate_of_a_composite_two_layer_model_run_resident_launches():
    """Without the flag a composite model with hidden layers is walked batch by batch (no plan); with it: one resident launch."""
    rng = np.random.default_rng(8)
    dims = (6, 6, 6)
    gl = with_mode(typed_graphs(rng, rng.integers(5, 40, 48), 1100, 'g', absent=3, lonely=7, dims=dims), 'composite_average')
    seq = CompositeMultiGraphSequencer(gl, 'g', 'composite_average', 4, shuffle=False)
    model = composite_hidden_model('g', dims, 0, (5, 16, 9), ACTS3, 15, 0.005, scale=0.3)
    model.compile(optimizer='adam', loss='categorical_crossentropy', metrics=['accuracy'])
    dev_ = torch.device('cuda', 0)
    plan = model._group_plan(seq, dev_)
    assert plan is not None and len(plan) == 1 and plan[0].resident and len(plan[0]) == 12, plan
    p1, e1, name = _walks(model, seq, 48)
    assert name == 'k_state_lds_types<16,true,true,hidden>', name          # ('composite_average' carries per-arc weights)
    model.native_flags = 0
    assert model._group_plan(seq, dev_) is None
    p0, e0, name0 = _walks(model, seq, 48)
    assert not name0.startswith('k_state_lds'), name0
    print(f'composite predict rel_err flag on / off {rel_err(p1, p0):.2e}; loss {e1["loss"]:.8f} / {e0["loss"]:.8f}')
    assert rel_err(p1, p0) <= TOL
    assert abs(e1['loss'] - e0['loss']) <= 1e-5 and abs(e1['accuracy'] - e0['accuracy']) <= 1e-6
    model.native_flags = nat.FLAG_LDS_HIDDEN
    for b in range(0, 12, 4):
        k64, st64, o64 = oracle_k_is_firm(model, seq[b][0], None)
        assert rel_err(p1[4 * b:4 * b + o64.shape[0]], o64) <= TOL, b
