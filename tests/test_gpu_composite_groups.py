"""Inference convergence groups of HETEROGENEOUS models: `CompositeGNN*.Loop(training=False, groups=...)` on the typed one-CU-per-group
kernel (csrc/kernel_state_lds_types.hpp), group sets, and the predict() / evaluate() planner - against the float64 oracle
(`oracle_composite_loop`) batch by batch, with the tolerance of tests/test_gpu_parity.py (TOL = 1e-5, rel_err = max|a - b| / max|b|).

k is exact: against the call on that batch alone and against the oracle.  With a threshold the inputs are first checked not to be borderline:
the float64 oracle must report the same k at threshold x (1 - 1e-3) and x (1 + 1e-3) (float32 rounding moves a row's relative step by
~1e-6; a batch whose k flips within 1e-3 of the threshold would be a coin toss and says nothing about the kernel)."""
import numpy as np
import pytest
import torch

from gnnkeras_amd import CompositeGraphObject
from gnnkeras_amd import _native as nat
from gnnkeras_amd.load_MUTAG import load_composite_graphs
from gnnkeras_amd.Models.MLP import MLP
from gnnkeras_amd.Sequencers.GraphSequencers import CompositeMultiGraphSequencer
from oracle.harness import oracle_composite_loop, rel_err
from test_gpu_parity import TOL, CCLS, dev
from test_gpu_composite_grouped import typed_graphs

pytestmark = pytest.mark.gpu
A, T = 3, 2
K_MARGIN = 1e-3


def _last_kernel():
    return nat.lib().gnn_last_kernel_name().decode()


def nets(dims, d, focus, act='tanh', scale=0.5, hidden=None, seed=0):
    """One state network per type on the composite input layout [labels[:, :d_t] | state | Adj^T state | aggregated_component] (S = d, or
    the label width for d = 0); the output network sees the state (arc focus: both ends' state and the arc label)."""
    S = d if d > 0 else max(dims)
    w_comp = sum(dims) + A
    ns = []
    for t, dt in enumerate(dims):
        lay = ([hidden[t]] if hidden and t in hidden else []) + [S]
        n_ = MLP((dt + 2 * S + w_comp,), lay, act, 'lecun_normal', 'lecun_normal', rng=seed + 30 + t)
        n_.set_weights([a * scale if a.ndim == 2 else a for a in n_.get_weights()])
        ns.append(n_)
    no = MLP((2 * S + A if focus == 'a' else S,), [T], 'softmax', 'glorot_normal', 'glorot_normal', rng=seed + 50)
    return ns, no


def with_mode(graphs, mode):
    for g in graphs: g.setAggregation(mode)
    return graphs


def oracle_k_is_firm(model, x, s0):
    """(k64, state64, out64), after asserting that k does not move when the threshold does by +- K_MARGIN (relative)."""
    k64, st64, o64 = oracle_composite_loop(model, x, s0, np.float64)
    thr = model.state_threshold
    if thr > 0:
        try:
            for f in (1 - K_MARGIN, 1 + K_MARGIN):
                model.state_threshold = thr * f
                assert float(oracle_composite_loop(model, x, s0, np.float64)[0]) == float(k64), 'borderline k in float64: choose another seed'
        finally:
            model.state_threshold = thr
    return float(k64), st64, o64


def run_groups(model, seq, batches, s0s, tag, group_sets=None, fine=None, check_alone=True, name_end=''):
    """ONE `Loop(groups=...)` over the merge of `batches` against the oracle and the call on every batch alone."""
    x, begin = seq.merged_batches(batches)
    d = model.state_vect_dim
    s0 = dev(np.concatenate([s0s[b] for b in batches])) if d else None
    kw = {} if group_sets is None else {'group_sets': group_sets}
    k, st, o = model.Loop(*model.process_inputs(x), state0=s0, groups=begin if fine is None else fine, **kw)
    name = _last_kernel()
    torch.cuda.synchronize()
    assert name.startswith('k_state_lds_types<') and name.endswith(name_end), (tag, name)
    if group_sets is not None:                      # every part reports the k of its set (Loop folds them with amin: look before the fold)
        kg = model._last_k_groups.cpu().numpy()
        assert kg.shape == (len(fine) - 1,), (tag, kg.shape)
        for j in range(len(group_sets) - 1):
            part_k = kg[group_sets[j]:group_sets[j + 1]]
            print(f'{tag} set {j}: k of its parts {part_k.tolist()}')
            assert np.all(part_k == part_k[0]), (tag, j, part_k)
    assert k.shape == (len(batches),), (tag, k.shape)
    k, st, o = k.cpu().numpy(), st.cpu().numpy(), o.cpu().numpy()
    assert np.all(np.isfinite(st)) and np.all(np.isfinite(o))
    r0, ks = 0, []
    for j, b in enumerate(batches):
        xb = seq[b][0]
        k64, st64, o64 = oracle_k_is_firm(model, xb, s0s[b] if d else None)
        rows = o64.shape[0]
        e_st, e_o = rel_err(st[begin[j]:begin[j + 1]], st64), rel_err(o[r0:r0 + rows], o64)
        print(f'{tag} batch {b}: n = {begin[j + 1] - begin[j]}, k = {k[j]} (float64 {k64}), rel_err state {e_st:.2e} out {e_o:.2e}')
        assert float(k[j]) == k64, (tag, b, float(k[j]), k64)
        assert e_st <= TOL and e_o <= TOL, (tag, b, e_st, e_o)
        if check_alone:
            kb, stb, ob = model.Loop(*model.process_inputs(xb), state0=dev(s0s[b]) if d else None)
            assert not _last_kernel().startswith('k_state_lds_types<')
            assert float(kb) == float(k[j]), (tag, b, float(kb), float(k[j]))
            assert rel_err(st[begin[j]:begin[j + 1]], stb.cpu().numpy()) <= TOL and rel_err(o[r0:r0 + rows], ob.cpu().numpy()) <= TOL
        r0 += rows
        ks.append(float(k[j]))
    assert r0 == o.shape[0]
    return ks


def states0(rng, seq, d):
    return [rng.normal(0, 0.1, (seq[i][0][0].shape[0], d)).astype(np.float32) if d else None for i in range(len(seq))]


# ---- 3. Loop(groups=...) against the float64 oracle, batch by batch --------------------------------------------------------------------------------
CASES = {
    # focus, mode, dims, d, threshold, max_iteration
    'n_cavg_w16_thr0':   ('n', 'composite_average', (5, 3, 4), 6, 0.0, 5),
    'a_avg_w32_thr0':    ('a', 'average', (5, 3, 4), 20, 0.0, 4),
    'g_sum_w16_thr':     ('g', 'sum', (5, 3, 4), 6, 0.01, 12),
    'n_cavg_w32_thr':    ('n', 'composite_average', (5, 3, 4), 32, 0.01, 12),
    'g_avg_d0_thr0':     ('g', 'average', (6, 6, 6), 0, 0.0, 5),
    'n_avg_1type_thr':   ('n', 'average', (7,), 10, 0.01, 10),
    'n_cavg_8types_thr0': ('n', 'composite_average', (3, 2, 4, 3, 2, 4, 3, 2), 12, 0.0, 5),
    'a_sum_8types_thr':  ('a', 'sum', (3, 2, 4, 3, 2, 4, 3, 2), 20, 0.01, 10),
}


def single_node(dims, focus):
    """A graph of ONE node (type 0) without arcs: one output row for node / graph focus, none for arc focus."""
    tm = np.zeros((1, len(dims)), bool); tm[0, 0] = True
    rows = 0 if focus == 'a' else 1
    nodes = np.zeros((1, max(dims))); nodes[0, 0] = 1.0
    return CompositeGraphObject(nodes=nodes, arcs=np.zeros((0, 2 + A)), targets=np.eye(T)[np.zeros(rows, int)], type_mask=tm, dim_node_label=dims,
                                focus=focus, set_mask=np.ones(rows, bool), output_mask=np.ones(rows, bool), aggregation_mode='composite_average')


def many_type_graphs(rng, sizes, dims, focus, seed0):
    """Graphs whose node types are drawn uniformly over len(dims) types (1 or 8 here: with 8, small graphs lack some of them)."""
    from gnnkeras_amd.synth import er_composite_graph
    out = []
    for i, n in enumerate(sizes):
        g = er_composite_graph(n, int(rng.integers(n, 3 * n)), dim_node_label=dims, seed=seed0 + i)
        rows = g.arcs.shape[0] if focus == 'a' else n
        if focus == 'g': sm, om, n_t = np.ones(n, bool), np.ones(n, bool), 1
        else:
            om, sm = rng.random(rows) < 0.7, rng.random(rows) < 0.8
            om[0] = sm[0] = True
            n_t = int(om.sum())
        out.append(CompositeGraphObject(nodes=g.nodes, arcs=g.arcs, targets=np.eye(T)[rng.integers(0, T, n_t)], type_mask=g.type_mask,
                                        dim_node_label=dims, focus=focus, set_mask=sm, output_mask=om, aggregation_mode='composite_average'))
    return out


def case_graphs(rng, focus, dims):
    """Ten graphs: with three types one lacks type 2 and one keeps a single row of type 1; one graph is ONE node; one has 150 nodes
    (several 16-row tiles per type)."""
    if len(dims) == 3:
        gl = typed_graphs(rng, [14, 9, 30], 300, focus, absent=0, lonely=1, dims=dims)
        gl += [single_node(dims, focus)]
        gl += typed_graphs(rng, [150, 22, 40, 11, 17, 25], 320, focus, absent=3, dims=dims)
    else:
        gl = many_type_graphs(rng, [14, 9, 30], dims, focus, 500) + [single_node(dims, focus)] + many_type_graphs(rng, [150, 22, 40, 11, 17, 25], dims, focus, 520)
    return gl


@pytest.mark.parametrize('case', list(CASES))
def test_loop_groups_match_float64_oracle(case):
    focus, mode, dims, d, thr, max_it = CASES[case]
    rng = np.random.default_rng(sum(map(ord, case)))
    gl = case_graphs(rng, focus, dims)
    with_mode(gl, mode)
    seq = CompositeMultiGraphSequencer(gl, focus, mode, 1, shuffle=False)           # one graph per batch: groups of 1 .. 150 nodes
    ns, no = nets(dims, d, focus, scale=0.3 if thr > 0 else 0.5)
    model = CCLS[focus](ns, no, d, max_it, thr)
    s0s = states0(rng, seq, d)
    ks = run_groups(model, seq, list(range(len(seq))), s0s, case)
    if thr == 0: assert ks == [float(max_it)] * len(seq)
    else: assert min(ks) >= 1
    # larger groups: three batches of several graphs each through another sequencer over the same graphs
    seq3 = CompositeMultiGraphSequencer(gl, focus, mode, 4, shuffle=False)
    s3 = states0(rng, seq3, d)
    run_groups(model, seq3, [0, 1, 2], s3, case + ' x4')


def test_threshold_cases_stop_at_different_k():
    """The early exit is per group: with a threshold the groups of one launch leave after different iteration counts."""
    focus, mode, dims, d, thr, max_it = 'n', 'composite_average', (5, 3, 4), 6, 0.02, 30
    rng = np.random.default_rng(77)
    gl = with_mode(typed_graphs(rng, [6, 40, 150, 12, 80, 9, 33, 20], 700, focus, absent=1, lonely=2, dims=dims), mode)
    seq = CompositeMultiGraphSequencer(gl, focus, mode, 1, shuffle=False)
    ns, no = nets(dims, d, focus, scale=0.45)
    model = CCLS[focus](ns, no, d, max_it, thr)
    ks = run_groups(model, seq, list(range(len(seq))), states0(rng, seq, d), 'different k')
    assert len(set(ks)) > 1 and max(ks) < max_it, ks


# the single-buffered form: a launch takes it when its largest group does not fit in LDS twice - with three types above 533 nodes at width 32
# (two state copies + record + Orig = 276 B per position, 45 pad positions, 4 B per node for Inv, against 161 792 B) and above 1 020 at width
# 16 (148 B per position).  The new state of an iteration then goes through the staging rows in global memory, every group behind the padded
# sizes of the groups before it: several groups per launch, the large ones not first, one of them without type 2.
SINGLE = {
    # mode, d, threshold, max_iteration, sizes, absent, lonely
    'w32_cavg_thr':  ('composite_average', 32, 0.01, 12, [90, 640, 610, 35], 2, 0),
    'w32_sum_thr0':  ('sum', 20, 0.0, 4, [35, 700, 90], 1, 2),
    'w16_avg_thr':   ('average', 6, 0.01, 12, [200, 1100, 1070, 50], 2, 3),
    'w16_cavg_thr0': ('composite_average', 12, 0.0, 4, [1200, 50, 1090], 2, 1),
}


@pytest.mark.parametrize('case', list(SINGLE))
def test_single_buffered_groups_match_float64_oracle(case):
    mode, d, thr, max_it, sizes, absent, lonely = SINGLE[case]
    dims, focus = (5, 3, 4), 'n'
    rng = np.random.default_rng(sum(map(ord, case)))
    gl = with_mode(typed_graphs(rng, sizes, 1500, focus, absent=absent, lonely=lonely, dims=dims), mode)
    assert max(sizes) > (533 if d > 16 else 1020)
    seq = CompositeMultiGraphSequencer(gl, focus, mode, 1, shuffle=False)
    ns, no = nets(dims, d, focus, scale=0.3 if thr > 0 else 0.5)
    model = CCLS[focus](ns, no, d, max_it, thr)
    ks = run_groups(model, seq, list(range(len(seq))), states0(rng, seq, d), case, name_end=',false>')
    if thr == 0: assert ks == [float(max_it)] * len(seq)
    else: assert min(ks) >= 1 and max(ks) < max_it, ks           # (the flag words of the single-buffered form end the loop)


# ---- 4. a batch cut into parts ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('thr', [0.0, 0.01])
def test_group_sets_report_the_k_of_the_uncut_batch(thr):
    focus, mode, dims, d, max_it = 'n', 'composite_average', (5, 3, 4), 20, 12
    rng = np.random.default_rng(5)
    gl = with_mode(typed_graphs(rng, [30, 45, 12, 60, 25, 18, 70, 33], 900, focus, absent=2, lonely=5, dims=dims), mode)
    seq = CompositeMultiGraphSequencer(gl, focus, mode, 4, shuffle=False)            # two batches of four graphs
    ns, no = nets(dims, d, focus, scale=0.3 if thr > 0 else 0.5)
    model = CCLS[focus](ns, no, d, max_it, thr)
    s0s = states0(rng, seq, d)
    n = [g.nodes.shape[0] for g in gl]
    # batch 0 cut into graphs (0, 1) | (2) | (3), batch 1 into (4, 5, 6) | (7): five groups, two sets
    fine = [0, n[0] + n[1], n[0] + n[1] + n[2], sum(n[:4]), sum(n[:7]), sum(n)]
    ks = run_groups(model, seq, [0, 1], s0s, f'sets thr {thr}', group_sets=[0, 3, 5], fine=fine)
    if thr == 0: assert ks == [float(max_it)] * 2


# ---- 5. predict() / evaluate() -----------------------------------------------------------------------------------------------------------------
def _predict_evaluate(model, seq, tag, oracle_batches=(0,)):
    model.compile(optimizer='adam', loss='categorical_crossentropy', metrics=['accuracy'])
    plan = model._group_plan(seq, torch.device('cuda', 0))
    assert plan is not None and sorted(b for bs in plan for b in bs) == list(range(len(seq))), plan
    assert all(bs.resident for bs in plan if len(bs) > 1) and any(len(bs) > 1 for bs in plan), [(len(bs), bs.resident) for bs in plan]
    model.group_batches = True
    p1 = model.predict(seq)
    assert _last_kernel().startswith('k_state_lds_types<') or len(plan[-1]) == 1, _last_kernel()
    e1 = model.evaluate(seq, return_dict=True)
    model.group_batches = False
    p0 = model.predict(seq); e0 = model.evaluate(seq, return_dict=True)
    model.group_batches = True
    print(f'{tag}: predict rel_err grouped / ungrouped {rel_err(p1, p0):.2e}; loss {e1["loss"]:.8f} / {e0["loss"]:.8f}; accuracy {e1["accuracy"]:.6f} / {e0["accuracy"]:.6f}')
    assert p1.shape == p0.shape and rel_err(p1, p0) <= TOL
    assert abs(e1['loss'] - e0['loss']) <= 1e-5 and abs(e1['accuracy'] - e0['accuracy']) <= 1e-6
    rows = [int(seq[i][1].shape[0]) for i in range(len(seq))]
    for b in oracle_batches:
        k64, st64, o64 = oracle_k_is_firm(model, seq[b][0], None)
        r0 = sum(rows[:b])
        assert rel_err(p1[r0:r0 + rows[b]], o64) <= TOL, (tag, b)
    return plan


def test_predict_and_evaluate_group_typed_batches():
    """48 small typed graphs in batches of 4 (state_vect_dim = 0 keeps the forward deterministic: the state starts from the labels)."""
    rng = np.random.default_rng(8)
    dims = (6, 6, 6)
    gl = with_mode(typed_graphs(rng, rng.integers(5, 40, 48), 1100, 'g', absent=3, lonely=7, dims=dims), 'composite_average')
    seq = CompositeMultiGraphSequencer(gl, 'g', 'composite_average', 4, shuffle=False)
    ns, no = nets(dims, 0, 'g', scale=0.3)
    model = CCLS['g'](ns, no, 0, 15, 0.005)
    plan = _predict_evaluate(model, seq, 'typed batches of 4', oracle_batches=range(12))
    assert len(plan) == 1 and len(plan[0]) == 12, [len(bs) for bs in plan]
    # node focus through the same planner
    gl = with_mode(typed_graphs(rng, rng.integers(5, 40, 40), 1200, 'n', dims=dims), 'average')
    seq = CompositeMultiGraphSequencer(gl, 'n', 'average', 4, shuffle=False)
    ns, no = nets(dims, 0, 'n', scale=0.3)
    _predict_evaluate(CCLS['n'](ns, no, 0, 15, 0.005), seq, 'typed batches of 4, node focus', oracle_batches=range(10))
    # 'normalized' divides by the merged graph's arc count: never grouped
    for g in gl: g.setAggregation('normalized')
    seqn = CompositeMultiGraphSequencer(gl, 'n', 'normalized', 4, shuffle=False)
    assert seqn.merged_batches(0, 2) is None and model._group_plan(seqn, torch.device('cuda', 0)) is None


def test_predict_and_evaluate_composite_mutag_shape():
    """The reference's composite starter shape: one node type, labels of 14 columns, d = 10, 5 iterations, threshold 0.01, 'average', graph
    focus, batches of 32.  predict() draws state_0 inside `Loop`; to compare the grouped walk with the batch-by-batch walk and the oracle,
    `Loop` is wrapped so that every node of the data set always starts from the same row of one fixed draw."""
    gl = load_composite_graphs(limit=256)
    for g in gl: g.setAggregation('average')
    seq = CompositeMultiGraphSequencer(gl, 'g', 'average', 32, shuffle=False)
    d = 10
    ns, no = nets((14,), d, 'g', act='selu', scale=0.3)
    model = CCLS['g'](ns, no, d, 5, 0.01)
    # state_0 fixed per node of the data set: a draw keyed by the node count, so that a merge of batches starts from the concatenation
    rng = np.random.default_rng(3)
    n_all = sum(g.nodes.shape[0] for g in gl)
    bank = torch.from_numpy(rng.normal(0, 0.1, (n_all, d)).astype(np.float32)).cuda()
    # (a batch is found again by its node labels: column 0 of the bank's rows carries them, so no lookup depends on tensor identity)
    labels_all = torch.cat([seq[i][0][0].to('cuda', torch.float32) for i in range(len(seq))])
    starts = np.concatenate([[0], np.cumsum([seq[i][0][0].shape[0] for i in range(len(seq))])])
    loop = model.Loop
    def loop_fixed(nodes, *a, **kw):
        if kw.get('state0') is None and not kw.get('training', False):
            n_ = nodes.shape[0]
            hit = [int(o_) for o_ in starts[:-1] if o_ + n_ <= n_all and torch.equal(labels_all[o_:o_ + n_], nodes.to('cuda', torch.float32))]
            assert hit, 'a batch that is no run of the data set'
            kw['state0'] = bank[hit[0]:hit[0] + n_]
        return loop(nodes, *a, **kw)
    model.Loop = loop_fixed
    model.compile(optimizer='adam', loss='categorical_crossentropy', metrics=['accuracy'])
    plan = model._group_plan(seq, torch.device('cuda', 0))
    assert plan is not None and len(plan) == 1 and plan[0].resident and list(plan[0]) == list(range(len(seq))), plan
    model.group_batches = True
    p1 = model.predict(seq); name = _last_kernel(); e1 = model.evaluate(seq, return_dict=True)
    assert name.startswith('k_state_lds_types<16,'), name
    model.group_batches = False
    p0 = model.predict(seq); e0 = model.evaluate(seq, return_dict=True)
    print(f'composite MUTAG: predict rel_err grouped / ungrouped {rel_err(p1, p0):.2e}; loss {e1["loss"]:.8f} / {e0["loss"]:.8f}')
    assert p1.shape == (256, 2) and rel_err(p1, p0) <= TOL
    assert abs(e1['loss'] - e0['loss']) <= 1e-5 and abs(e1['accuracy'] - e0['accuracy']) <= 1e-6
    off = 0
    for b in range(len(seq)):
        nb_ = seq[b][0][0].shape[0]
        k64, st64, o64 = oracle_k_is_firm(model, seq[b][0], bank[off:off + nb_].cpu().numpy())
        assert rel_err(p1[32 * b:32 * b + o64.shape[0]], o64) <= TOL, b
        off += nb_


# ---- 6. uncovered shapes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('what', ['hidden_layer', 'width40'])
def test_uncovered_shapes_stay_batch_by_batch(what):
    rng = np.random.default_rng(12)
    dims = (5, 3, 4)
    gl = with_mode(typed_graphs(rng, rng.integers(5, 30, 16), 1300, 'n', dims=dims), 'composite_average')
    seq = CompositeMultiGraphSequencer(gl, 'n', 'composite_average', 4, shuffle=False)
    d = 40 if what == 'width40' else 6
    ns, no = nets(dims, d, 'n', hidden={1: 9} if what == 'hidden_layer' else None)
    model = CCLS['n'](ns, no, d, 4, 0.0)
    assert model._group_plan(seq, torch.device('cuda', 0)) is None
    x, begin = seq.merged_batches(0, 2)
    with pytest.raises(NotImplementedError, match='groups'):
        model.Loop(*model.process_inputs(x), groups=begin)
    with pytest.raises(NotImplementedError, match='groups'):
        model.Loop(*model.process_inputs(x), training=True, groups=begin)
    n_out = sum(int(seq[i][1].shape[0]) for i in range(len(seq)))
    assert np.array_equal(model.predict(seq).shape, (n_out, T))


def test_a_graph_of_one_node_trains_like_the_building_blocks():
    """A heterogeneous graph of ONE node (its type mask is (T, 1) after `process_inputs`: the node axis must survive) through
    `Loop(training=True)`, `forward_native` and `train_step(apply=False)`: k, state and output of the building-block `forward()`.  The
    bound is the file's TOL: the two orchestrations differ in the order of float32 sums over < 40 input columns, five iterations."""
    from gnnkeras_amd.Models.training import LoopTrainer
    dims, d = (5, 3, 4), 6
    nodes = np.zeros((1, max(dims))); nodes[0, 1] = 1.0
    tm = np.zeros((1, len(dims)), bool); tm[0, 1] = True
    g = CompositeGraphObject(nodes=nodes, arcs=np.array([[0, 0, 1.0, 0.0, 0.0]]), targets=np.eye(T)[:1], type_mask=tm, dim_node_label=dims, focus='n',
                             aggregation_mode='composite_average')
    x, y, sw = CompositeMultiGraphSequencer([g], 'n', 'composite_average', 1, shuffle=False)[0]
    assert tuple(x[3].shape) == (len(dims), 1, 1)
    ns, no = nets(dims, d, 'n')
    model = CCLS['n'](ns, no, d, 5, 0.0)
    model.compile(optimizer='adam', loss='categorical_crossentropy')
    s0 = dev(np.full((1, d), 0.05, np.float32))
    tp = LoopTrainer(model).forward(x, state0=s0, seed=3)
    k, state, out = model.Loop(*model.process_inputs(x), training=True, state0=s0, seed=3)
    k_n, state_n, out_n = LoopTrainer(model).forward_native(x, state0=s0, seed=3)
    res = LoopTrainer(model).train_step(x, y, sw, state0=s0, seed=3, apply=False)
    torch.cuda.synchronize()
    assert 'grads_ok' in res                  # (the in-library step ran: the building blocks leave no validity word)
    assert float(k) == k_n == res['k'] == tp.k >= 1
    for got_state, got_out in ((state, out), (state_n, out_n), (res['state'], res['y_pred'])):
        assert tuple(got_state.shape) == (1, d) and tuple(got_out.shape) == (1, T)
        assert rel_err(got_state.cpu(), tp.state.cpu()) < TOL and rel_err(got_out.cpu(), tp.y_pred.cpu()) < TOL


# ---- 7. determinism ----------------------------------------------------------------------------------------------------------------------------
def test_grouped_call_twice_is_bit_identical():
    rng = np.random.default_rng(2)
    dims = (5, 3, 4)
    for d, sizes in ((6, [30, 150, 7, 64, 90]), (32, [300, 420, 17]), (32, [60, 600, 580])):        # (width 32 above 533 nodes: the single-buffered form with staging rows)
        gl = with_mode(typed_graphs(rng, sizes, 1400, 'n', absent=0, dims=dims), 'composite_average')
        seq = CompositeMultiGraphSequencer(gl, 'n', 'composite_average', 1, shuffle=False)
        ns, no = nets(dims, d, 'n', scale=0.3)
        model = CCLS['n'](ns, no, d, 10, 0.01)
        x, begin = seq.merged_batches(0, len(seq))
        s0 = dev(rng.normal(0, 0.1, (begin[-1], d)).astype(np.float32))
        r1 = model.Loop(*model.process_inputs(x), state0=s0, groups=begin)
        name = _last_kernel()
        r2 = model.Loop(*model.process_inputs(x), state0=s0, groups=begin)
        torch.cuda.synchronize()
        assert name.startswith('k_state_lds_types<') and name.endswith(',false>' if max(sizes) > 533 else ',true>'), name
        for a, b in zip(r1, r2): assert torch.equal(a, b)
