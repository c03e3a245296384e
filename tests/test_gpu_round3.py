def test_state_widths_129_to_256_run_fused(N, arcs_per_node, d, mode, act, thr):
    """`state_vect_dim` between 129 and 256 (reference GNN.py:26-28 allows any width): one launch per iteration (k_state_xwide_b3: the Dense
    layer as six bf16 products of three-term splits, kernel_state_xwide.hpp) - k, state and output against the fp64 oracle and against the
    un-fused path; row counts that are not multiples of the 32-row tile,
    in-degrees above 16 (the gather's second chunk), per-row and per-arc weights, widths that are not multiples of 32 / 8, an
    activation with f(0) != 0 (pad columns must stay zero), an early exit."""
"""Round-3 parity closure: every path that had not met the oracle on the device.

  * the f4 sequencers (SURVEY §8f rank 4): `SingleGraphSequencer`, `CompositeSingleGraphSequencer`,
    `TransductiveMultiGraphSequencer`, `TransductiveSingleGraphSequencer` batches through the HIP loop against the oracle
    (reference GraphSequencers.py:133-208, :252-266, TransductiveGraphSequencers.py:63-95), incl. the Q7 mask quirk;
  * every batch of the full MUTAG plan - all LDS-resident groups and the spread ones - against the float64 oracle;
  * BASELINE C4 (1 M nodes / 10 M arcs) as 8 emulated shards built from per-rank graph slices;
  * hub rows on shards;
  * the standalone composite `convergence()` step (reference CompositeGNN.py:215-234).

Same tolerance as test_gpu_parity.py: 1e-5 relative (max-norm), k exact."""
import numpy as np
import pytest
import torch

from gnnkeras_amd import _native as nat
from gnnkeras_amd import GraphObject, CompositeGraphObject
from gnnkeras_amd.Models.MLP import MLP, get_inout_dims
from gnnkeras_amd.Models.GNN import GNNnodeBased, GNNgraphBased
from gnnkeras_amd.Models.CompositeGNN import CompositeGNNnodeBased
from gnnkeras_amd.Sequencers.GraphSequencers import (MultiGraphSequencer, SingleGraphSequencer, CompositeMultiGraphSequencer,
                                                     CompositeSingleGraphSequencer)
from gnnkeras_amd.Sequencers.TransductiveGraphSequencers import TransductiveMultiGraphSequencer, TransductiveSingleGraphSequencer
from gnnkeras_amd.synth import er_graph, er_composite_graph, er_graph_slice
from oracle import gnn_oracle as O
from oracle.harness import oracle_loop, oracle_composite_loop, rel_err, _np, _triple

pytestmark = pytest.mark.gpu
TOL = 1e-5


def dev(x):
    return torch.as_tensor(np.asarray(x)).cuda()


def _last_kernel():
    return nat.lib().gnn_last_kernel_name().decode()


def _nets(focus, d, L, A, T, scale=0.4, act='tanh'):
    inp, lay = get_inout_dims('state', L, A, T, focus, d)
    ns = [MLP(i, lay, act, 'lecun_normal', 'lecun_normal', rng=t) for t, i in enumerate(inp)]
    for n in ns: n.set_weights([w * scale if w.ndim == 2 else w for w in n.get_weights()])
    inp, lay = get_inout_dims('output', L, A, T, focus, d)
    no = MLP(inp[0], lay, 'softmax', 'glorot_normal', 'glorot_normal', rng=9)
    return (ns if isinstance(L, (tuple, list)) else ns[0]), no


def _ring_graph(rng, n, L=5, A=2, T=2, n_set=None, extra=3):
    """A connected directed graph: ring + `extra` random arcs per node; node-focused, a subset of the nodes in the set."""
    src = np.concatenate([np.arange(n), rng.integers(0, n, extra * n)])
    dst = np.concatenate([(np.arange(n) + 1) % n, rng.integers(0, n, extra * n)])
    keep = src != dst
    arcs = np.unique(np.concatenate([np.stack([src[keep], dst[keep]], 1), rng.normal(size=(keep.sum(), A)).round(1)], axis=1), axis=0)
    _, first = np.unique(arcs[:, :2], axis=0, return_index=True)            # one arc per (src, dst) pair
    arcs = arcs[np.sort(first)]
    set_mask = np.zeros(n, bool); set_mask[rng.permutation(n)[:n_set or n]] = True
    om = rng.random(n) < 0.8
    return GraphObject(rng.normal(size=(n, L)), arcs, np.eye(T)[rng.integers(0, T, int(om.sum()))], focus='n', set_mask=set_mask,
                       output_mask=om, aggregation_mode='average')


# ----------------------------------------------------------------------------------------------------------------------
# f4: single-graph and transductive sequencers through the HIP loop
# ----------------------------------------------------------------------------------------------------------------------
def test_single_graph_sequencer_through_the_hip_loop():
    """Reference GraphSequencers.py:133-208.  Every batch of a `SingleGraphSequencer` is the whole graph: `x` carries the full
    set_mask (the Q7 quirk, kept), so the model's output covers every row of `set_mask & output_mask` whatever the batch, and
    predict() over B batches is that output B times.  (Round 2's predict() raised AttributeError here: the grouping probe called
    `merged_batches` on a sequencer that has no merged batches.)"""
    rng = np.random.default_rng(0)
    n = 300
    g = _ring_graph(rng, n, n_set=120)
    seq = SingleGraphSequencer(g, 'n', batch_size=50, shuffle=False)
    assert len(seq) == 3
    ns, no = _nets('n', 8, 5, 2, 2)
    model = GNNnodeBased(ns, no, 8, 10, 0.001)
    model.compile(optimizer='adam', loss='categorical_crossentropy', metrics=['accuracy'])
    s0 = rng.normal(0, 0.1, (n, 8)).astype(np.float32)
    x, y, sw = seq[1]
    assert int(_np(x[3]).sum()) == 120 and y.shape[0] == int((seq.batch_masks[1] & g.output_mask).sum())     # Q7
    k64, st64, o64 = oracle_loop(model, x, s0, np.float64)
    k, st, o = model.Loop(*model.process_inputs(x), state0=dev(s0))
    assert float(k) == float(k64) and rel_err(st.cpu().numpy(), st64) <= TOL and rel_err(o.cpu().numpy(), o64) <= TOL
    assert o.shape[0] == int((g.set_mask & g.output_mask).sum())
    # predict(): three batches, batch by batch (no grouping for this sequencer), state_0 drawn on the device: compare with a
    # contractive network whose fixed point does not depend on state_0 beyond the tolerance of the early exit -> use d = 0
    ns0, no0 = _nets('n', 0, 5, 2, 2)
    m0 = GNNnodeBased(ns0, no0, 0, 6, 0.0)
    m0.compile(optimizer='adam', loss='categorical_crossentropy', metrics=['accuracy'])
    assert m0._group_plan(seq, torch.device('cuda', 0)) is None
    pred = m0.predict(seq)
    want = oracle_loop(m0, x, None, np.float64)[2]
    assert pred.shape == (3 * want.shape[0], 2) and rel_err(pred, np.tile(want, (3, 1))) <= TOL
    # evaluate(): meaningful only when one batch covers the whole set (rows of the output = rows of the targets)
    seq1 = SingleGraphSequencer(g, 'n', batch_size=1000, shuffle=False)
    assert len(seq1) == 1
    res = m0.evaluate(seq1, return_dict=True)
    yy = _np(seq1[0][1])
    loss = float(np.mean(-np.sum(yy * np.log(np.clip(want, 1e-7, 1 - 1e-7)), axis=1)))
    assert abs(res['loss'] - loss) < 1e-5 and abs(res['accuracy'] - float(np.mean(want.argmax(1) == yy.argmax(1)))) < 1e-6


def _composite_toy(rng, n, dims=(4, 3), A=2, T=2, n_set=None):
    g = _ring_graph(rng, n, L=max(dims), A=A, T=T, n_set=n_set)
    tm = np.zeros((n, len(dims)), bool); tm[np.arange(n), rng.integers(0, len(dims), n)] = True
    return CompositeGraphObject(g.nodes, g.arcs, g.targets, type_mask=tm, dim_node_label=dims, focus='n', set_mask=g.set_mask,
                                output_mask=g.output_mask, aggregation_mode='composite_average')


def test_composite_single_graph_sequencer_through_the_hip_loop():
    """Reference GraphSequencers.py:252-266: one heterogeneous graph, batches = subsets of set_mask; 10-element x."""
    rng = np.random.default_rng(1)
    n, dims = 400, (4, 3)
    g = _composite_toy(rng, n, dims, n_set=150)
    seq = CompositeSingleGraphSequencer(g, 'n', batch_size=64, shuffle=False)
    assert len(seq) == 3 and len(seq[0][0]) == 10
    ns, no = _nets('n', 6, dims, 2, 2)
    model = CompositeGNNnodeBased(ns, no, 6, 8, 0.0)
    s0 = rng.normal(0, 0.1, (n, 6)).astype(np.float32)
    for i in range(len(seq)):
        x = seq[i][0]
        k64, st64, o64 = oracle_composite_loop(model, x, s0, np.float64)
        k, st, o = model.Loop(*model.process_inputs(x), state0=dev(s0))
        assert float(k) == float(k64) == 8.0
        assert rel_err(st.cpu().numpy(), st64) <= TOL and rel_err(o.cpu().numpy(), o64) <= TOL
    ns0 = [MLP((dt + 2 * max(dims) + sum(dims) + 2,), [max(dims)], 'tanh', 'lecun_normal', 'zeros', rng=t) for t, dt in enumerate(dims)]
    m0 = CompositeGNNnodeBased(ns0, MLP((max(dims),), [2], 'softmax', 'glorot_normal', 'zeros', rng=5), 0, 4, 0.0)
    pred = m0.predict(seq)                                           # state_vect_dim = 0: deterministic forward
    want = oracle_composite_loop(m0, seq[0][0], None, np.float64)[2]
    assert rel_err(pred, np.tile(want, (3, 1))) <= TOL


@pytest.mark.parametrize('rate', [0.5, 0.25])
def test_transductive_multi_graph_sequencer_through_the_hip_loop(rate):
    """Reference TransductiveGraphSequencers.py:13-95: homogeneous graphs re-typed into 2-type heterogeneous graphs (type 1 =
    transductive nodes whose target sits behind their label), merged into batches, fed to the composite loop."""
    rng = np.random.default_rng(2)
    graphs = [_ring_graph(rng, int(n)) for n in rng.integers(20, 60, 12)]
    np.random.seed(3)
    seq = TransductiveMultiGraphSequencer(graphs, 'n', 'average', rate, batch_size=5, shuffle=False)
    assert len(seq) == 3
    L, T = 5, 2
    dims = (L, L + T)
    ns, no = _nets('n', 7, dims, 2, T)
    model = CompositeGNNnodeBased(ns, no, 7, 9, 0.0)
    model.compile(optimizer='adam', loss='categorical_crossentropy', metrics=['accuracy'])
    outs = []
    for i in range(len(seq)):
        x, y, sw = seq[i]
        assert tuple(_np(x[2]).reshape(-1)) == dims and _np(x[3]).shape[0] == 2
        tm = _np(x[3]).reshape(2, -1)
        assert 0 < tm[1].sum() < tm.shape[1]                           # both node types present
        assert not np.any(_np(x[5]).reshape(-1) & tm[1].astype(bool))   # transductive nodes left the output mask
        s0 = rng.normal(0, 0.1, (tm.shape[1], 7)).astype(np.float32)
        k64, st64, o64 = oracle_composite_loop(model, x, s0, np.float64)
        k, st, o = model.Loop(*model.process_inputs(x), state0=dev(s0))
        assert float(k) == float(k64) == 9.0
        assert rel_err(st.cpu().numpy(), st64) <= TOL and rel_err(o.cpu().numpy(), o64) <= TOL
        assert o.shape[0] == y.shape[0]                                # supervised rows = targets that stayed
    # a new split every epoch (reference :56-59), still the same loop
    before = _np(seq[0][0][3]).copy()
    seq.on_epoch_end()
    assert not np.array_equal(before, _np(seq[0][0][3]))
    # predict / evaluate over the batches (state_vect_dim = 0: no random state_0)
    ns0 = [MLP((dt + 2 * (L + T) + sum(dims) + 2,), [L + T], 'tanh', 'lecun_normal', 'zeros', rng=t) for t, dt in enumerate(dims)]
    m0 = CompositeGNNnodeBased(ns0, MLP((L + T,), [T], 'softmax', 'glorot_normal', 'zeros', rng=5), 0, 5, 0.0)
    m0.compile(optimizer='adam', loss='categorical_crossentropy', metrics=['accuracy'])
    want = np.concatenate([oracle_composite_loop(m0, seq[i][0], None, np.float64)[2] for i in range(len(seq))])
    yy = np.concatenate([_np(seq[i][1]) for i in range(len(seq))])
    assert rel_err(m0.predict(seq), want) <= TOL
    res = m0.evaluate(seq, return_dict=True)
    assert abs(res['loss'] - float(np.mean(-np.sum(yy * np.log(np.clip(want, 1e-7, 1 - 1e-7)), axis=1)))) < 1e-5


def test_transductive_single_graph_sequencer_through_the_hip_loop():
    """Reference TransductiveGraphSequencers.py:100-153: one homogeneous graph, re-typed, batches = subsets of set_mask (Q7 as in
    every single-graph sequencer)."""
    rng = np.random.default_rng(4)
    n = 500
    g = _ring_graph(rng, n, n_set=200)
    np.random.seed(5)
    seq = TransductiveSingleGraphSequencer(g, 'n', 0.4, batch_size=80, shuffle=False)
    L, T = 5, 2
    dims = (L, L + T)
    ns, no = _nets('n', 12, dims, 2, T)
    model = CompositeGNNnodeBased(ns, no, 12, 6, 0.0)
    s0 = rng.normal(0, 0.1, (n, 12)).astype(np.float32)
    assert len(seq) == 3
    for i in (0, 2):
        x = seq[i][0]
        k64, st64, o64 = oracle_composite_loop(model, x, s0, np.float64)
        k, st, o = model.Loop(*model.process_inputs(x), state0=dev(s0))
        assert float(k) == float(k64) and rel_err(st.cpu().numpy(), st64) <= TOL and rel_err(o.cpu().numpy(), o64) <= TOL
    seq.on_epoch_end()                                               # new split + reshuffled batches, new device tensors
    x = seq[0][0]
    k64, st64, o64 = oracle_composite_loop(model, x, s0, np.float64)
    k, st, o = model.Loop(*model.process_inputs(x), state0=dev(s0))
    assert rel_err(st.cpu().numpy(), st64) <= TOL and rel_err(o.cpu().numpy(), o64) <= TOL


# ----------------------------------------------------------------------------------------------------------------------
# the full MUTAG plan: EVERY batch against the float64 oracle
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d,K_it,thr', [(32, 50, 0.0), (32, 30, 0.01), (0, 5, 0.01)])
def test_every_batch_of_the_mutag_plan_against_the_oracle(mutag_graphs, d, K_it, thr):
    """The 136 batches as predict() launches them - ONE resident launch (`k_state_lds`): a batch whose state fits one CU's LDS is
    one group (122 of them at d = 32, all 136 at the starter configuration), a bigger one is cut along graph boundaries into
    groups that share only the convergence flag (group sets, round 3) - and EVERY batch's k, state and output against the float64
    oracle run on that batch alone (round 2 compared 2 of the resident groups)."""
    seq = MultiGraphSequencer(mutag_graphs, 'g', 'average', 32, shuffle=False)
    from test_gpu_parity import starter_nets
    ns, no = starter_nets('g', d, scale=0.22 if thr > 0 else 1.0)
    model = GNNgraphBased(ns, no, d, K_it, thr)
    plan = model._group_plan(seq, torch.device('cuda', 0))
    assert plan is not None and sorted(b for bs in plan for b in bs) == list(range(len(seq)))
    assert plan[0].resident and len(plan[0]) >= (len(seq) if d == 0 else 100)
    rng = np.random.default_rng(1)
    s0s = [rng.normal(0, 0.1, (seq[i][0][0].shape[0], d)).astype(np.float32) if d else None for i in range(len(seq))]
    checked, worst, off_by_one = 0, 0.0, []
    for li, bs in enumerate(plan):
        if len(bs) == 1 and not bs.parts:
            k, st, o = model.Loop(*model.process_inputs(seq[bs[0]][0]), state0=None if not d else dev(s0s[bs[0]]))
            k = k.reshape(1); begin = [0, st.shape[0]]
        else:
            x, begin = seq.merged_batches(bs)
            kw, fine = {}, begin
            if bs.parts: fine, kw['group_sets'] = bs.groups_and_sets({b: begin[i + 1] - begin[i] for i, b in enumerate(bs)})
            k, st, o = model.Loop(*model.process_inputs(x), state0=dev(np.concatenate([s0s[b] for b in bs])) if d else None, groups=fine, **kw)
            assert _last_kernel().startswith('k_state_lds' if bs.resident else 'k_state_small'), (li, _last_kernel())
        k, st, o = k.cpu().numpy(), st.cpu().numpy(), o.cpu().numpy()
        r0 = 0
        for j, b in enumerate(bs):
            k64, st64, o64 = oracle_loop(model, seq[b][0], s0s[b], np.float64)
            if thr == 0.0: assert float(k[j]) == float(k64) == K_it
            else: assert abs(float(k[j]) - float(k64)) <= 1, (b, float(k[j]), float(k64))     # a batch sitting on the threshold
            if float(k[j]) == float(k64):
                es, eo = rel_err(st[begin[j]:begin[j + 1]], st64), rel_err(o[r0:r0 + o64.shape[0]], o64)
                assert es <= TOL and eo <= TOL, (b, es, eo)
                worst = max(worst, es, eo)
            else:
                # one iteration apart: the float32 loop stopped next to the float64 one because some node's distance sits ON the
                # threshold.  No batch leaves this test unchecked: the float64 oracle is re-run for exactly the
                # device's k iterations and state / output are held to that; such batches are counted, printed and bounded.
                model.max_iteration, model.state_threshold = int(k[j]), 0.0
                try: kf, stf, of = oracle_loop(model, seq[b][0], s0s[b], np.float64)
                finally: model.max_iteration, model.state_threshold = K_it, thr
                es, eo = rel_err(st[begin[j]:begin[j + 1]], stf), rel_err(o[r0:r0 + o64.shape[0]], of)
                off_by_one.append((b, float(k[j]), float(k64), es, eo))
                assert float(kf) == float(k[j]) and es <= TOL and eo <= TOL, off_by_one[-1]
            r0 += o64.shape[0]
            checked += 1
    assert checked == len(seq)
    print(f'd={d} thr={thr}: {checked} batches, {len(plan)} launches, worst rel err {worst:.2e}; k one off the float64 oracle in '
          f'{len(off_by_one)} of {len(seq)} batches (batch, k device, k fp64, state / output err vs the fp64 oracle stopped at the k of the device): {off_by_one}')
    assert len(off_by_one) <= 2, off_by_one


# ----------------------------------------------------------------------------------------------------------------------
# BASELINE C4 as 8 shards, emulated on one device, every shard built from its own graph slice
# ----------------------------------------------------------------------------------------------------------------------
def _run_slices_on_one_gpu(model, slices, s0, overlap):
    from gnnkeras_amd.distributed import ShardedLoop
    R = len(slices)
    shards = [ShardedLoop(model, gs, r, R, 'cuda', overlap=overlap) for r, gs in enumerate(slices)]
    if overlap: assert all(sl.overlap for sl in shards)
    s0d = torch.from_numpy(s0).cuda()
    for sl in shards:
        sl._load_state0(s0d); sl._setup(); sl._initial_flags()
    n = shards[0].plan.rows_per_slice * shards[0].SP
    for it in range(model.max_iteration):
        for sl in shards:
            if overlap: sl._partial(it); sl._iteration_split(it)
            else: sl._iteration(it)
        for r, src in enumerate(shards):                     # "all-gather": slice r of rank r's buffer -> everyone
            piece = src.buf[(it + 1) & 1].view(-1)[r * n:(r + 1) * n]
            for dst in shards:
                if dst is not src: dst.buf[(it + 1) & 1].view(-1)[r * n:(r + 1) * n].copy_(piece)
    outs = [sl._output() for sl in shards]
    torch.cuda.synchronize()
    return [float(o[0]) for o in outs], np.concatenate([o[1].cpu().numpy() for o in outs]), np.concatenate([o[2].cpu().numpy() for o in outs])


# (BASELINE C4 as 8 shards built from per-rank slices, at full size: tests/test_gpu_round4.py::test_c4_as_8_shards_at_the_timed_depth - 50 iterations,
# overlap split on and off, against the float64 oracle)


def test_hub_rows_on_shards():
    """Rows above 512 in-arcs on a shard (round 2: "hub segments are not supported on shards"): the shard's adjacency is split
    like the single-GPU one, the segment sums land in virtual rows behind the exchanged buffer."""
    from test_gpu_parity import starter_nets, _run_shards_on_one_gpu
    rng = np.random.default_rng(0)
    N, d = 6000, 32
    base = er_graph(N, 30000, seed=3).arc_ids
    hubs = [(17, 3000), (4100, 900)]                                       # (node, in-degree)
    extra = np.concatenate([np.stack([rng.choice(N, deg, replace=False), np.full(deg, h)], 1) for h, deg in hubs])
    ids = np.unique(np.concatenate([base, extra[extra[:, 0] != extra[:, 1]]]), axis=0)
    arcs = np.concatenate([ids, np.eye(3)[rng.integers(0, 3, len(ids))]], axis=1)
    nodes = np.eye(14, dtype=np.float32)[rng.integers(0, 14, N)]
    for mode in ('average', 'sum'):
        g = GraphObject(nodes, arcs, np.eye(2)[rng.integers(0, 2, N)], focus='n', aggregation_mode=mode)
        ns, no = starter_nets('n', d, scale=0.3 if mode == 'average' else 0.01)
        model = GNNnodeBased(ns, no, d, 5, 0.0)
        s0 = rng.normal(0, 0.1, (N, d)).astype(np.float32)
        xg = MultiGraphSequencer([g], 'n', mode, 1, shuffle=False)[0][0]
        k64, st64, o64 = oracle_loop(model, xg, s0, np.float64)
        for R in (1, 3):
            for flags in (0, nat.FLAG_UNFUSED, nat.FLAG_FUSED_GEN4):
                model.native_flags = flags
                ks, st, o = _run_shards_on_one_gpu(model, g, s0, R)
                assert all(k == 5.0 for k in ks)
                assert rel_err(st, st64) <= TOL and rel_err(o, o64) <= TOL, (mode, R, flags, rel_err(st, st64))
        model.native_flags = 0


# ----------------------------------------------------------------------------------------------------------------------
# standalone composite convergence()
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,d', [(700, 6), (40_000, 32)])
def test_composite_convergence_step_matches_oracle(N, d):
    """`CompositeGNNnodeBased.convergence` (reference CompositeGNN.py:215-234) as a public method: one step, per-type networks on
    per-type rows, against the oracle's `composite_convergence`; chaining two steps equals Loop(max_iteration = 2)."""
    rng = np.random.default_rng(7)
    dims = (5, 3, 4)
    g = er_composite_graph(N, 8 * N, dim_node_label=dims, aggregation_mode='composite_average', seed=11)
    seq = CompositeMultiGraphSequencer([g], 'n', 'composite_average', 1, shuffle=False)
    x = seq[0][0]
    ns, no = _nets('n', d, dims, 3, 2)
    model = CompositeGNNnodeBased(ns, no, d, 2, 0.0)
    nodes, arcs, dim_node_label, type_mask, set_mask, output_mask, cas, adjacency, arcnode, nodegraph = model.process_inputs(x)
    s0 = rng.normal(0, 0.1, (N, d)).astype(np.float32)
    # oracle: aggregated_component as Loop builds it (CompositeGNN.py:251-253), then one convergence()
    f64 = np.float64
    nodes_h, arcs_h = _np(x[0]).astype(f64), _np(x[1]).astype(f64)
    agg_nodes = [O.sparse_dense_matmul_adjoint(*_triple(c), nodes_h[:, :dt], f64) for c, dt in zip(x[6], dims)]
    agg_arcs = O.sparse_dense_matmul_adjoint(*_triple(x[8]), arcs_h[:, 2:], f64)
    comp = np.concatenate(agg_nodes + [agg_arcs], axis=1)
    tm = _np(x[3]).reshape(len(dims), -1).astype(bool)
    want1 = O.composite_convergence(s0.astype(f64), nodes_h, list(dims), tm, _triple(x[7]), comp, [n.spec() for n in ns], False, f64)
    for flags in (0, nat.FLAG_UNFUSED):
        model.native_flags = flags
        out = model.convergence(0.0, dev(s0), None, nodes, dim_node_label, type_mask, adjacency, None, False,
                                arcs=arcs, arcnode=arcnode, composite_adjacencies=cas)
        assert len(out) == 9 and out[0] == 1.0 and out[2] is not None
        assert rel_err(out[1].cpu().numpy(), want1) <= TOL, (flags, rel_err(out[1].cpu().numpy(), want1))
        out2 = model.convergence(out[0], out[1], out[2], nodes, dim_node_label, type_mask, adjacency, None, False,
                                 arcs=arcs, arcnode=arcnode, composite_adjacencies=cas)
        k, st, o = model.Loop(*model.process_inputs(x), state0=dev(s0))
        assert float(k) == 2.0 == out2[0] and rel_err(out2[1].cpu().numpy(), st.cpu().numpy()) <= TOL
    with pytest.raises(ValueError):
        model.convergence(0.0, dev(s0), None, nodes, dim_node_label, type_mask, adjacency, None, False)


# ----------------------------------------------------------------------------------------------------------------------
# training at large M: the row-streaming kernels of kernels_train_big.hpp
# ----------------------------------------------------------------------------------------------------------------------
from test_gpu_training import prefetch_oracle


@pytest.mark.parametrize('d,bn,mode,thr', [(64, True, 'average', 0.0), (32, True, 'sum', 0.0), (16, False, 'average', 0.0), (32, False, 'average', -1.0)])
@prefetch_oracle
def test_large_graph_training_step_matches_autograd(d, bn, mode, thr):
    """From 32 768 nodes `gnn_train_step` runs an iteration on k_aggregate_stats (neighbour sum + its BatchNorm statistics),
    k_train_fwd_b6 (rows straight into the matrix cores, statistics folded into the weights, predicate and the next iteration's
    statistics in the epilogue) and k_train_bwd_dx_b6 (dZ . W^T with the BatchNorm input gradient and the 'average' row scale in the
    epilogue, unit-weight transposed aggregate): every gradient against torch autograd in float64, and against the Python
    building-block orchestration (which keeps the general kernels)."""
    from test_gpu_training import nets, check_step
    rng = np.random.default_rng(d)
    N = 40_000
    g = er_graph(N, 6 * N, seed=5, aggregation_mode=mode)
    om = rng.random(N) < 0.6
    t = np.zeros((int(om.sum()), 2)); t[np.arange(len(t)), rng.integers(0, 2, len(t))] = 1
    g = GraphObject(g.nodes, g.arcs, t, focus='n', set_mask=rng.random(N) < 0.9, output_mask=om, aggregation_mode=mode,
                    sample_weight=rng.uniform(0.5, 1.5, len(t)))
    seq = MultiGraphSequencer([g], 'n', mode, 1, shuffle=False)
    x, y, sw = seq[0]
    ns, no = nets('n', d, bn, scale=(0.5 if thr >= 0 else 0.1) if mode == 'average' else 0.08)      # (early exit: a contractive network)
    s0 = rng.normal(0, 0.1, (N, d)).astype(np.float32)
    key = ('large_graph_step', d, bn, mode, thr)              # (the inputs are seeded: the alternative-kernel tests re-run a configuration on its oracle result)
    if thr < 0:                                               # early exit: a threshold at which the oracle stops after 1 .. 3 iterations
        from test_gpu_training import oracle_step, cached_oracle

        def search():
            seen = {}
            for th in (0.05, 0.1, 0.2, 0.4, 0.8):
                k = seen[th] = oracle_step(GNNnodeBased(ns, no, d, 4, th), x, y, sw, s0, 'categorical_crossentropy')['k']
                if 0 < k < 4: return th
            raise AssertionError(f'no threshold with an early exit found: {seen}')
        thr = cached_oracle((key, 'thr'), search)
    model = GNNnodeBased(ns, no, d, 4, thr)
    res, want = check_step(model, x, y, sw, s0, oracle_key=key)      # both orchestrations against the oracle


def test_small_graph_training_on_the_large_graph_kernels(mutag_graphs, monkeypatch):
    """GNN_TRAIN_BIG_MIN_NODES=0 (read at every call) sends the eligible models of the gradient tests - MUTAG batches, all three foci, with
    and without BatchNormalization, the Adam step, fit(), inference afterwards - through the large-graph kernels (ragged tiny row counts)."""
    import test_gpu_training as T
    monkeypatch.setenv('GNN_TRAIN_BIG_MIN_NODES', '0')
    for focus, bn in (('g', True), ('n', False), ('a', True)): T.test_gradients_single_layer(mutag_graphs, focus, bn)
    T.test_adam_step_matches_reference_formula(mutag_graphs)
    T.test_fit_reduces_loss_starter_config(mutag_graphs, True)
    T.test_inference_after_training_matches_oracle(mutag_graphs)


# ----------------------------------------------------------------------------------------------------------------------
# training on small graphs: the persistent kernels of kernels_train_small.hpp (one launch for the K forward iterations, one for the
# k backward iterations)
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('focus,d,bn,mode,n_graphs,thr', [
    ('g', 32, True, 'average', 60, 0.0), ('g', 64, True, 'average', 188, 0.0), ('n', 16, False, 'sum', 40, 0.0),
    ('a', 32, True, 'normalized', 24, 0.0), ('n', 64, False, 'average', 7, 0.0), ('g', 32, False, 'average', 50, -1.0),
    ('n', 32, True, 'sum', 1, 0.0), ('g', 16, True, 'average', 100, -1.0),
    # state widths that are not 16 / 32 / 64 run the next wider kernels on a padded tape: the starter configuration (state = the 14
    # label columns, state_vect_dim = 0), 20 -> 32, 40 -> 64, 5 -> 16
    ('g', 0, True, 'average', 64, 0.0), ('n', 20, True, 'average', 30, 0.0), ('a', 40, False, 'sum', 20, 0.0), ('g', 5, True, 'average', 40, -1.0),
    ('n', 0, False, 'normalized', 25, 0.0)])
@pytest.mark.parametrize('tiled', [True, False])
def test_small_graph_training_persistent_kernels_match_autograd(mutag_graphs, focus, d, bn, mode, n_graphs, thr, tiled, monkeypatch):
    """A merged MUTAG batch (18 .. 3 400 nodes: 1 .. 54 workgroups, the last tile ragged) through `gnn_train_step`: state widths
    16 / 32 / 64, with and without BatchNormalization, per-arc weights ('normalized') and per-row scales ('average'), early exit:
    k, loss, predictions, every gradient and the moving statistics against torch autograd in float64 - and against the Python
    building-block orchestration, which keeps the general kernels.  `tiled`: the graphs of the batch packed into tiles of <= 64
    nodes (state in LDS, one barrier per iteration) or tiles of 64 consecutive nodes whatever the graphs (rows exchanged through
    memory, two barriers)."""
    from test_gpu_training import nets, check_step, refocus, oracle_step, CLS
    from gnnkeras_amd.Models.training import LoopTrainer
    monkeypatch.setattr(LoopTrainer, 'use_tiles', tiled)
    rng = np.random.default_rng(100 + d + n_graphs)
    pool = [g for g in mutag_graphs if g.nodes.shape[0] <= 64] if tiled else mutag_graphs      # (the data set has graphs of up to 417 nodes)
    gl = refocus([g.copy() for g in pool[:n_graphs]], focus, rng)
    seq = MultiGraphSequencer(gl, focus, mode, n_graphs, shuffle=False)
    x, y, sw = seq[0]
    contractive = thr < 0
    ns, no = nets(focus, d, bn, scale=(0.15 if contractive else 0.5) if mode != 'sum' else 0.2)
    s0 = rng.normal(0, 0.1, (x[0].shape[0], d)).astype(np.float32) if d > 0 else None
    K = 7
    if contractive:
        seen = {}
        for thr in (0.02, 0.05, 0.1, 0.2, 0.4, 0.8):
            k = seen[thr] = oracle_step(CLS[focus](ns, no, d, K, thr), x, y, sw, s0, 'categorical_crossentropy')['k']
            if 1 < k < K: break
        assert 1 < k < K, f'no threshold with an early exit found: {seen}'
    model = CLS[focus](ns, no, d, K, thr)
    res, want = check_step(model, x, y, sw, s0, avg=(n_graphs % 2 == 0))
    tiles = x[5].matrix.tiles(64) if hasattr(x[5], 'matrix') else None
    if tiled: assert tiles is not None and tiles[-1] == x[0].shape[0] and int(np.diff(tiles).max()) <= 64


def test_tiles_with_an_arc_that_leaves_its_tile_fail_loudly(mutag_graphs):
    """`tile_node_begin` is a promise (no arc joins two tiles): the forward kernel checks every arc it walks and the call fails."""
    from test_gpu_training import nets
    from gnnkeras_amd.Models.training import LoopTrainer
    from gnnkeras_amd.Models.training import SGD
    seq = MultiGraphSequencer([g for g in mutag_graphs if g.nodes.shape[0] <= 64][:20], 'g', 'average', 20, shuffle=False)
    x, y, sw = seq[0]
    ns, no = nets('g', 32, True)
    model = GNNgraphBased(ns, no, 32, 4, 0.0)
    model.compile(optimizer=SGD(0.0), loss='categorical_crossentropy')
    adj = x[5].matrix
    good = adj.tiles(64)
    assert good is not None
    adj.__dict__['_tiles'][64] = np.asarray([0] + [int(t) + 1 for t in good[1:-1]] + [int(good[-1])], dtype=np.int32)     # cuts moved INTO graphs
    try:
        with pytest.raises(RuntimeError, match='leaves its tile'):
            LoopTrainer(model).train_step(x, y, sw, apply=False, seed=1)
    finally:
        adj.__dict__['_tiles'][64] = good
    LoopTrainer(model).train_step(x, y, sw, apply=False, seed=1)


def test_small_graph_training_with_the_persistent_kernels_switched_off(mutag_graphs, monkeypatch):
    """GNN_TRAIN_SMALL=0 keeps the per-iteration launches of round 2 (the path wide / deep state networks still take): the same
    gradient tests pass on it."""
    import test_gpu_training as T
    monkeypatch.setenv('GNN_TRAIN_SMALL', '0')
    for focus, bn in (('g', True), ('n', True), ('a', False)): T.test_gradients_single_layer(mutag_graphs, focus, bn)
    T.test_fit_reduces_loss_starter_config(mutag_graphs, False)


# ----------------------------------------------------------------------------------------------------------------------
# state networks with two or more hidden layers: the first two Dense layers fused with the aggregate (iteration_prefix)
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,d,hidden,mode,thr', [(40_000, 64, [48, 64], 'average', 0.0), (30_000, 32, [32, 20, 24], 'sum', 0.0),
                                                 (40_000, 64, [64, 33], 'normalized', 0.0), (40_000, 64, [40, 56], 'average', -1.0),
                                                 (935, 24, [30, 17], 'average', 0.0)])
def test_deep_state_networks_keep_the_aggregate_fused_with_the_first_two_layers(mutag_graphs, N, d, hidden, mode, thr):
    """`MLP(hidden_units=[h1, h2, ..])` (reference MLP.py:83-139) as the state network: the wave-specialised kernel's two-layer form
    runs the aggregate, Dense 1 and Dense 2 and writes the SECOND hidden layer; the remaining layers are dense launches, the last one
    carrying the predicate.  k, state and output against the fp64 oracle, and against the un-fused path (aggregate + one dense launch
    per layer), on ER graphs with per-row and per-arc weights, with an early exit, and on a MUTAG batch."""
    from test_gpu_parity import starter_nets
    rng = np.random.default_rng(N + d)
    if N == 935:
        seq = MultiGraphSequencer(mutag_graphs[:32], 'g', mode, 32, shuffle=False)
        focus, cls = 'g', GNNgraphBased
    else:
        g = er_graph(N, 6 * N, seed=3, aggregation_mode=mode)
        seq = MultiGraphSequencer([g], 'n', mode, 1, shuffle=False)
        focus, cls = 'n', GNNnodeBased
    x = seq[0][0]
    n_nodes = x[0].shape[0]
    ns, no = starter_nets(focus, d, hidden_state=hidden, act='tanh', scale=0.3 if thr >= 0 else 0.12)
    s0 = rng.normal(0, 0.1, (n_nodes, d)).astype(np.float32)
    K = 6
    if thr < 0:
        seen = {}
        for thr in (0.01, 0.02, 0.05, 0.1, 0.2, 0.4):
            k = seen[thr] = float(oracle_loop(cls(ns, no, d, K, thr), x, s0, np.float64)[0])
            if 1 < k < K: break
        assert 1 < k < K, seen
    model = cls(ns, no, d, K, thr)
    k64, st64, o64 = oracle_loop(model, x, s0, np.float64)
    inputs = model.process_inputs(x)
    got = {}
    for flags in (0, nat.FLAG_UNFUSED):
        model.native_flags = flags
        k, st, o = model.Loop(*inputs, state0=dev(s0))
        torch.cuda.synchronize()
        if flags == 0: assert 'remaining layers' in _last_kernel(), _last_kernel()
        else: assert 'un-fused' in _last_kernel(), _last_kernel()
        assert float(k) == float(k64), (flags, float(k), k64)
        assert rel_err(st.cpu().numpy(), st64) <= TOL and rel_err(o.cpu().numpy(), o64) <= TOL, flags
        got[flags] = st
    assert rel_err(got[0].cpu().numpy(), got[nat.FLAG_UNFUSED].cpu().numpy()) <= TOL


# ----------------------------------------------------------------------------------------------------------------------
# label aggregates of a large graph: the whole CSR row in flight (k_aggregate_narrow)
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F,ldx,weights', [(14, 14, 'rows'), (3, 5, 'rows'), (1, 1, 'arcs'), (16, 20, 'arcs'), (7, 7, 'ones'), (2, 2, 'arcs')])
def test_narrow_aggregate_of_a_large_graph_matches_adjoint_spmm(F, ldx, weights):
    """`gnn_aggregate` (reference `tf.sparse.sparse_dense_matmul(A, X, adjoint_a=True)`, GNN.py:254, :258) from 4 096 destination rows
    with at most 16 columns: empty rows, rows of more than 16 arcs (several trips), a 300-arc row, strided X (the arc-label columns of
    the arcs matrix), per-arc weights / one scale per row / all-ones - against the float64 product and, bit for bit, against the
    general kernel (same arc-order sums) on a graph below the size threshold made of the same rows."""
    import ctypes as C
    from gnnkeras_amd.sparse import SparseMatrix
    rng = np.random.default_rng(F * 10 + ldx)
    n_src, n_dst = 30_000, 9_000
    deg = rng.poisson(9, n_dst); deg[::97] = 0; deg[5] = 300; deg[77] = 40
    dst = np.repeat(np.arange(n_dst), deg)
    src = rng.integers(0, n_src, len(dst))
    idx = np.unique(np.stack([src, dst], 1), axis=0)
    if weights == 'arcs': val = rng.normal(size=len(idx)).astype(np.float32)
    elif weights == 'rows': val = (1.0 / np.maximum(np.bincount(idx[:, 1], minlength=n_dst), 1))[idx[:, 1]].astype(np.float32)
    else: val = np.ones(len(idx), np.float32)
    Xfull = rng.normal(size=(n_src, ldx)).astype(np.float32)
    X = Xfull[:, ldx - F:]                                       # the last F columns of a wider matrix (ld = ldx)
    want = O.sparse_dense_matmul_adjoint(idx, val, (n_src, n_dst), np.ascontiguousarray(X), np.float64)

    def run(index, values, nd):
        m = SparseMatrix(index, values, (n_src, nd))
        c = m.device_csr('cuda')
        assert (c['w'] is not None) == (weights == 'arcs')
        Xd = dev(Xfull)
        out = torch.zeros((nd, F), dtype=torch.float32, device='cuda')
        csr = nat.make_csr(c)
        nat.check(nat.lib().gnn_aggregate(C.byref(csr), C.c_void_p(Xd.data_ptr() + 4 * (ldx - F)), ldx, F, nat.ptr(out), F, nat.current_stream(Xd.device)))
        torch.cuda.synchronize()
        return out.cpu().numpy()

    got = run(idx, val, n_dst)
    assert rel_err(got, want) <= TOL
    keep = idx[:, 1] < 3000                                      # below 4 096 rows: the general kernel, same rows
    small = run(idx[keep], val[keep], 3000)
    assert np.array_equal(small, got[:3000])


@pytest.mark.parametrize('max_iteration,ones', [(1, False), (5, True), (3, False)])
def test_small_graph_training_edge_iteration_counts(mutag_graphs, max_iteration, ones):
    """The persistent training kernels at the ends of the iteration range: one iteration (no barrier between iterations ever taken),
    and state_0 = ones with threshold 0 - the reference's `state_old = ones_like(state)` makes the very first condition false, k = 0,
    the loop body never runs, the state network gets zero gradients and the output network trains on state_0."""
    from test_gpu_training import nets, check_step
    rng = np.random.default_rng(max_iteration)
    seq = MultiGraphSequencer(mutag_graphs[:20], 'g', 'average', 20, shuffle=False)
    x, y, sw = seq[0]
    d = 32
    ns, no = nets('g', d, True)
    model = GNNgraphBased(ns, no, d, max_iteration, 0.0)
    n = x[0].shape[0]
    s0 = np.ones((n, d), np.float32) if ones else rng.normal(0, 0.1, (n, d)).astype(np.float32)
    res, want = check_step(model, x, y, sw, s0)
    assert res['k'] == (0 if ones else max_iteration)


@pytest.mark.parametrize('tiled', [True, False])
def test_small_graph_training_is_bitwise_reproducible(mutag_graphs, tiled, monkeypatch):
    """Every cross-tile sum of the persistent training kernels runs in a fixed order (partials in workgroup order, arcs in CSR
    order, the waves' shares in wave order): two runs of the same step give the same bits - loss, predictions, every gradient."""
    from test_gpu_training import nets
    from gnnkeras_amd.Models.training import LoopTrainer, SGD
    monkeypatch.setattr(LoopTrainer, 'use_tiles', tiled)
    pool = [g for g in mutag_graphs if g.nodes.shape[0] <= 64] if tiled else mutag_graphs
    seq = MultiGraphSequencer(pool[:48], 'g', 'average', 48, shuffle=False)
    x, y, sw = seq[0]
    ns, no = nets('g', 32, True)
    model = GNNgraphBased(ns, no, 32, 12, 0.0)
    model.compile(optimizer=SGD(0.0), loss='categorical_crossentropy')
    s0 = torch.from_numpy(np.random.default_rng(3).normal(0, 0.1, (x[0].shape[0], 32)).astype(np.float32)).cuda()
    runs = []
    for rep in range(3):
        tr = LoopTrainer(model)
        res = tr.train_step(x, y, sw, state0=s0, apply=False)
        torch.cuda.synchronize()
        runs.append([res['loss'].clone(), res['y_pred'].clone()] + [g.clone() for g in tr.gs.gradients() + tr.go.gradients()])
        w = model.net_state.get_weights() + model.net_output.get_weights()       # (the step moved the BN moving statistics: restore)
        if rep == 0: w0 = [a.copy() for a in w]
        model.net_state.set_weights(w0[:len(model.net_state.get_weights())]); model.net_output.set_weights(w0[len(model.net_state.get_weights()):])
    for other in runs[1:]:
        for a, b in zip(runs[0], other): assert torch.equal(a, b)


# ----------------------------------------------------------------------------------------------------------------------
# arc- and graph-focused models on shards: the device pieces (emulated ranks on one GPU; the collectives run in tests/test_distributed.py)
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('focus,d', [('a', 32), ('g', 32), ('a', 0), ('g', 0)])
def test_arc_and_graph_focused_shards_on_the_device(focus, d):
    """Reference GNN.py:317-330 / :341-346 on node-range shards: 3 emulated ranks, the real shard kernels for the loop, then per rank
    the arc-shaped output network over the masked arcs it owns (sources read from the exchanged buffer) or the per-graph partial sums
    of its nodes' outputs; assembled / added, they are the oracle's output on the whole graph."""
    from gnnkeras_amd.distributed import ShardedLoop, GraphSlice, partition
    from gnnkeras_amd.Models.GNN import GNNarcBased
    from test_gpu_parity import starter_nets
    rng = np.random.default_rng(5)
    R, K = 3, 5
    if focus == 'a':
        g0 = er_graph(5003, 30000, seed=7)
        E = g0.arcs.shape[0]
        om = rng.random(E) < 0.6
        sm = rng.random(E) < 0.9
        g = GraphObject(g0.nodes, g0.arcs, rng.normal(size=(int(om.sum()), 2)), focus='a', set_mask=sm, output_mask=om,
                        aggregation_mode='average')
        cls = GNNarcBased
    else:
        parts = [er_graph(n, 6 * n, seed=11 + n) for n in (1400, 2071, 523, 1009)]
        parts = [GraphObject(q.nodes, q.arcs, rng.normal(size=(1, 2)), focus='g', aggregation_mode='average') for q in parts]
        g = GraphObject.merge(parts, focus='g', aggregation_mode='average')
        cls = GNNgraphBased
    N = g.nodes.shape[0]
    ns, no = starter_nets(focus, d, scale=0.3, act='tanh')
    model = cls(ns, no, d, K, 0.0)
    s0 = rng.normal(0, 0.1, (N, d)).astype(np.float32) if d else None
    x = MultiGraphSequencer([g], focus, 'average', 1, shuffle=False)[0][0]
    k64, st64, o64 = oracle_loop(model, x, s0, np.float64)
    shards = [ShardedLoop(model, GraphSlice.from_graph(g, lo, hi, focus=focus), r, R, 'cuda') for r, (lo, hi) in enumerate(partition(N, R)[1])]
    for sl in shards:
        if d: sl._load_state0(torch.from_numpy(s0).cuda())
        else: sl._load_state0(sl.plan_nodes_as_state())
        sl._setup(); sl._initial_flags()
    n = shards[0].plan.rows_per_slice * shards[0].SP
    for it in range(K):
        for sl in shards: sl._iteration(it)
        for r, src in enumerate(shards):
            piece = src.buf[(it + 1) & 1].view(-1)[r * n:(r + 1) * n]
            for dst in shards:
                if dst is not src: dst.buf[(it + 1) & 1].view(-1)[r * n:(r + 1) * n].copy_(piece)
    outs = [sl._output() for sl in shards]
    assert all(float(o[0]) == float(k64) for o in outs)
    assert rel_err(np.concatenate([o[1].cpu().numpy() for o in outs]), st64) <= TOL
    if focus == 'g':
        pooled = sum(sl._pool(o[2]) for sl, o in zip(shards, outs)).cpu().numpy()
        assert pooled.shape == o64.shape and rel_err(pooled, o64) <= TOL
    else:
        mask = np.flatnonzero(g.set_mask & g.output_mask)
        out = np.full(o64.shape, np.nan, dtype=np.float32)
        for sl, o in zip(shards, outs): out[np.searchsorted(mask, sl.plan.arc_out_index)] = sl._arc_outputs(float(o[0])).cpu().numpy()
        assert rel_err(out, o64) <= TOL


@pytest.mark.parametrize('M,K,ldx,H,act,bias', [(131072, 64, 64, 64, 'selu', True), (70001, 48, 52, 24, 'tanh', True), (40000, 8, 8, 64, 'relu', False),
                                              (100003, 20, 64, 12, 'linear', True), (65536, 64, 68, 40, 'sigmoid', True)])
def test_row_streaming_dense_layer_matches_float64(M, K, ldx, H, act, bias):
    """`gnn_dense` over ONE contiguous matrix at large M runs k_rowdense (rows straight into the matrix cores): ragged last tile, leading
    dimensions above the width, widths that are not multiples of 16, no bias - against the float64 product."""
    from gnnkeras_amd.Models.training import _Prim
    rng = np.random.default_rng(M + K)
    p = _Prim(torch.device('cuda'))
    x = dev(rng.normal(0, 1, (M, ldx)).astype(np.float32))[:, :K]
    W = dev(rng.normal(0, 0.3, (K, H)).astype(np.float32))
    b = dev(rng.normal(0, 0.3, H).astype(np.float32)) if bias else None
    Y = torch.full((M, H), float('nan'), dtype=torch.float32, device='cuda')
    p.dense([(x, None)], W, H, b, nat.ACTIVATIONS[act], Y)
    torch.cuda.synchronize()
    z = x.double() @ W.double() + (b.double() if bias else 0.0)
    want = {'selu': torch.nn.functional.selu, 'linear': lambda t: t, 'tanh': torch.tanh, 'relu': torch.relu, 'sigmoid': torch.sigmoid}[act](z)
    assert float((Y.double() - want).abs().max() / want.abs().max()) <= 1e-5


@pytest.mark.parametrize('N,d,hidden,mode', [(40_000, 200, None, 'average'), (36_000, 132, None, 'sum'), (40_000, 96, [96], 'average'),
                                             (33_000, 160, [72], 'normalized'), (34_000, 300, None, 'average')])
def test_wide_layers_of_the_unfused_path_at_scale(N, d, hidden, mode):
    """Two-layer networks between 65 and 128, and everything above 256 (or with GNN_FLAG_UNFUSED), take the un-fused path; from 32 768
    rows its dense layers run k_rowdense_wide / k_rowdense (rows straight into the matrix cores, output columns in passes of 64): k,
    state and output against the fp64 oracle."""
    from test_gpu_parity import starter_nets
    rng = np.random.default_rng(d)
    g = er_graph(N, 5 * N, seed=9, aggregation_mode=mode)
    seq = MultiGraphSequencer([g], 'n', mode, 1, shuffle=False)
    x = seq[0][0]
    ns, no = starter_nets('n', d, hidden_state=hidden, act='tanh', scale=0.2 if mode != 'sum' else 0.02)
    model = GNNnodeBased(ns, no, d, 4, 0.0)
    if hidden is None and d <= 256: model.native_flags = nat.FLAG_UNFUSED       # (these widths have a fused kernel of their own now)
    s0 = rng.normal(0, 0.1, (N, d)).astype(np.float32)
    k64, st64, o64 = oracle_loop(model, x, s0, np.float64)
    k, st, o = model.Loop(*model.process_inputs(x), state0=dev(s0))
    torch.cuda.synchronize()
    assert 'un-fused' in _last_kernel(), _last_kernel()
    assert float(k) == float(k64)
    assert rel_err(st.cpu().numpy(), st64) <= TOL and rel_err(o.cpu().numpy(), o64) <= TOL


# ----------------------------------------------------------------------------------------------------------------------
# state widths 129 .. 256: gathered rows in LDS, weights streamed from L2 in fragment order (kernel_state_xwide.hpp)
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,arcs_per_node,d,mode,act,thr', [(40_000, 5, 200, 'average', 'tanh', 0.0), (5_003, 6, 130, 'sum', 'tanh', 0.0),
                                                            (3_000, 40, 256, 'normalized', 'selu', 0.0), (20_011, 8, 160, 'average', 'tanh', -1.0),
                                                            (17, 3, 129, 'average', 'sigmoid', 0.0), (9_000, 20, 224, 'sum', 'relu', 0.0),
                                                            (33, 2, 192, 'normalized', 'tanh', 0.0)])
def test_state_widths_129_to_256_run_fused(N, arcs_per_node, d, mode, act, thr):
    """`state_vect_dim` between 129 and 256 (reference GNN.py:26-28 allows any width): one launch per iteration (k_state_xwide_b3: the Dense
    layer as six bf16 products of three-term splits, kernel_state_xwide.hpp) - k, state and output against the fp64 oracle and against the
    un-fused path; row counts that are not multiples of the 32-row tile, in-degrees above 16 (the gather's second chunk), per-row and
    per-arc weights, widths that are not multiples of 32 / 8, an activation with f(0) != 0 (pad columns must stay zero), an early exit."""
    from test_gpu_parity import starter_nets
    rng = np.random.default_rng(N + d)
    g = er_graph(N, arcs_per_node * N, seed=5, aggregation_mode=mode)
    seq = MultiGraphSequencer([g], 'n', mode, 1, shuffle=False)
    x = seq[0][0]
    scale = {'sum': 0.1 / arcs_per_node, 'average': 0.2, 'normalized': 0.2}[mode] * (0.5 if thr < 0 else 1.0)
    ns, no = starter_nets('n', d, act=act, scale=scale)
    s0 = rng.normal(0, 0.1, (N, d)).astype(np.float32)
    K = 5
    if thr < 0:
        seen = {}
        for thr in (0.005, 0.01, 0.02, 0.05, 0.1, 0.2, 0.4):
            k = seen[thr] = float(oracle_loop(GNNnodeBased(ns, no, d, K, thr), x, s0, np.float64)[0])
            if 1 < k < K: break
        assert 1 < k < K, seen
    model = GNNnodeBased(ns, no, d, K, thr)
    k64, st64, o64 = oracle_loop(model, x, s0, np.float64)
    inputs = model.process_inputs(x)
    got = {}
    for flags in (0, nat.FLAG_UNFUSED):
        model.native_flags = flags
        k, st, o = model.Loop(*inputs, state0=dev(s0))
        torch.cuda.synchronize()
        assert ('k_state_xwide_b3' if flags == 0 else 'un-fused') in _last_kernel(), _last_kernel()
        assert float(k) == float(k64), (flags, float(k), k64)
        assert rel_err(st.cpu().numpy(), st64) <= TOL and rel_err(o.cpu().numpy(), o64) <= TOL, flags
        got[flags] = st
    assert rel_err(got[0].cpu().numpy(), got[nat.FLAG_UNFUSED].cpu().numpy()) <= TOL


def test_state_width_200_is_bitwise_reproducible():
    """The LDS hand-overs of k_state_xwide (rows deposited / waves done / rounds freed) carry no arithmetic: the neighbour sum runs in
    arc order, the predicate's row shares are added in block order - five runs of the same loop must agree bit for bit."""
    from test_gpu_parity import starter_nets
    N, d = 30_000, 200
    g = er_graph(N, 8 * N, seed=2, aggregation_mode='average')
    x = MultiGraphSequencer([g], 'n', 'average', 1, shuffle=False)[0][0]
    ns, no = starter_nets('n', d, act='tanh', scale=0.2)
    model = GNNnodeBased(ns, no, d, 8, 0.001)
    inputs = model.process_inputs(x)
    s0 = dev(np.random.default_rng(0).normal(0, 0.1, (N, d)).astype(np.float32))
    ref = None
    for rep in range(5):
        k, st, o = model.Loop(*inputs, state0=s0)
        torch.cuda.synchronize()
        assert 'k_state_xwide' in _last_kernel()
        if ref is None: ref = (float(k), st.clone(), o.clone())
        else: assert float(k) == ref[0] and torch.equal(st, ref[1]) and torch.equal(o, ref[2]), rep


# ----------------------------------------------------------------------------------------------------------------------
# a softmax as the state network's last activation (reference MLP.py:12-78 takes any Keras activation)
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,d,hidden,mode', [(40_000, 64, None, 'average'), (5_003, 32, None, 'sum'), (40_000, 64, [48], 'normalized'),
                                             (935, 16, None, 'average'), (3_001, 24, [20], 'average')])
def test_softmax_state_activation_runs_fused(mutag_graphs, N, d, hidden, mode):
    """The wave-specialised kernel's row-major epilogue holds whole rows in one lane group: a softmax state (one- and two-layer state
    networks, widths up to 64, any graph size - the kernel is chosen whatever the size heuristics say) stays one launch per iteration.
    k, state and output against the fp64 oracle and the un-fused path (dense + k_softmax_rows)."""
    rng = np.random.default_rng(N + d)
    if N == 935:
        seq = MultiGraphSequencer(mutag_graphs[:32], 'g', mode, 32, shuffle=False)
        focus, cls = 'g', GNNgraphBased
    else:
        g = er_graph(N, 6 * N, seed=4, aggregation_mode=mode)
        seq = MultiGraphSequencer([g], 'n', mode, 1, shuffle=False)
        focus, cls = 'n', GNNnodeBased
    x = seq[0][0]
    n_nodes = x[0].shape[0]
    inp, lay = get_inout_dims('state', 14, 3, 2, focus, d, hidden_units=hidden)
    ns = MLP(inp[0], lay, ['tanh'] * (len(lay) - 1) + ['softmax'], 'lecun_normal', 'lecun_normal', rng=0, batch_normalization=True)
    inp, lay = get_inout_dims('output', 14, 3, 2, focus, d)
    no = MLP(inp[0], lay, 'softmax', 'glorot_normal', 'glorot_normal', rng=1)
    s0 = np.abs(rng.normal(0, 0.1, (n_nodes, d))).astype(np.float32)
    model = cls(ns, no, d, 5, 0.0)
    k64, st64, o64 = oracle_loop(model, x, s0, np.float64)
    inputs = model.process_inputs(x)
    got = {}
    for flags in (0, nat.FLAG_UNFUSED):
        model.native_flags = flags
        k, st, o = model.Loop(*inputs, state0=dev(s0))
        torch.cuda.synchronize()
        assert ('k_state_fused4' if flags == 0 else 'un-fused') in _last_kernel(), _last_kernel()
        assert float(k) == float(k64), (flags, float(k), k64)
        assert rel_err(st.cpu().numpy(), st64) <= TOL and rel_err(o.cpu().numpy(), o64) <= TOL, flags
        got[flags] = st
    assert abs(float(got[0].sum(1).mean()) - 1.0) < 1e-5          # rows of a softmax state sum to one
    assert rel_err(got[0].cpu().numpy(), got[nat.FLAG_UNFUSED].cpu().numpy()) <= TOL


def test_standalone_convergence_step_at_state_width_200():
    """`convergence()` (reference GNN.py:217-236; `gnn_state_step`) at a width the 129..256 kernel serves: one step against the fp64
    oracle's step and against the un-fused path."""
    from test_gpu_parity import starter_nets
    N, d = 4_099, 200
    g = er_graph(N, 7 * N, seed=6, aggregation_mode='average')
    x = MultiGraphSequencer([g], 'n', 'average', 1, shuffle=False)[0][0]
    ns, no = starter_nets('n', d, act='tanh', scale=0.3)
    model = GNNnodeBased(ns, no, d, 5, 0.0)
    nodes, arcs, _, _, _, adj, an, ng = model.process_inputs(x)
    s = np.random.default_rng(0).normal(0, .1, (N, d)).astype(np.float32)
    a = (adj.indices, adj.values, np.array(adj.shape))
    agg_nodes = O.sparse_dense_matmul_adjoint(*a, nodes.cpu().numpy(), np.float64)
    agg_arcs = O.sparse_dense_matmul_adjoint(an.indices, an.values, np.array(an.shape), arcs.cpu().numpy()[:, 2:], np.float64)
    want = O.convergence(s.astype(np.float64), nodes.cpu().numpy().astype(np.float64), a, agg_nodes, agg_arcs, ns.spec(), d, False, np.float64)
    for flags in (0, nat.FLAG_UNFUSED):
        model.native_flags = flags
        k1, new, old, *_ = model.convergence(0, dev(s), None, nodes, adj, None, None, False, arcs=arcs, arcnode=an)
        torch.cuda.synchronize()
        assert ('k_state_xwide' if flags == 0 else 'un-fused') in _last_kernel(), _last_kernel()
        assert k1 == 1 and rel_err(new.cpu().numpy(), want) <= TOL, flags
