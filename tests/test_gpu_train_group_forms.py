"""Every instantiation of the two grouped training-forward kernels (gnnkeras_amd/csrc/kernels_train_group.hpp `k_train_group_fwd<SQ, HAS_W>`,
kernels_train_group_types.hpp `k_train_group_fwd_types<SQ, HAS_W>`), one case each: model kind x padded state width 16 / 32 / 64 (state
widths 6 / 20 / 40: pad columns in every form) x an adjacency with and without per-arc weights.  A case is ONE grouped call over four
Erdos-Renyi graphs - one tile, a full tile, one row into a second tile, several tiles - against `oracle.torch_train.lgnn_serial_propagate`
graph by graph, held to the bar of tests/test_gpu_lgnn_grouped.py: max(BAR, 2 x float32-oracle distance) per graph, the moving statistics
through `check_moving`.  BatchNormalization on, threshold 0 and max_iteration 3: k = 3 for every graph, no case can be borderline.

Per-arc weights are put on the merged batch's Adjacency (the operand the kernels gather with) and, cut per graph, on the oracle's
operands; the constants keep the 'average' ArcNode."""
import numpy as np
import pytest
import torch

from gnnkeras_amd import CompositeGraphObject
from gnnkeras_amd.Models.MLP import MLP, get_inout_dims
from gnnkeras_amd.Models.GNN import GNNnodeBased
from gnnkeras_amd.Models.training import LoopTrainer
from gnnkeras_amd.Sequencers.GraphSequencers import MultiGraphSequencer, CompositeMultiGraphSequencer
from gnnkeras_amd.sparse import SparseMatrix, SparseTriple
from gnnkeras_amd.synth import er_graph
from oracle import torch_train
from oracle.harness import rel_err
from test_gpu_training import log_rows
from test_gpu_lgnn_serial import BAR, operands, oracle_layer, check_moving, kernel_name, perturb_bn
from test_gpu_lgnn_grouped import GROUPED
from test_gpu_composite_grouped import GROUPED_TYPES, DIMS, T, A, typed_graphs, comp_stack

pytestmark = pytest.mark.gpu
K = 3
L = 5                                                     # homogeneous label columns: 2 L + A = 13 constant input columns
SIZES = {'homogeneous': (20, 64, 65, 150), 'composite': (20, 64, 65, 250)}
CASES = [(kind, d, weighted) for kind in SIZES for d in (6, 20, 40) for weighted in (False, True)]


def _graphs(kind, rng):
    sizes = SIZES[kind]
    if kind == 'homogeneous':
        return [er_graph(n, int(rng.integers(n, 3 * n)), dim_node_label=L, dim_arc_label=A, dim_target=T, focus='n', aggregation_mode='average',
                         seed=700 + i) for i, n in enumerate(sizes)]
    graphs = typed_graphs(rng, sizes, 800, 'n', absent=1)          # graph 1: no row of type 2
    g = graphs[0]                                                    # graph 0: every row of type 0
    tm = np.zeros((g.nodes.shape[0], len(DIMS)), bool); tm[:, 0] = True
    graphs[0] = CompositeGraphObject(nodes=g.nodes, arcs=g.arcs, targets=g.targets, type_mask=tm, dim_node_label=DIMS, focus='n',
                                     set_mask=g.set_mask, output_mask=g.output_mask, aggregation_mode='average')
    for g in graphs: g.setAggregation('average')                     # one scale per destination row: no per-arc weights of its own
    per_type = [np.asarray(g.type_mask).reshape(g.nodes.shape[0], -1).sum(0) for g in graphs]
    assert per_type[0].tolist() == [sizes[0], 0, 0] and per_type[1][2] == 0 and per_type[1][:2].min() > 0
    assert per_type[3].max() > 64 and per_type[3].min() > 0       # a type with several tiles of its own
    return graphs


def _model(kind, d):
    if kind == 'composite': return comp_stack('n', d, 1, 0.0, max_it=K).gnns[0]
    wrng = np.random.default_rng(19)
    inp, lay = get_inout_dims('state', L, A, T, 'n', d)
    ns = MLP(inp[0], lay, 'selu', 'lecun_normal', 'lecun_normal', rng=10, batch_normalization=True)
    inp, lay = get_inout_dims('output', L, A, T, 'n', d)
    no = MLP(inp[0], lay, 'softmax', 'glorot_normal', 'glorot_normal', rng=20, batch_normalization=True)
    for n_ in (ns, no): perturb_bn(n_, wrng)
    return GNNnodeBased(ns, no, d, K, 0.0)


def build_case(kind, d, weighted):
    """(model, merged batch x, group table, per-graph oracle operands, per-graph state_0, graphs) of one case."""
    comp = kind == 'composite'
    rng = np.random.default_rng(1000 + 10 * d + int(comp))
    graphs = _graphs(kind, rng)
    seq_cls, adj_at = (CompositeMultiGraphSequencer, 7) if comp else (MultiGraphSequencer, 5)
    x = list(seq_cls(list(graphs), 'n', 'average', len(graphs), shuffle=False)[0][0])
    ops_ = operands(seq_cls(list(graphs), 'n', 'average', 1, shuffle=False), graphs, comp)
    begin = np.concatenate([[0], np.cumsum([g.nodes.shape[0] for g in graphs])])
    adj = x[adj_at].matrix
    assert adj.csr().w is None
    if weighted:
        idx = np.asarray(adj.indices)
        w = rng.uniform(0.2, 1.0, len(idx)).astype(np.float32) * np.asarray(adj.values)          # (the row's 1 / in-degree, times the arc's own weight)
        x[adj_at] = SparseTriple(SparseMatrix(idx, w, adj.dense_shape))
        assert x[adj_at].matrix.csr().w is not None
        for i, o in enumerate(ops_):
            own = (idx[:, 0] >= begin[i]) & (idx[:, 0] < begin[i + 1])
            assert np.all((idx[own, 1] >= begin[i]) & (idx[own, 1] < begin[i + 1])) and int(own.sum()) == len(o['adjacency'][1])
            assert np.array_equal(idx[own] - begin[i], o['adjacency'][0])
            o['adjacency'] = (idx[own] - begin[i], w[own], o['adjacency'][2])
    s0s = [rng.normal(0, 0.1, (g.nodes.shape[0], d)).astype(np.float32) for g in graphs]
    return _model(kind, d), x, begin, ops_, s0s, graphs


def run_case(kind, gnn, x, begin, s0s):
    """The ONE grouped library call of a case: (k, state, node-level output) as numpy."""
    state0 = torch.from_numpy(np.concatenate(s0s)).cuda()
    if kind == 'composite':
        if getattr(gnn, '_trainer', None) is None: gnn._trainer = LoopTrainer(gnn)
        k, state, out = gnn._trainer.forward_native(x, state0=state0, node_level=True, groups=begin)
    else:
        k, state, out = gnn.Loop(*gnn.process_inputs(x), training=True, groups=begin, state0=state0, node_level=True)
    assert kernel_name() == (GROUPED_TYPES if kind == 'composite' else GROUPED)
    return k.cpu().numpy(), state.cpu().numpy(), out.cpu().numpy()


@pytest.mark.parametrize('kind,d,weighted', CASES)
def test_every_form_of_the_grouped_forward_matches_the_float64_oracle(kind, d, weighted):
    gnn, x, begin, ops_, s0s, graphs = build_case(kind, d, weighted)
    layer, layer32 = oracle_layer(gnn), oracle_layer(gnn, torch.float32)
    want = torch_train.lgnn_serial_propagate(ops_, layer, focus='n', get_state=True, get_output=True, state0s=s0s)
    want32 = torch_train.lgnn_serial_propagate(ops_, layer32, focus='n', get_state=True, get_output=True, state0s=s0s)
    assert want['k'] == [K] * len(graphs)
    k, state, out = run_case(kind, gnn, x, begin, s0s)
    assert [int(v) for v in k] == want['k'], (k, want['k'])
    S = d
    rows, o0 = [], 0
    for i, g in enumerate(graphs):
        mask = np.logical_and(np.asarray(g.set_mask).reshape(-1), np.asarray(g.output_mask).reshape(-1))
        w_out, w32_out = want['nodes'][i][:, S:S + T][mask], want32['nodes'][i][:, S:S + T][mask]
        assert len(w_out) > 0
        e32 = max(rel_err(want32['nodes'][i][:, :S], want['nodes'][i][:, :S]), rel_err(w32_out, w_out))
        bar = max(BAR, 2 * e32)
        e_state, e_out = rel_err(state[begin[i]:begin[i + 1]], want['nodes'][i][:, :S]), rel_err(out[o0:o0 + int(mask.sum())], w_out)
        o0 += int(mask.sum())
        rows.append(dict(graph=i, nodes=g.nodes.shape[0], state=e_state, out=e_out, float32_oracle=e32, bar=bar))
        print(f'{kind} d={d} weighted={weighted} graph {i}: {rows[-1]}')
        assert max(e_state, e_out) <= bar, (kind, d, weighted, i, e_state, e_out, bar)
    assert o0 == out.shape[0]
    moving = check_moving(gnn, want, f'group forms {kind} d={d} weighted={weighted}')
    log_rows(f'train_group_forms {kind} d={d} weighted={weighted}', rows + [dict(moving=moving)])
