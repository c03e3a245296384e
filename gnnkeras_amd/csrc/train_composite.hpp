// gnn_train_step for HETEROGENEOUS models (reference GNN/Models/CompositeGNN.py:275-304: `train_step` of CompositeGNNnodeBased /
// graphBased): one state network per node type, each applied to the rows of its type
//     state_new[type t rows] = net_state[t]([labels[:, :d_t] | state | Adj^T state | aggregated_component][type t rows], training=True)
// (CompositeGNN.py:215-234), BatchNormalization of network t on the batch statistics of ITS rows, moving averages updated once per
// executed iteration and network, the output network on the converged state alone (CompositeGNN.py:237-239), Keras loss, and
// back-propagation through the k executed iterations.
//
// The same arithmetic as the building blocks driven from Python (Models/training.py) with the orchestration inside the library (the general
// kernels of train_loop.hpp with per-type row lists: k_segdense / k_dense_grad_* / k_colstats_* take a row index per segment), one host
// synchronisation per step (to learn k).  Node, graph and arc focus (CompositeGNN.py:315-327: the output network over [state_src | state_dst
// | arc label] of the masked arcs).  The phases the step shares with the homogeneous one (argument checks, read_k, output head, loss, head
// backward, finish_step, ..) are train_loop.hpp's.  gnn_train_step_composite_ex (the end of this file) cuts the step into the two phases of
// gnn_train_step_ex, takes upstream gradients and leaves d loss / d nodes: what a joint CompositeLGNN step is made of.
#pragma once
// (included by gnnloop.hip behind train_loop.hpp: shares its anonymous-namespace helpers)
#include "train_composite_big.hpp"      // large graphs: the row-streaming kernels on per-type position ranges

namespace {

struct CType {                       // one node type
    const gnn_mlp_t *m;
    gnn_mlp_grads_t g;
    int count, d_t, in_dim, off_state, off_agg, off_comp;
    const int *rows;                 // device: node ids of this type, ascending
    NetCtx nc;
    float *stats, *stats_tpl;        // [K][2 in_dim], [2 in_dim]: mean | var per input column
    float *Wf, *bf;                  // [K][in_dim x H1], [K][H1]: folded first layers (thin first layers only)
    float *Gc, *dx;                  // [count, S] gathered gradient rows, [count, 2 S] d loss / d [state | agg] rows
};

struct CPlan : StepPlan {            // (train_loop.hpp: what the two kinds' plans share)
    int n_types, sum_d, W_comp;
    float *agg_comp, *dx_full;
    CType ty[GNN_MAX_TYPES];
    // small graphs: the K forward / k backward iterations as ONE persistent launch each (kernels_train_small.hpp), the nodes walked in type
    // order in tiles of <= 64 nodes of one type: the tape's rows are POSITIONS (position i = node type_nodes[i]), `inv` maps back
    int wg_begin[GNN_MAX_TYPES + 1];
    int *inv; float *sm_dxa, *sm_partW[GNN_MAX_TYPES], *sm_partBN[GNN_MAX_TYPES];
    // large graphs (train_composite_big.hpp): the tape's rows are POSITIONS too, every type a contiguous range of them
    CBig B;
};

// The BatchNormalization epsilon of the persistent launches, one for all their tiles: that of the first type WITH ROWS.  A type without rows does
// not count towards the path (composite_train_path) and may be the only one without BatchNormalization - its bn_eps is 0.
inline float composite_small_eps(const CPlan &p) {
    for (int q = 0; q < p.n_types; ++q) if (p.ty[q].count > 0) return p.ty[q].m->bn_eps;
    return p.ty[0].m->bn_eps;
}

// inv[perm[i]] = i
__global__ void __launch_bounds__(256) k_invert_perm(const int *__restrict__ perm, int n, int *__restrict__ inv) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) inv[perm[i]] = i;
}

// rows[m] of a [*, ld_dst] matrix <- row m of a compact [M, width] one (every node has exactly one type: the types' rows partition it)
__global__ void __launch_bounds__(256) k_scatter_rows(const float *__restrict__ src, int ld_src, const int *__restrict__ idx, int M, int width,
                                                      float *__restrict__ dst, int ld_dst) {
    const size_t total = (size_t)M * width;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t m = i / width;
        const int j = (int)(i % width);
        dst[(size_t)idx[m] * ld_dst + j] = src[m * ld_src + j];
    }
}

int scatter_rows(const float *src, int ld_src, const int *idx, int M, int width, float *dst, int ld_dst, hipStream_t st) {
    if (M == 0 || width == 0) return 0;
    k_scatter_rows<<<std::min(cdiv((long)M * width, 256), 256 * 16), 256, 0, st>>>(src, ld_src, idx, M, width, dst, ld_dst);
    LAUNCH_OK();
    return 0;
}

int gather_rows(const float *src, int ld_src, const int *idx, int M, int width, float *dst, int ld_dst, hipStream_t st) {
    if (M == 0 || width == 0) return 0;
    const long total = (long)M * ((width & 3) == 0 ? width / 4 : width);
    gnn::k_gather_rows<<<std::min(cdiv(total, 256), 256 * 16), 256, 0, st>>>(src, ld_src, idx, M, width, dst, ld_dst);
    LAUNCH_OK();
    return 0;
}

// Which path a composite step takes (dims, SPs, n_wg of `p` are set; the sibling of homogeneous_train_path, train_loop.hpp).  The
// persistent kernels: every state network one Dense layer of the state's width, every non-empty type with or every one without
// BatchNormalization - the tiles meet at the same grid barriers -, 1 .. 256 tiles, all resident at once.  The row-streaming kernels on type
// ranges: composite_big_applies (train_composite_big.hpp).  Else one launch per layer, type and iteration.
TrainPath composite_train_path(const gnn_train_args_t &ta, CPlan &p, bool drop_s) {
    const gnn_loop_args_t &a = ta.loop;
    bool uniform = true;
    int bn_seen = -1;
    float eps_seen = 0.0f;                             // (the launch has ONE epsilon for all its tiles: composite_small_eps)
    for (int t = 0; t < p.n_types; ++t) {
        const gnn_mlp_t &m = a.net_state[t];
        if (!one_dense_of_state_width(m, p.S)) uniform = false;
        if (a.type_offsets[t + 1] - a.type_offsets[t] <= 0) continue;
        if (bn_seen < 0) { bn_seen = m.has_bn ? 1 : 0; eps_seen = m.bn_eps; }
        else if (bn_seen != (m.has_bn ? 1 : 0) || (m.has_bn && m.bn_eps != eps_seen)) uniform = false;
    }
    if (uniform && train_small_fits(p, drop_s) && p.n_wg >= 1 && p.n_wg <= 256) return TrainPath::small;
    return !drop_s && composite_big_applies(ta, p.N, p.S, p.W_comp, &p.B.XT) ? TrainPath::big : TrainPath::general;
}

// the first half of make_cplan: the dims checked against the networks, the tiles, the path
int cplan_dims_and_path(const gnn_train_args_t &ta, void *ws, CPlan &p) {
    const gnn_loop_args_t &a = ta.loop;
    memset(&p, 0, sizeof(p));
    if (a.abi_version != GNN_ABI_VERSION) return fail("abi_version %d != %d", a.abi_version, GNN_ABI_VERSION);
    if (a.n_nodes < 1) return not_covered("gnn_train_step: empty graph");
    if (a.n_types < 1 || a.n_types > GNN_MAX_TYPES) return fail("n_types %d out of [1,%d]", a.n_types, GNN_MAX_TYPES);
    if (a.max_iteration < 1) return not_covered("composite GNN requires max_iteration > 0");
    p.N = a.n_nodes; p.E = a.n_arcs; p.L = a.dim_node_label; p.A = a.dim_arc_label; p.n_types = a.n_types;
    p.S = a.state_dim > 0 ? a.state_dim : a.dim_node_label;
    p.K = a.max_iteration; p.M = a.n_out;
    for (int t = 0; t < p.n_types; ++t) {
        if (a.type_dim_label[t] < 0 || a.type_dim_label[t] > p.L) return fail("type_dim_label[%d]=%d out of [0,%d]", t, a.type_dim_label[t], p.L);
        p.sum_d += a.type_dim_label[t];
    }
    p.W_comp = p.sum_d + p.A;
    if (a.type_offsets[0] != 0 || a.type_offsets[p.n_types] != p.N) return fail("type_offsets must span [0, n_nodes]");
    const gnn_mlp_t &no = a.net_output;
    TRY(check_mlp(no, "net_output", ws != nullptr));
    TRY(check_dropout(ta.drop_output, no, "net_output"));
    bool drop_s = false;                               // (a state network with Dropout layers: the general kernels)
    for (int t = 0; t < p.n_types; ++t) {
        TRY(check_mlp(a.net_state[t], "net_state", ws != nullptr));
        TRY(check_dropout(ta.drop_state[t], a.net_state[t], "net_state"));
        drop_s |= ta.drop_state[t].n > 0;
    }
    const bool arc = a.focus == GNN_FOCUS_ARC;      // CompositeGNN.py:315-327: [state_src | state_dst | arc label] of the masked arcs
    const int expect_o = arc ? 2 * p.S + p.A : p.S;
    if (no.in_dim != expect_o) return fail("net_output.in_dim %d != %d expected for this focus (composite models filter on the state alone)", no.in_dim, expect_o);
    p.T = no.units[no.n_layers - 1];
    p.pooled = a.focus == GNN_FOCUS_GRAPH;
    p.G = p.pooled ? a.nodegraph.n_dst : 0;
    p.R = p.pooled ? p.G : p.M;

    p.SPs = p.S <= 16 ? 16 : p.S <= 32 ? 32 : 64;
    p.n_wg = 0; p.wg_begin[0] = 0;
    for (int t = 0; t < p.n_types; ++t) {          // tiles of <= 64 nodes of ONE type
        p.n_wg += cdiv(std::max(a.type_offsets[t + 1] - a.type_offsets[t], 0), 64);
        p.wg_begin[t + 1] = p.n_wg;
    }
    p.path = composite_train_path(ta, p, drop_s);
    p.ldS = p.path == TrainPath::small ? p.SPs : p.S;
    p.B.XW = 32 * p.B.XT;
    return 0;
}

int make_cplan(const gnn_train_args_t &ta, void *ws, CPlan &p) {
    TRY(cplan_dims_and_path(ta, ws, p));
    const gnn_loop_args_t &a = ta.loop;
    const gnn_mlp_t &no = a.net_output;
    const bool arc = a.focus == GNN_FOCUS_ARC, small = p.path == TrainPath::small, big = p.path == TrainPath::big;
    Carver c(ws);
    p.grads_ok = c.take<int>(4);
    p.flags = c.take<int>(p.K + 8);
    p.k_dev = c.take<float>(4);
    p.states = c.take<float>((size_t)(p.K + 1) * p.N * p.ldS);
    p.agg_taped = (size_t)p.K * p.N * p.ldS * sizeof(float) <= agg_tape_budget();
    p.agg = c.take<float>((size_t)(p.agg_taped ? p.K : 1) * p.N * p.ldS);
    p.agg_comp = c.take<float>((size_t)p.N * std::max(p.W_comp, 1));
    p.stats_o = c.take<float>(2 * (size_t)no.in_dim);
    p.Wf_o = c.take<float>((size_t)no.in_dim * no.units[0]); p.bf_o = c.take<float>(no.units[0]);
    p.dx_o_all = c.take<float>((size_t)std::max(p.M, 1) * no.in_dim);
    p.dx_full = c.take<float>((size_t)p.N * 2 * p.S);                // (large graphs: d loss / d [state | agg] by position)
    p.G_state = c.take<float>((size_t)p.N * p.S);
    p.G_out = c.take<float>((size_t)std::max(p.M, 1) * p.T);
    p.dpred = c.take<float>((size_t)std::max(p.R, 1) * p.T);
    p.loss_rows = c.take<float>(std::max(p.R, 1));
    p.loss_part = c.take<float>(256);
    p.isrc = c.take<int>(arc ? std::max(p.M, 1) : 0); p.idst = c.take<int>(arc ? std::max(p.M, 1) : 0);
    p.part_floats = 0;
    for (int t = 0; t < p.n_types; ++t) {
        CType &y = p.ty[t];
        y.m = &a.net_state[t];
        y.g = ta.grad_state_types[t];
        y.count = a.type_offsets[t + 1] - a.type_offsets[t];
        if (y.count < 0) return fail("type_offsets must ascend");
        y.rows = a.type_nodes ? a.type_nodes + a.type_offsets[t] : nullptr;
        y.d_t = a.type_dim_label[t];
        y.in_dim = y.d_t + 2 * p.S + p.W_comp;
        if (y.m->in_dim != y.in_dim) return fail("net_state[%d].in_dim %d != %d expected from the graph dims", t, y.m->in_dim, y.in_dim);
        if (y.m->units[y.m->n_layers - 1] != p.S) return fail("net_state[%d] output width %d != state width %d", t, y.m->units[y.m->n_layers - 1], p.S);
        y.off_state = y.d_t; y.off_agg = y.d_t + p.S; y.off_comp = y.d_t + 2 * p.S;
        carve_net(c, y.nc, *y.m, big ? 0 : y.count, p.part_floats, &ta.drop_state[t]);      // (large graphs: no per-layer row buffers - the kernels stream the tape)
        y.nc.m = y.m; y.nc.g = &y.g;
        y.stats = c.take<float>((size_t)p.K * 2 * y.in_dim);
        y.stats_tpl = c.take<float>(2 * (size_t)y.in_dim);
        y.Wf = c.take<float>((size_t)p.K * y.in_dim * y.m->units[0]);
        y.bf = c.take<float>((size_t)p.K * y.m->units[0]);
        y.Gc = c.take<float>(big ? 0 : (size_t)std::max(y.count, 1) * p.S);
        y.dx = c.take<float>(big ? 0 : (size_t)std::max(y.count, 1) * 2 * p.S);
        int nc_; rows_per_chunk_for(std::max(y.count, 1), &nc_);
        p.part_floats = std::max(p.part_floats, (size_t)(nc_ + 1) * y.in_dim);
        const int tiles_t = p.wg_begin[t + 1] - p.wg_begin[t];
        p.sm_partW[t] = c.take<float>(small ? (size_t)tiles_t * ((size_t)y.in_dim * p.S + p.S) : 0);
        p.sm_partBN[t] = c.take<float>(small ? (size_t)tiles_t * 2 * y.in_dim : 0);
    }
    // every node is an output row (out_index the identity: checked on the device, read with k), one thin Dense over the state alone
    p.head_fast = big && !arc && no.n_layers == 1 && no.units[0] <= 4 && p.M == p.N && p.S % 4 == 0 && p.S / 4 <= 32 && ta.drop_output.n == 0;
    p.part_h = c.take<float>(p.head_fast ? (size_t)BIG_HEAD_BLOCKS * ((size_t)no.in_dim * no.units[0] + no.units[0]) : 0);
    p.inv = c.take<int>((small || big) ? p.N : 0);
    if (big) {
        CBig &B = p.B;
        const gnn_csr_t &ad = a.adjacency, &as = ta.adjacency_by_source;
        B.scan_tmp = c.take<int>((size_t)cdiv(p.N, SCAN_CHUNK) + 2);
        B.d.rp = c.take<int>((size_t)p.N + 1); B.d.src = c.take<int>((size_t)std::max(ad.nnz, 1));
        B.d.w = c.take<float>(ad.w ? (size_t)std::max(ad.nnz, 1) : 0); B.d.row_scale = c.take<float>(ad.row_scale ? (size_t)p.N : 0);
        B.s.rp = c.take<int>((size_t)p.N + 1); B.s.src = c.take<int>((size_t)std::max(as.nnz, 1));
        B.s.w = c.take<float>(as.w ? (size_t)std::max(as.nnz, 1) : 0); B.s.row_scale = c.take<float>(as.row_scale ? (size_t)p.N : 0);
        if (!ad.w) B.d.w = nullptr;
        if (!ad.row_scale) B.d.row_scale = nullptr;
        if (!as.w) B.s.w = nullptr;
        if (!as.row_scale) B.s.row_scale = nullptr;
        B.xc = c.take<float>((size_t)p.N * B.XW);
        B.Cc = c.take<float>((size_t)p.N * p.S);
        B.Gpos = c.take<float>((size_t)p.N * p.S);
        int counts[GNN_MAX_TYPES];
        for (int t = 0; t < p.n_types; ++t) counts[t] = p.ty[t].count;
        split_blocks(std::min(device_cus(), BIG_FWD_BLOCKS), counts, p.n_types, B.fwd_blocks);          // one 8-wave workgroup per CU
        split_blocks(2 * device_cus(), counts, p.n_types, B.bwd_blocks);                                // 256-thread workgroups, two per CU
        split_blocks(std::min(device_cus(), BIG_WGRAD_BLOCKS), counts, p.n_types, B.wgrad_blocks);      // one workgroup per CU (LDS ring)
        B.one_act = true; B.act = -1;
        for (int t = 0; t < p.n_types; ++t) {
            const CType &y = p.ty[t];
            if (y.count > 0) { if (B.act < 0) B.act = y.m->activation[0]; else if (B.act != y.m->activation[0]) B.one_act = false; }
            B.fwd_blocks[t] = std::min(B.fwd_blocks[t], std::max(1, cdiv(cdiv(std::max(y.count, 1), 16), gnn::TB_WAVES)));
            B.bwd_blocks[t] = std::min(B.bwd_blocks[t], std::max(1, cdiv(cdiv(std::max(y.count, 1), 16), 4)));
            B.wgrad_blocks[t] = std::min(B.wgrad_blocks[t], std::max(1, cdiv(std::max(y.count, 1), 64)));
            if (y.count == 0) B.fwd_blocks[t] = B.bwd_blocks[t] = B.wgrad_blocks[t] = 0;
            B.part_a[t] = c.take<float>((size_t)BIG_AGG_BLOCKS * 2 * p.S);
            B.part_y[t] = c.take<float>((size_t)std::max(BIG_FWD_BLOCKS, 1) * 2 * std::max(p.S, B.XW));
            B.part_w[t] = c.take<float>((size_t)std::max(B.wgrad_blocks[t], 1) * ((size_t)y.in_dim * p.S + p.S));
        }
        for (int t = 0; t < p.n_types; ++t) {         // the constants line of type t: [labels[:, :d_t] | aggregated_component | 1 | 0 ..]
            const CType &y = p.ty[t];
            gnn::ConstCols &cc = B.cc[t];
            memset(&cc, 0, sizeof(cc));
            if (y.d_t > 0) { cc.width[cc.n] = y.d_t; cc.wrow[cc.n] = 0; ++cc.n; }
            if (p.W_comp > 0) { cc.width[cc.n] = p.W_comp; cc.wrow[cc.n] = y.off_comp; ++cc.n; }
            B.Kc[t] = y.d_t + p.W_comp;
        }
    }
    p.sm_cc = c.take<float>(small ? (size_t)p.N * p.SPs : 0);
    p.sm_part = c.take<float>(small ? (size_t)2 * p.n_wg * 8 * p.SPs : 0);
    p.sm_dxa = c.take<float>(small ? (size_t)p.N * p.SPs : 0);
    p.sm_bar = c.take<unsigned long long>(small ? 4 : 0);
    carve_net(c, p.co, no, p.M, p.part_floats, &ta.drop_output);
    p.co.m = &no; p.co.g = &ta.grad_output;
    {
        int nc_; rows_per_chunk_for(std::max(p.M, 1), &nc_);
        p.part_floats = std::max(p.part_floats, (size_t)(nc_ + 1) * no.in_dim);
    }
    p.part = c.take<float>(p.part_floats);
    p.bytes = (c.off + 255) & ~(size_t)255;
    return 0;
}

// segments of network `y`'s input at iteration t (CompositeGNN.py:222-223): [labels[:, :d_t] | state | agg | aggregated_component], all
// read through the type's row list; returns the count and the positions of the state / agg segments
int ctype_segs(const gnn_loop_args_t &a, const CPlan &p, const CType &y, int t, gnn::Seg *segs, int *i_state, int *i_agg) {
    int n = 0;
    const float *st_t = p.states + (size_t)t * p.N * p.S;
    const float *agg_t = p.agg + (p.agg_taped ? (size_t)t * p.N * p.S : 0);
    if (y.d_t > 0) segs[n++] = gnn::Seg{a.nodes, y.rows, a.ld_nodes, y.d_t, 0};
    *i_state = n; segs[n++] = gnn::Seg{st_t, y.rows, p.S, p.S, y.off_state};
    *i_agg = n;   segs[n++] = gnn::Seg{agg_t, y.rows, p.S, p.S, y.off_agg};
    if (p.W_comp > 0) segs[n++] = gnn::Seg{p.agg_comp, y.rows, p.W_comp, p.W_comp, y.off_comp};
    return n;
}

// ---- large graphs: the step in position space (train_composite_big.hpp) --------------------------------------------------------------------
// rows [off, off + count) of the by-destination / by-source adjacency in positions
gnn_csr_t big_sub_csr(const PosCsr &c, int N, int off, int count, bool with_w) {
    gnn_csr_t r;
    r.n_dst = count; r.n_src = N; r.nnz = c.nnz; r.rowptr = c.rp + off; r.src = c.src;
    r.w = with_w ? c.w : nullptr; r.row_scale = (with_w && c.row_scale) ? c.row_scale + off : nullptr;
    return r;
}

// positions, the re-labelled adjacency, state_0 by position, every type's constants line and the constant part of its first layer
int composite_big_setup(const gnn_train_args_t &ta, CPlan &p, hipStream_t st) {
    const gnn_loop_args_t &a = ta.loop;
    CBig &B = p.B;
    k_invert_perm<<<std::min(cdiv(p.N, 256), 1024), 256, 0, st>>>(a.type_nodes, p.N, p.inv);
    LAUNCH_OK();
    TRY(build_pos_csr(a.adjacency, a.type_nodes, p.inv, p.N, B.d, B.scan_tmp, st));
    if (!ta.forward_only) TRY(build_pos_csr(ta.adjacency_by_source, a.type_nodes, p.inv, p.N, B.s, B.scan_tmp, st));      // (the backward's walk)
    if (a.state_dim > 0) TRY(gather_rows(a.state0, p.S, a.type_nodes, p.N, p.S, p.states, p.S, st));
    else TRY(gather_rows(a.nodes, a.ld_nodes, a.type_nodes, p.N, p.S, p.states, p.S, st));
    for (int q = 0; q < p.n_types; ++q) {
        const CType &y = p.ty[q];
        if (y.count == 0) continue;
        const int off = a.type_offsets[q];
        gnn::PackSegs ps{};
        if (y.d_t > 0) { ps.ptr[ps.n] = a.nodes; ps.ld[ps.n] = a.ld_nodes; ps.width[ps.n] = y.d_t; ps.wrow[ps.n] = 0; ++ps.n; }
        if (p.W_comp > 0) { ps.ptr[ps.n] = p.agg_comp; ps.ld[ps.n] = p.W_comp; ps.width[ps.n] = p.W_comp; ps.wrow[ps.n] = y.off_comp; ++ps.n; }
        float *line = B.xc + (size_t)off * B.XW;
        const int grid = (int)std::min<long>(cdiv((long)y.count * B.XW, 256), 256 * 16);
        if (B.XT == 2) k_pack_xc_pos<64><<<grid, 256, 0, st>>>(y.count, y.rows, ps, line);
        else k_pack_xc_pos<32><<<grid, 256, 0, st>>>(y.count, y.rows, ps, line);
        LAUNCH_OK();
        if (y.m->has_bn) {
            // the batch statistics of the constant columns (the same in every iteration): one pass over the packed line, moments around its
            // row 0; each segment's columns land at its BatchNorm columns of the template, which every iteration's slot starts from
            HIP_OK(hipMemsetAsync(y.stats_tpl, 0, sizeof(float) * 2 * y.in_dim, st));
            TRY(line_stats(line, B.XW, y.count, B.part_y[q], ps.width, ps.wrow, ps.n, y.stats_tpl, y.in_dim, st));
            gnn::k_replicate<<<std::min(cdiv((long)2 * y.in_dim * p.K, 256), 1024), 256, 0, st>>>(y.stats_tpl, 2 * y.in_dim, p.K, y.stats);
            LAUNCH_OK();
        }
        // Cc = b + sum over the constant columns of (a (x - mean) + beta) W: the first layer over the line's segments alone, BatchNormalization
        // applied as the columns are staged (the mean leaves the value first)
        gnn::SegDenseArgs sa{};
        sa.M = y.count; sa.H = p.S;
        int c0 = 0;
        for (int sg = 0; sg < ps.n; ++sg) { sa.seg[sa.nseg++] = gnn::Seg{line + c0, nullptr, B.XW, ps.width[sg], ps.wrow[sg]}; c0 += ps.width[sg]; }
        sa.W = y.m->kernel[0]; sa.ldw = p.S; sa.bias = y.m->bias[0]; sa.act = GNN_ACT_LINEAR;
        sa.Y = B.Cc + (size_t)off * p.S; sa.ldy = p.S;
        if (y.m->has_bn) { sa.in_gamma = y.m->bn_gamma; sa.in_beta = y.m->bn_beta; sa.in_mean = y.stats_tpl; sa.in_var = y.stats_tpl + y.in_dim; sa.in_eps = y.m->bn_eps; }
        if (sa.nseg > 0) TRY(launch_segdense(sa, st));
        else TRY(launch_copy2d(nullptr, y.m->bias[0], 0, sa.Y, p.S, y.count, p.S, p.S, st));      // (no constant inputs at all: the bias row)
    }
    return 0;
}

// the K gated training-mode iterations (CompositeGNN.py:215-234), every type's rows by its own network.  Per iteration: one neighbour sum
// (+ column statistics) per type, then ONE launch each for the statistics' finish, the folds, the first layers of all types (when they share
// the activation: the kernel is compiled per activation) and the new rows' statistics.
int composite_big_forward(const gnn_train_args_t &ta, CPlan &p, hipStream_t st) {
    const gnn_loop_args_t &a = ta.loop;
    CBig &B = p.B;
    const size_t NS = (size_t)p.N * p.S;
    for (int t = 0; t < p.K; ++t) {
        const int *gate = p.flags + t;
        const float *s_t = p.states + (size_t)t * NS;
        float *s_n = p.states + (size_t)(t + 1) * NS;
        float *agg_t = p.agg + (p.agg_taped ? (size_t)t * NS : 0);
        gnn::StatsFinishJobs fin{};
        int n_fin = 0;
        for (int q = 0; q < p.n_types; ++q) {
            CType &y = p.ty[q];
            if (y.count == 0) continue;
            const int off = a.type_offsets[q];
            const size_t ro = (size_t)off * p.S;
            const gnn_csr_t cd = big_sub_csr(B.d, p.N, off, y.count, true);
            float *stats = y.stats + (size_t)t * 2 * y.in_dim;
            if (y.m->has_bn) {
                // (moments around the previous iteration's column means, as the homogeneous step takes them)
                const float *prev = t > 0 ? y.stats + (size_t)(t - 1) * 2 * y.in_dim : nullptr;
                int grid = 0;
                TRY(launch_aggregate_stats(gate, cd, s_t, p.S, agg_t + ro, B.part_a[q], nullptr, nullptr, prev ? prev + y.off_agg : nullptr, st, &grid));
                fin.t[n_fin++] = gnn::StatsFinishT{B.part_a[q], grid, 1.0f / (float)y.count, stats + y.off_agg, stats + y.in_dim + y.off_agg, prev ? prev + y.off_agg : nullptr};
                if (t == 0) {       // (later iterations: the launch that wrote the rows left their statistics)
                    TRY(rows_stats(gate, s_t + ro, p.S, p.S, y.count, B.part_y[q], st, &grid));
                    fin.t[n_fin++] = gnn::StatsFinishT{B.part_y[q], grid, 1.0f / (float)y.count, stats + y.off_state, stats + y.in_dim + y.off_state, s_t + ro};
                }
            } else TRY(launch_aggregate(gate, cd, s_t, p.S, p.S, agg_t + ro, p.S, st));
        }
        if (n_fin > 0) { gnn::k_stats_finish_jobs<<<dim3(p.S, n_fin), 256, 0, st>>>(gate, fin, p.S); LAUNCH_OK(); }
        // the state / agg rows of every type's first layer with this iteration's statistics folded in; the bias the kernel adds is the shift of
        // THOSE columns alone (sum beta W over them) - b and the constant columns' share sit in Cc
        FoldList fl;
        gnn::TypeLaunch<gnn::TrainFwdArgs> fw{};
        gnn::StatsFinishJobs nxt{};
        int n_nxt = 0;
        fw.n = p.n_types;
        for (int q = 0; q < p.n_types; ++q) {
            CType &y = p.ty[q];
            fw.blk_begin[q + 1] = fw.blk_begin[q] + (y.count > 0 ? B.fwd_blocks[q] : 0);
            if (y.count == 0) continue;
            const gnn_mlp_t &ns = *y.m;
            const bool bn = ns.has_bn != 0;
            const size_t ro = (size_t)a.type_offsets[q] * p.S;
            float *stats = y.stats + (size_t)t * 2 * y.in_dim;
            float *Wf = y.Wf + (size_t)t * y.in_dim * p.S, *bf = y.bf + (size_t)t * p.S;
            gnn::FoldJob &j = fl.fa.job[fl.fa.n_jobs++];
            j.centred = 1;
            j.W = ns.kernel[0]; j.b = nullptr; j.K = y.in_dim; j.H = p.S;
            j.gamma = bn ? ns.bn_gamma : nullptr; j.beta = ns.bn_beta; j.mean = stats; j.var = stats + y.in_dim; j.eps = ns.bn_eps;
            j.Wf = Wf; j.bf = bf; j.blk_begin = fl.blocks;
            j.dyn0 = y.off_state; j.dyn1 = y.off_agg; j.dyn_w = p.S;
            fl.blocks += j.H;
            gnn::TrainFwdArgs &fa = fw.t[q];
            fa.in_mean = bn ? stats : nullptr;
            fa.gate = gate; fa.M = y.count;
            fa.state = s_t + ro; fa.ld_state = p.S; fa.agg = agg_t + ro; fa.ld_agg = p.S;
            fa.addend = B.Cc + ro; fa.ld_add = p.S;
            fa.Wf = Wf; fa.bf = bf; fa.H = p.S; fa.wrow_state = y.off_state; fa.wrow_agg = y.off_agg;
            fa.act = ns.activation[0];
            fa.Y = s_n + ro; fa.ldy = p.S;
            fa.thr = a.state_threshold; fa.pred_flag = p.flags + t + 1; fa.pred_k = p.k_dev; fa.pred_kval = (float)(t + 1);
            const bool next_stats = bn && t + 1 < p.K;
            fa.stat_part = next_stats ? B.part_y[q] : nullptr;
            fa.stat_shift = next_stats ? stats + y.off_state : nullptr;       // (the new rows' moments around the input rows' column means)
            if (next_stats) {
                float *nx = y.stats + (size_t)(t + 1) * 2 * y.in_dim;
                nxt.t[n_nxt++] = gnn::StatsFinishT{B.part_y[q], B.one_act ? B.fwd_blocks[q] : 0 /* (set below) */, 1.0f / (float)y.count, nx + y.off_state,
                                                   nx + y.in_dim + y.off_state, stats + y.off_state};
            }
        }
        if (fl.fa.n_jobs > 0) TRY(launch_fold_list(fl, st));
        if (B.one_act) TRY(launch_train_fwd_types(fw, B.act, p.S, st));
        else {
            int jn = 0;
            for (int q = 0; q < p.n_types; ++q) {
                if (p.ty[q].count == 0) continue;
                int grid = 0;
                TRY(launch_train_fwd_add(fw.t[q], p.S, st, &grid));
                if (fw.t[q].stat_part) nxt.t[jn++].n_part = grid;
            }
        }
        if (n_nxt > 0) { gnn::k_stats_finish_jobs<<<dim3(p.S, n_nxt), 256, 0, st>>>(gate, nxt, p.S); LAUNCH_OK(); }
    }
    return 0;
}

// back-propagation through the k executed iterations; p.G_state = d loss / d state_k in the caller's node order.  Per iteration ONE launch each
// for the weight-gradient products, their reduction, the parameter gradients and the input gradients of all types, then one transposed
// neighbour sum per type (its epilogue applies the type's activation and BatchNormalization coefficients).
int composite_big_backward(const gnn_train_args_t &ta, CPlan &p, int k, hipStream_t st) {
    const gnn_loop_args_t &a = ta.loop;
    CBig &B = p.B;
    const size_t NS = (size_t)p.N * p.S;
    if (k == 0) return 0;
    {   // the first dZ: G by position, times act'(state_k) of the row's own type
        ActRanges ar{};
        ar.n = p.n_types;
        for (int q = 0; q < p.n_types; ++q) { ar.begin[q] = a.type_offsets[q]; ar.act[q] = p.ty[q].m->activation[0]; }
        ar.begin[p.n_types] = p.N;
        k_gather_rows_dz<<<(int)std::min<long>(cdiv((long)p.N * (p.S / 4), 256), 256 * 16), 256, 0, st>>>(p.G_state, a.type_nodes, p.states + (size_t)k * NS, p.N, p.S, ar, B.Gpos);
        LAUNCH_OK();
    }
    const bool unit_w = !a.adjacency.w;       // entries depend on the destination only: the agg-half of a row's gradient is scaled once, the transposed walk is unit-weight
    float *dx = p.dx_full;
    int max_in = 1;
    for (int q = 0; q < p.n_types; ++q) max_in = std::max(max_in, p.ty[q].in_dim);
    for (int t = k - 1; t >= 0; --t) {
        const float *s_t = p.states + (size_t)t * NS;
        const float *agg_t = p.agg + (p.agg_taped ? (size_t)t * NS : 0);
        if (!p.agg_taped) {
            const gnn_csr_t all = big_sub_csr(B.d, p.N, 0, p.N, true);
            TRY(launch_aggregate(nullptr, all, s_t, p.S, p.S, p.agg, p.S, st));
        }
        gnn::TypeLaunch<gnn::TrainWgradArgs> wg;
        gnn::TypeLaunch<gnn::TrainBwdArgs> bw;
        gnn::ReduceTypes rd;
        gnn::ParamGradsTypes pg;
        memset(&wg, 0, sizeof(wg)); memset(&bw, 0, sizeof(bw)); memset(&rd, 0, sizeof(rd)); memset(&pg, 0, sizeof(pg));
        wg.n = bw.n = p.n_types;
        for (int q = 0; q < p.n_types; ++q) {
            CType &y = p.ty[q];
            wg.blk_begin[q + 1] = wg.blk_begin[q]; bw.blk_begin[q + 1] = bw.blk_begin[q];
            if (y.count == 0) continue;
            const gnn_mlp_t &ns = *y.m;
            const bool bn = ns.has_bn != 0;
            const int off = a.type_offsets[q];
            const size_t ro = (size_t)off * p.S;
            const float *stats = bn ? y.stats + (size_t)t * 2 * y.in_dim : nullptr;
            // P = [state | agg | constants]^T dZ and q = colsum(dZ) over the type's rows, then its parameter gradients and m1 / m2
            gnn::TrainWgradArgs &wa = wg.t[q];
            wa.M = y.count; wa.rows_per_wg = cdiv(cdiv(y.count, B.wgrad_blocks[q]), 64) * 64;
            wa.G = B.Gpos + ro; wa.Y = nullptr; wa.act = GNN_ACT_LINEAR;
            wa.state = s_t + ro; wa.agg = agg_t + ro; wa.xc = B.xc + (size_t)off * B.XW;
            wa.K = y.in_dim; wa.wrow_state = y.off_state; wa.wrow_agg = y.off_agg; wa.Kc = B.Kc[q]; wa.cs = B.cc[q];
            wa.part = B.part_w[q];
            wa.mean = stats;
            const int grid = cdiv(y.count, wa.rows_per_wg);
            wg.blk_begin[q + 1] = wg.blk_begin[q] + grid;
            const int nP = y.in_dim * p.S + p.S;
            rd.t[q] = gnn::ReduceT{B.part_w[q], grid, nP, y.nc.P, 0, 1.0f, y.in_dim * p.S, y.nc.q};
            pg.t[q] = gnn::ParamGradsT{y.nc.P, y.nc.q, ns.kernel[0], y.in_dim, p.S, bn ? ns.bn_gamma : nullptr, ns.bn_beta, stats, stats ? stats + y.in_dim : nullptr, ns.bn_eps,
                                       1.0f / (float)y.count, y.g.dkernel[0], y.g.dbias[0], y.g.dgamma, y.g.dbeta, bn ? y.nc.m1 : nullptr, bn ? y.nc.m2 : nullptr,
                                       t != k - 1 ? 1 : 0, 1, stats ? 1 : 0};
            gnn::TrainBwdArgs &ba = bw.t[q];
            ba.M = y.count; ba.dZ = B.Gpos + ro; ba.ldz = p.S;
            ba.W = ns.kernel[0]; ba.ldw = p.S; ba.H = p.S; ba.S = p.S; ba.wrow_state = y.off_state; ba.wrow_agg = y.off_agg;
            ba.state = s_t + ro; ba.ld_state = p.S; ba.agg = agg_t + ro; ba.ld_agg = p.S;
            if (bn) { ba.gamma = ns.bn_gamma; ba.mean = stats; ba.var = stats + y.in_dim; ba.m1 = y.nc.m1; ba.m2 = y.nc.m2; ba.eps = ns.bn_eps; }
            ba.defer_state_bn = bn ? 1 : 0;    // (k_aggregate_dz below adds the rest of the state half's BatchNorm gradient: it reads state_t anyway)
            ba.agg_row_scale = (unit_w && B.d.row_scale) ? B.d.row_scale + off : nullptr;
            ba.dx = dx + (size_t)off * 2 * p.S; ba.ld_dx = 2 * p.S;
            bw.blk_begin[q + 1] = bw.blk_begin[q] + B.bwd_blocks[q];
        }
        TRY(launch_train_wgrad_types(wg, p.S, B.XT, st));
        gnn::k_reduce_partials_types<<<dim3(cdiv(max_in * p.S + p.S, 64), p.n_types), 256, 0, st>>>(rd);
        LAUNCH_OK();
        gnn::k_first_layer_param_grads_types<<<dim3(max_in, p.n_types), 64, 0, st>>>(pg);
        LAUNCH_OK();
        if (t == 0) break;                 // nothing consumes d loss / d state_0: no input gradient, no transposed sum
        TRY(launch_train_bwd_types(bw, p.S, st));
        // dZ_{t-1} = (dx_state' + Adj . dx_agg + the deferred BatchNorm term) (.) act'(state_t): arcs by source, every type's rows with ITS network's
        // coefficients and activation (state_t's rows of type q are outputs of network q and inputs of network q)
        for (int q = 0; q < p.n_types; ++q) {
            const CType &y = p.ty[q];
            if (y.count == 0) continue;
            const gnn_mlp_t &ns = *y.m;
            const int off = a.type_offsets[q];
            const size_t ro = (size_t)off * p.S;
            const gnn_csr_t cs = big_sub_csr(B.s, p.N, off, y.count, !unit_w);
            gnn::AggDzArgs z{};
            z.Y = s_t + ro; z.ldy = p.S; z.wrow_state = y.off_state;
            if (ns.has_bn) {
                const float *stats = y.stats + (size_t)t * 2 * y.in_dim;
                z.gamma = ns.bn_gamma; z.var = stats + y.in_dim; z.mean = stats; z.m1 = y.nc.m1; z.m2 = y.nc.m2; z.eps = ns.bn_eps;
            }
            if (!launch_aggregate_dz(cs, dx + p.S, 2 * p.S, B.Gpos + ro, p.S, dx + (size_t)off * 2 * p.S, 2 * p.S, z, ns.activation[0], p.S, st))
                return fail("k_aggregate_dz: no instance for state width %d / activation %d", p.S, ns.activation[0]);
            LAUNCH_OK();
        }
    }
    return 0;
}

size_t composite_train_workspace_bytes(const gnn_train_args_t &ta) {
    CPlan p;
    if (make_cplan(ta, nullptr, p)) return 0;
    return p.bytes;
}

// ==== the composite step's own phases, in the order train_step_composite() below calls them ==============================================

// the constant inputs of type y's first layer: [labels[:, :d_t] | aggregated_component]
gnn::ConstSegs ctype_const_segs(const gnn_loop_args_t &a, const CPlan &p, const CType &y) {
    gnn::ConstSegs cs{};
    if (y.d_t > 0) { cs.ptr[cs.n] = a.nodes; cs.ld[cs.n] = a.ld_nodes; cs.width[cs.n] = y.d_t; cs.wrow[cs.n] = 0; ++cs.n; }
    if (p.W_comp > 0) { cs.ptr[cs.n] = p.agg_comp; cs.ld[cs.n] = p.W_comp; cs.width[cs.n] = p.W_comp; cs.wrow[cs.n] = y.off_comp; ++cs.n; }
    return cs;
}

// ---- label gradients (gnn_train_step_composite_ex): what the caller wants, and the scratch of its own they live in (the tape keeps its layout)
// `lab`: the constant segments' gradient is wanted (sum of dZ per type); `g0`: state_0 = nodes - d loss / d state_0 is part of d loss / d nodes
struct CLabelWants { bool nodes, lab, g0; };
struct CLabelScratch {
    float *dz;                       // small graphs: [N][SPs] sum_t dZ_t by POSITION (the persistent backward launch stores it)
    float *g0;                       // small graphs, state_dim == 0: [N][SPs] d loss / d state_0 by position
    float *dz_t[GNN_MAX_TYPES];      // general path: [count_t][H_t] per type, zeroed per step, accumulated by net_backward
    size_t dz_t_bytes;               // ... all of them, contiguous from dz_t[0]
    float *g_comp;                   // [N][W_comp] d loss / d aggregated_component by node
    size_t bytes;
};

CLabelScratch carve_label_scratch(const gnn_train_args_t &ta, const CPlan &p, void *base) {
    CLabelScratch sc{};
    Carver c(base);
    const bool small = p.path == TrainPath::small;
    sc.dz = c.take<float>(small ? (size_t)p.N * p.SPs : 0);
    sc.g0 = c.take<float>(small && ta.loop.state_dim == 0 ? (size_t)p.N * p.SPs : 0);
    const size_t first = (c.off + 255) & ~(size_t)255;
    for (int q = 0; q < p.n_types; ++q) sc.dz_t[q] = c.take<float>(small ? 0 : (size_t)std::max(p.ty[q].count, 0) * p.ty[q].m->units[0]);
    sc.dz_t_bytes = c.off - std::min(first, c.off);
    sc.g_comp = c.take<float>((size_t)p.N * std::max(p.W_comp, 1));
    sc.bytes = (c.off + 255) & ~(size_t)255;
    return sc;
}

int moving_state(const gnn_train_args_t &ta, const CPlan &p, int k, const int *gate, hipStream_t st) {
    for (int q = 0; q < p.n_types; ++q)
        if (p.ty[q].count > 0) TRY(bn_moving(*p.ty[q].m, p.ty[q].stats, k, ta.bn_momentum, gate, st));
    return 0;
}

// ---- setup: the previous step's validity word, transposes, aggregated_component (CompositeGNN.py:251-253), state_0 (by position on the two
// fast paths: position i = node type_nodes[i]), the constant columns' statistics
int composite_setup(const gnn_train_args_t &ta, CPlan &p, hipStream_t st) {
    const gnn_loop_args_t &a = ta.loop;
    const bool small = p.path == TrainPath::small, big = p.path == TrainPath::big;
    if (ta.prev_grads_ok_host) HIP_OK(hipMemcpyAsync(ta.prev_grads_ok_host, p.grads_ok, sizeof(int), hipMemcpyDeviceToHost, st));
    if (!ta.forward_only) {               // (a forward leaves the word of the last STEP on this tape as it is)
        HIP_OK(hipMemsetAsync(p.grads_ok, 0, sizeof(int) * 4, st));
        if (ta.grads_ok_dev) *ta.grads_ok_dev = p.grads_ok;
        for (int t = 0; t < p.n_types; ++t) TRY(transposes(p.ty[t].nc, st));
        TRY(transposes(p.co, st));
    }
    HIP_OK(hipMemsetAsync(p.flags, 0, sizeof(int) * (p.K + 8), st));
    HIP_OK(hipMemsetAsync(p.k_dev, 0, sizeof(float) * 4, st));
    int col = 0;
    for (int t = 0; t < p.n_types; ++t) {
        const int dt = a.type_dim_label[t];
        if (dt > 0) TRY(launch_aggregate(nullptr, a.composite_adjacency[t], a.nodes, a.ld_nodes, dt, p.agg_comp + col, p.W_comp, st));
        col += dt;
    }
    if (p.A > 0) TRY(launch_aggregate(nullptr, a.arcnode, a.arc_labels, a.ld_arcs, p.A, p.agg_comp + col, p.W_comp, st));
    if (small) {            // rows of ldS floats, pad columns zero
        if (p.ldS != p.S) HIP_OK(hipMemsetAsync(p.states, 0, sizeof(float) * p.N * p.ldS, st));
        if (a.state_dim > 0) TRY(gather_rows(a.state0, p.S, a.type_nodes, p.N, p.S, p.states, p.ldS, st));
        else TRY(gather_rows(a.nodes, a.ld_nodes, a.type_nodes, p.N, p.S, p.states, p.ldS, st));
        k_invert_perm<<<std::min(cdiv(p.N, 256), 1024), 256, 0, st>>>(a.type_nodes, p.N, p.inv);
        LAUNCH_OK();
    } else if (!big) {      // (large graphs: composite_big_setup below)
        if (a.state_dim > 0) HIP_OK(hipMemcpyAsync(p.states, a.state0, sizeof(float) * p.N * p.ldS, hipMemcpyDeviceToDevice, st));
        else TRY(launch_copy2d(nullptr, a.nodes, a.ld_nodes, p.states, p.S, p.N, p.S, p.S, st));
    }
    gnn::Seg segs[GNN_MAX_SEGS];
    for (int t = 0; t < p.n_types && !big; ++t) {      // (large graphs: composite_big_setup takes them from the packed constants line, one pass)
        CType &y = p.ty[t];
        if (!y.m->has_bn || y.count == 0) continue;
        int is_, ia_;
        const int n = ctype_segs(a, p, y, 0, segs, &is_, &ia_);
        gnn::Seg cst[GNN_MAX_SEGS]; int nc = 0;
        for (int s = 0; s < n; ++s) if (s != is_ && s != ia_) cst[nc++] = segs[s];
        HIP_OK(hipMemsetAsync(y.stats_tpl, 0, sizeof(float) * 2 * y.in_dim, st));
        TRY(colstats_segs(nullptr, cst, nc, y.count, y.stats_tpl, y.stats_tpl + y.in_dim, p.part, st));
        gnn::k_replicate<<<std::min(cdiv((long)2 * y.in_dim * p.K, 256), 1024), 256, 0, st>>>(y.stats_tpl, 2 * y.in_dim, p.K, y.stats);
        LAUNCH_OK();
    }
    // (gnn_last_kernel_name(): which orchestration took the step - tests and bench.py read it)
    if (big) GNN_SET_KERNEL_NAME("train_step composite: row-streaming kernels on type ranges (fwd_b6<ADD>, wgrad_b6<XT=%d>)", p.B.XT);
    else if (small) GNN_SET_KERNEL_NAME("train_step composite: persistent small-graph kernels");
    else GNN_SET_KERNEL_NAME("train_step composite: general kernels (one launch per layer, type and iteration)");
    if (big) TRY(composite_big_setup(ta, p, st));
    return finish_setup(ta, p, st);
}

// ---- training-mode forward: K gated iterations; tape = states, neighbour sums, per-type statistics (large graphs: composite_big_forward) ----
// Small graphs: one persistent launch over tiles of <= 64 consecutive positions of ONE type (`tiles`); per type the network, its statistics
// tape and where its shares go (`yt`) - the backward launch takes the same tables (host data alone: a phase-2 call builds them again)
int composite_tile_tables(const gnn_train_args_t &ta, const CPlan &p, gnn::TileTab &tiles, gnn::TypeTab &yt) {
    const gnn_loop_args_t &a = ta.loop;
    int b = 0;
    for (int q = 0; q < p.n_types; ++q) {
        const CType &y = p.ty[q];
        const int pos0 = a.type_offsets[q];
        for (int r0 = 0; r0 < y.count; r0 += 64) tiles.begin[b++] = pos0 + r0;
        yt.wg_begin[q] = p.wg_begin[q]; yt.count[q] = y.count;
        yt.W[q] = y.m->kernel[0]; yt.gamma[q] = y.m->has_bn ? y.m->bn_gamma : nullptr; yt.beta[q] = y.m->bn_beta; yt.stats[q] = y.stats;
        yt.in_s[q] = y.in_dim; yt.off_state[q] = y.off_state; yt.off_agg[q] = y.off_agg; yt.act[q] = y.m->activation[0];
        yt.partW[q] = p.sm_partW[q]; yt.partBN[q] = p.sm_partBN[q];
    }
    tiles.begin[b] = p.N; tiles.n = b;
    yt.n = p.n_types; yt.wg_begin[p.n_types] = p.n_wg; yt.perm = a.type_nodes; yt.inv = p.inv;
    if (b != p.n_wg) return fail("composite tiles: %d != %d", b, p.n_wg);
    return 0;
}

int composite_forward_small(const gnn_train_args_t &ta, CPlan &p, gnn::TileTab &tiles, gnn::TypeTab &yt, hipStream_t st) {
    const gnn_loop_args_t &a = ta.loop;
    TRY(composite_tile_tables(ta, p, tiles, yt));
    // the constant part of every node's first layer (its type's network over its labels and the aggregated component), in position order
    for (int q = 0; q < p.n_types; ++q) {
        const CType &y = p.ty[q];
        if (y.count == 0) continue;
        gnn::k_train_small_const<<<cdiv(y.count * p.SPs, 256), 256, 0, st>>>(y.count, p.SPs, p.S, ctype_const_segs(a, p, y), y.m->kernel[0], y.m->bias[0],
                                                                         y.m->has_bn ? y.m->bn_gamma : nullptr, y.m->bn_beta, y.stats_tpl, y.stats_tpl + y.in_dim,
                                                                         y.m->bn_eps, p.sm_cc + (size_t)a.type_offsets[q] * p.SPs, y.rows);
        LAUNCH_OK();
    }
    HIP_OK(hipMemsetAsync(p.sm_bar, 0, sizeof(unsigned long long) * 4, st));
    gnn::TrainSmallFwd fa{};
    fa.eps = composite_small_eps(p);
    return launch_train_small_fwd(fa, ta, p, tiles, &yt, st);
}

// the general path: one launch per layer, type and iteration, every type's rows through its row list
int composite_forward_general(const gnn_train_args_t &ta, CPlan &p, hipStream_t st) {
    const gnn_loop_args_t &a = ta.loop;
    gnn::Seg segs[GNN_MAX_SEGS];
    for (int t = 0; t < p.K; ++t) {
        const int *gate = p.flags + t;
        const float *s_t = state_at(p, t);
        float *s_n = state_at(p, t + 1);
        TRY(launch_aggregate(gate, a.adjacency, s_t, p.S, p.S, agg_at(p, t), p.S, st));
        for (int q = 0; q < p.n_types; ++q) {
            CType &y = p.ty[q];
            if (y.count == 0) continue;
            const gnn_mlp_t &ns = *y.m;
            int is_, ia_;
            const int n = ctype_segs(a, p, y, t, segs, &is_, &ia_);
            const gnn::Seg dyn[2] = {segs[is_], segs[ia_]};
            FirstLayer f;
            TRY(first_layer_of(ns, gate, dyn, y.count, y.stats + (size_t)t * 2 * y.in_dim, y.Wf + (size_t)t * y.in_dim * ns.units[0], y.bf + (size_t)t * ns.units[0],
                               p.part, f, st));
            const DropRun drs = drop_run(&ta.drop_state[q], ta.drop_seed, t, y.nc);      // (ABI 8: the type's Dropout layers, fresh masks every iteration)
            TRY(forward_layers(ns, segs, n, y.count, f.W0, f.b0, y.nc.hid, gate, st, nullptr, f.bn_on_load, f.centre, &drs));
            // the type's rows of the new state (CompositeGNN.py:229-231: scatter_nd + reduce_sum over the one-hot types).  A closed gate
            // leaves the layer buffers stale and the scatter harmless: state t + 1 is never read then.
            TRY(scatter_rows(drop_at(&drs, ns.n_layers) ? drs.buf[ns.n_layers] : y.nc.hid[ns.n_layers - 1], p.S, y.rows, y.count, p.S, s_n, p.S, st));
        }
        TRY(launch_converge(gate, s_n, s_t, p.N, p.S, p.S, p.S, a.state_threshold, p.flags + t + 1, p.k_dev, (float)(t + 1), st));
    }
    return 0;
}

// ---- backward through the k executed iterations; p.G_state = d loss / d state_k in the caller's node order (large graphs:
// composite_big_backward).  Small graphs: one persistent launch, then every tile's [kernel | bias] (and [d gamma | d beta]) share of ITS
// type's gradients summed in tile order
int composite_backward_small(const gnn_train_args_t &ta, CPlan &p, const gnn::TileTab &tiles, const gnn::TypeTab &yt, int k, const CLabelScratch &sc,
                             const CLabelWants &w, hipStream_t st) {
    gnn::TypeConsts yc{};
    for (int q = 0; q < p.n_types; ++q) yc.cs[q] = ctype_const_segs(ta.loop, p, p.ty[q]);
    gnn::TrainSmallBwd ba{};
    ba.eps = composite_small_eps(p); ba.dxa = p.sm_dxa;
    ba.dz_out = w.lab ? sc.dz : nullptr; ba.g0_out = w.g0 ? sc.g0 : nullptr;      // (by POSITION, rows of SPs floats: the LAB instantiations)
    TRY(launch_train_small_bwd(ba, ta, p, k, tiles, &yt, &yc, st));
    for (int q = 0; q < p.n_types; ++q) {
        const CType &y = p.ty[q];
        const int tiles_q = p.wg_begin[q + 1] - p.wg_begin[q];
        if (tiles_q == 0) continue;
        const int n = (y.in_dim + 1) * p.S;
        gnn::k_reduce_partials<<<cdiv(n, 64), 256, 0, st>>>(p.sm_partW[q], tiles_q, n, y.g.dkernel[0], 0, 1.0f, y.in_dim * p.S, y.g.dbias[0]);
        LAUNCH_OK();
        if (y.m->has_bn) {
            gnn::k_reduce_partials<<<cdiv(2 * y.in_dim, 64), 256, 0, st>>>(p.sm_partBN[q], tiles_q, 2 * y.in_dim, y.g.dgamma, 0, 1.0f, y.in_dim, y.g.dbeta);
            LAUNCH_OK();
        }
    }
    return 0;
}

// the general path: net_backward per type and iteration on the type's gathered rows, then the transposed aggregate over all nodes
int composite_backward_general(const gnn_train_args_t &ta, CPlan &p, int k, const CLabelScratch &sc, const CLabelWants &w, hipStream_t st) {
    const gnn_loop_args_t &a = ta.loop;
    gnn::Seg segs[GNN_MAX_SEGS];
    for (int t = k - 1; t >= 0; --t) {
        const float *s_t = state_at(p, t), *s_n = state_at(p, t + 1), *agg_t = agg_at(p, t);
        if (!p.agg_taped) TRY(launch_aggregate(nullptr, a.adjacency, s_t, p.S, p.S, p.agg, p.S, st));
        for (int q = 0; q < p.n_types; ++q) {
            CType &y = p.ty[q];
            if (y.count == 0) continue;
            const gnn_mlp_t &ns = *y.m;
            int is_, ia_;
            const int n = ctype_segs(a, p, y, t, segs, &is_, &ia_);
            const float *stats = ns.has_bn ? y.stats + (size_t)t * 2 * y.in_dim : nullptr;
            float *const *hs = y.nc.hid;
            const DropRun drs = drop_run(&ta.drop_state[q], ta.drop_seed, t, y.nc);      // (iteration t's masks again: the same keys)
            const bool drop_any = ta.drop_state[q].n > 0;
            TRY(recompute_hidden(ns, segs, n, y.count, stats, y.Wf + (size_t)t * y.in_dim * ns.units[0], y.bf + (size_t)t * ns.units[0], hs, drs, drop_any, st));
            if (!drop_any) TRY(gather_rows(s_n, p.S, y.rows, y.count, p.S, hs[ns.n_layers - 1], p.S, st));      // the last layer's output: the type's rows of state t + 1
            TRY(gather_rows(p.G_state, p.S, y.rows, y.count, p.S, y.Gc, p.S, st));
            TRY(net_backward(y.nc, segs, n, hs, y.Gc, p.S, y.count, stats, t != k - 1, y.dx, 2 * p.S, p.part, st, -1, y.off_state, &drs, w.lab ? sc.dz_t[q] : nullptr));
            gnn::BnGradReq rq[2] = {gnn::BnGradReq{y.dx, 2 * p.S, s_t, p.S, y.rows, p.S, y.off_state},
                                    gnn::BnGradReq{y.dx + p.S, 2 * p.S, agg_t, p.S, y.rows, p.S, y.off_agg}};
            TRY(bn_input_grads(ns, y.nc, stats, rq, 2, y.count, st));
            TRY(scatter_rows(y.dx, 2 * p.S, y.rows, y.count, 2 * p.S, p.dx_full, 2 * p.S, st));
        }
        // G_state = d state (own) + Adj . d agg   (arcs walked by source)
        TRY(launch_aggregate_add(ta.adjacency_by_source, p.dx_full + p.S, 2 * p.S, p.S, p.dx_full, 2 * p.S, p.G_state, p.S, st));
    }
    return 0;
}

// ---- d loss / d nodes: one launch turns every type's sum_t dZ_t into the gradients of its constant inputs (k_label_grads_types: the own-label
// columns straight into d_nodes, d loss / d aggregated_component into the scratch), then per type t' with labels the transposed CompositeAdjacency
// aggregate of its component columns on top (CompositeGNN.py:251 transposed), and d loss / d state_0 where state_0 = nodes.  The composite output
// network reads the state alone: no head label segments.
int composite_label_grads(const gnn_train_args_t &ta, const gnn_train_phase_args_t &px, const gnn_train_composite_phase_args_t &cx, const CPlan &p,
                          const CLabelScratch &sc, int k, const CLabelWants &w, hipStream_t st) {
    const gnn_loop_args_t &a = ta.loop;
    const int ldn = px.ld_d_nodes > 0 ? px.ld_d_nodes : p.L;
    float *d_nodes = px.d_nodes;
    const bool small = p.path == TrainPath::small;
    if (k == 0) {                  // no iteration ran: nothing reached the constants
        if (w.g0) return launch_copy2d(nullptr, p.G_state, p.S, d_nodes, ldn, p.N, p.L, p.L, st);
        HIP_OK(hipMemset2DAsync(d_nodes, sizeof(float) * ldn, 0, sizeof(float) * p.L, p.N, st));
        return 0;
    }
    gnn::LabelGradTypesArgs la{};
    la.n_types = p.n_types; la.L = p.L; la.W_comp = p.W_comp;
    la.type_nodes = a.type_nodes; la.nodes = a.nodes; la.ld_nodes = a.ld_nodes; la.agg_comp = p.agg_comp;
    la.lab_own = d_nodes; la.ld_own = ldn; la.g_comp = sc.g_comp;
    int H_max = 1;
    for (int q = 0; q < p.n_types; ++q) {
        const CType &y = p.ty[q];
        const gnn_mlp_t &m = *y.m;
        la.tile_begin[q + 1] = la.tile_begin[q] + cdiv(std::max(y.count, 0), gnn::LG_ROWS);
        gnn::LabelGradType &t = la.t[q];
        t.pos0 = a.type_offsets[q]; t.count = y.count; t.H = m.units[0];
        t.DZ = small ? sc.dz + (size_t)t.pos0 * p.SPs : sc.dz_t[q]; t.ldz = small ? p.SPs : t.H;
        t.W = m.kernel[0]; t.d_t = y.d_t; t.wrow_comp = y.off_comp;
        if (m.has_bn) { t.gamma = m.bn_gamma; t.mean = y.stats_tpl; t.var = y.stats_tpl + y.in_dim; t.dgamma = y.g.dgamma; t.dbeta = y.g.dbeta; t.eps = m.bn_eps; }
        t.inv_n = 1.0f / (float)std::max(y.count, 1);
        if (y.count > 0) H_max = std::max(H_max, t.H);
    }
    const int n_tiles = la.tile_begin[p.n_types];
    gnn::k_label_grads_types<<<std::min(n_tiles, 4096), 256, sizeof(float) * gnn::LG_ROWS * (H_max + 1), st>>>(la);
    LAUNCH_OK();
    int col = 0;
    for (int q = 0; q < p.n_types; ++q) {
        const int dt = a.type_dim_label[q];
        if (dt > 0) TRY(launch_aggregate_add(cx.composite_adjacency_by_source[q], sc.g_comp + col, p.W_comp, dt, d_nodes, ldn, d_nodes, ldn, st));
        col += dt;
    }
    if (w.g0) {                    // state_0 = nodes (CompositeGNN.py:258); the persistent launch left it by position
        if (small) TRY(scatter_add_rows(sc.g0, p.SPs, a.type_nodes, p.N, p.S, d_nodes, ldn, st));
        else { gnn::k_add2d<<<std::min(cdiv((long)p.N * p.S, 256), 1024), 256, 0, st>>>(d_nodes, ldn, p.G_state, p.S, p.N, p.S); LAUNCH_OK(); }
    }
    return 0;
}

// what gnn_train_composite_phases_supported answers from the plan: the paths with phases, first layers the label-gradient kernel can stage
int composite_phases_covered(const CPlan &p) {
    if (p.path == TrainPath::big)
        return not_covered("gnn_train_step_composite_ex: the row-streaming path (>= GNN_TRAIN_BIG_MIN_NODES nodes) has no phases / upstream gradients / label gradients: such steps train through the building blocks");
    for (int q = 0; q < p.n_types; ++q)
        if (p.ty[q].m->units[0] > gnn::LG_MAX_H)
            return not_covered("gnn_train_step_composite_ex: first state layer of %d units (at most %d)", p.ty[q].m->units[0], gnn::LG_MAX_H);
    return 0;
}

// the two extra argument blocks against the plan: everything that refuses a call, before its first launch
int check_composite_phase_args(const gnn_train_args_t &ta, const gnn_train_phase_args_t &px, const gnn_train_composite_phase_args_t *cx, const CPlan &p,
                               const CLabelScratch &need) {
    TRY(composite_phases_covered(p));
    TRY(check_phase_loss_kind(ta, px));
    TRY(check_phase_state(px, p.K, p.L, "gnn_train_step_composite_ex"));
    if (px.phase != 0 || px.d_nodes) {
        if (!cx || !cx->scratch || ((uintptr_t)cx->scratch & 255) != 0) return fail("gnn_train_step_composite_ex: phases and label gradients need cx->scratch, a 256-byte aligned device buffer");
        if (cx->scratch_bytes < need.bytes) return fail("gnn_train_step_composite_ex: scratch too small: %zu < %zu bytes", cx->scratch_bytes, need.bytes);
    }
    for (int q = 0; q < p.n_types && px.d_nodes; ++q) {
        if (ta.loop.type_dim_label[q] <= 0) continue;
        if (!cx->composite_adjacency_by_source[q].rowptr) return fail("gnn_train_step_composite_ex: d_nodes needs composite_adjacency_by_source[%d]", q);
        TRY(check_csr(cx->composite_adjacency_by_source[q], "composite_adjacency_by_source", p.N, p.N));
    }
    return 0;
}

// The step as its phases.  `px` / `cx` (gnn_train_step_composite_ex; all-zero / NULL: the plain gnn_train_step): phase 1 stops behind the output
// network, in front of the loss, with the tape kept; phase 2 goes on from there with the k phase 1 learned at its synchronisation - the launches
// of the whole step, in its order, cut in two.
int train_step_composite(const gnn_train_args_t &ta, const gnn_train_phase_args_t &px, const gnn_train_composite_phase_args_t *cx) {
    const gnn_loop_args_t &a = ta.loop;
    CPlan p;
    const bool fwd_only = ta.forward_only != 0;         // the training-mode forward alone: no loss, no gradients, the validity word untouched
    const int phase = px.phase;
    // (`d_arc_labels`, which the predicate counts and this line did not spell out, is NULL here: gnn_train_step_composite_ex refuses it in
    // front of this call, and the plain step hands in an all-zero block)
    const bool ex = phase_block_used(px);
    if (fwd_only && ta.prev_grads_ok_host) return fail("gnn_train_step(forward_only): prev_grads_ok_host must be NULL");
    TRY(make_cplan(ta, ta.tape, p));
    CLabelScratch sc{};
    if (ex) {
        const CLabelScratch need = carve_label_scratch(ta, p, nullptr);
        TRY(check_composite_phase_args(ta, px, cx, p, need));
        if (cx && cx->scratch) sc = carve_label_scratch(ta, p, cx->scratch);
    }
    if (!ta.tape || ta.tape_bytes < p.bytes) return fail("tape too small: %zu < %zu bytes", ta.tape_bytes, p.bytes);
    const bool do_fwd = phase != GNN_TRAIN_PHASE_BACKWARD;        // phase 0 / 1: setup, loop, output network
    const bool no_loss = ta.loss_kind == GNN_LOSS_NONE && phase != 0;
    TRY(check_step_args(ta, p, !fwd_only && phase != GNN_TRAIN_PHASE_FORWARD && !no_loss, !fwd_only && phase != GNN_TRAIN_PHASE_FORWARD));
    const bool small = p.path == TrainPath::small, big = p.path == TrainPath::big;
    const gnn_mlp_t &no = a.net_output;
    hipStream_t st = (hipStream_t)a.stream;

    // ---- forward: setup, the K gated iterations on the plan's path, k (the step's one synchronisation), the converged state -----------------
    gnn::TileTab tiles;
    gnn::TypeTab yt;
    memset(&tiles, 0, sizeof(tiles)); memset(&yt, 0, sizeof(yt));
    int k = 0;
    if (do_fwd) {
        TRY(composite_setup(ta, p, st));
        TRY(big ? composite_big_forward(ta, p, st) : small ? composite_forward_small(ta, p, tiles, yt, st) : composite_forward_general(ta, p, st));
        TRY(read_k(ta, p, &k, st));
        if (phase == GNN_TRAIN_PHASE_FORWARD) *px.phase_state = gnn_train_phase_state_t{PHASE_MAGIC, k, 1, 0};      // (phases: always the general head)
        if (small || big) TRY(scatter_rows(state_at(p, k), p.ldS, a.type_nodes, p.N, p.S, ta.state, p.S, st));      // positions -> the caller's node order
        else HIP_OK(hipMemcpyAsync(ta.state, state_at(p, k), sizeof(float) * p.N * p.ldS, hipMemcpyDeviceToDevice, st));
        if (!small) TRY(moving_state(ta, p, k, nullptr, st));          // (the persistent path: moving_deferred)
    } else {                       // phase 2: what phase 1 learned at its synchronisation; the host tables of the persistent backward launch again
        k = px.phase_state->k;
        if (ta.grads_ok_dev) *ta.grads_ok_dev = p.grads_ok;
        if (small) TRY(composite_tile_tables(ta, p, tiles, yt));
    }
    const float *state_k = ta.state;                                   // [N, S] in the caller's node order

    // ---- output network on the converged state of the masked nodes (CompositeGNN.py:237-239, :270), training mode ----------------------------
    HeadRun h;
    TRY(head_segments(ta, p, state_k, p.S, 0, do_fwd, h, st));
    if (do_fwd) {
        const bool stats_one_pass = p.M > 0 && no.has_bn && p.head_fast;
        if (stats_one_pass) {      // every node a row, in order: one pass over the state (moments around its row 0)
            int grid = 0;
            TRY(rows_stats(nullptr, state_k, p.S, p.S, p.N, p.B.part_y[0], st, &grid));
            gnn::k_stats_finish<<<p.S, 256, 0, st>>>(nullptr, p.B.part_y[0], grid, p.S, 1.0f / (float)p.N, p.stats_o, p.stats_o + no.in_dim, state_k);
            LAUNCH_OK();
        }
        TRY(head_forward(ta, p, h, stats_one_pass, st));
        if (px.node_out && p.M > 0) HIP_OK(hipMemcpyAsync(px.node_out, h.out_nodes, sizeof(float) * (size_t)p.M * p.T, hipMemcpyDeviceToDevice, st));
    }
    if (phase == GNN_TRAIN_PHASE_FORWARD) return 0;                    // THE PHASE CUT, in front of the loss: the tape is kept, phase 2 goes on from here
    if (fwd_only) return moving_deferred(ta, p, k, nullptr, st);       // the forward alone: what the persistent path keeps back for the validity word is due now

    // ---- loss and its gradient, upstream gradients added ------------------------------------------------------------------------------------------
    float *G_out = nullptr;
    TRY(loss_gradient(ta, p, !no_loss, px.loss_scale, px.d_pred_extra, &G_out, st));
    if (px.d_out_extra && p.M > 0) TRY(add_into(G_out, px.d_out_extra, (size_t)p.M * p.T, st));
    const CLabelWants want{px.d_nodes != nullptr, px.d_nodes != nullptr, px.d_nodes != nullptr && a.state_dim == 0};
    if (want.lab && !small && k > 0 && sc.dz_t_bytes > 0) HIP_OK(hipMemsetAsync(sc.dz_t[0], 0, sc.dz_t_bytes, st));

    // ---- backward: output network, the k iterations on the plan's path, label gradients ------------------------------------------------------------
    // (the thin head: its parameter gradients, d loss / d state_k written straight into the state gradient - every row is an output row)
    if (p.head_fast) TRY(head_backward(p, a, nullptr, 0, state_k, p.S, h.out_nodes, G_out, no.has_bn ? p.stats_o : nullptr, st, -1));
    else TRY(head_backward_general(ta, p, h, G_out, st));
    if (px.d_state_extra) TRY(add_into(p.G_state, px.d_state_extra, (size_t)p.N * p.S, st));
    for (int q = 0; q < p.n_types; ++q)
        if (k == 0 || p.ty[q].count == 0) TRY(zero_grads(*p.ty[q].m, p.ty[q].g, st));
    if (big) TRY(composite_big_backward(ta, p, k, st));
    else if (small && k > 0) TRY(composite_backward_small(ta, p, tiles, yt, k, sc, want, st));
    else if (!small) TRY(composite_backward_general(ta, p, k, sc, want, st));
    if (want.nodes) TRY(composite_label_grads(ta, px, *cx, p, sc, k, want, st));
    for (int q = 0; q < p.n_types && ta.average_st_grads && k > 0; ++q) TRY(scale_grads(*p.ty[q].m, p.ty[q].g, 1.0f / (float)k, st));
    return finish_step(ta, p, k, st);
}

int train_step_composite(const gnn_train_args_t &ta) {
    gnn_train_phase_args_t none;
    memset(&none, 0, sizeof(none));
    return train_step_composite(ta, none, nullptr);
}

}  // namespace

extern "C" {

int gnn_train_composite_phases_supported(const gnn_train_args_t *args) {
    if (!args || !args->loop.composite || args->n_groups != 0 || args->forward_only) return -1;
    CPlan p;
    if (make_cplan(*args, nullptr, p)) return -1;
    return composite_phases_covered(p) ? -1 : 0;
}

size_t gnn_train_composite_phase_scratch_bytes(const gnn_train_args_t *args) {
    if (!args) { fail("args is NULL"); return 0; }
    if (!args->loop.composite || args->n_groups != 0 || args->forward_only) {
        not_covered("gnn_train_step_composite_ex covers whole steps of heterogeneous models only (gnn_train_composite_phases_supported)");
        return 0;
    }
    CPlan p;
    if (make_cplan(*args, nullptr, p) || composite_phases_covered(p)) return 0;
    return carve_label_scratch(*args, p, nullptr).bytes;
}

int gnn_train_step_composite_ex(const gnn_train_args_t *args, const gnn_train_phase_args_t *px, const gnn_train_composite_phase_args_t *cx) {
    if (!args) return fail("args is NULL");
    gnn_train_phase_args_t x;
    memset(&x, 0, sizeof(x));
    if (px) x = *px;
    if (!phase_block_used(x) && !cx) return gnn_train_step(args);                 // exactly the plain call: same checks, same order, same messages
    const gnn_train_args_t &ta = *args;
    if (!ta.tape || ((uintptr_t)ta.tape & 255) != 0) return fail("tape must be a 256-byte aligned device buffer");
    if (x.phase < 0 || x.phase > GNN_TRAIN_PHASE_BACKWARD) return fail("gnn_train_step_composite_ex: unknown phase %d", x.phase);
    if (!ta.loop.composite) return not_covered("gnn_train_step_composite_ex: heterogeneous models only (homogeneous models have gnn_train_step_ex)");
    if (ta.n_groups != 0 || ta.forward_only)
        return not_covered("gnn_train_step_composite_ex: phases, upstream gradients and label gradients cover whole steps only (no convergence groups, no forward_only)");
    if (x.d_arc_labels) return not_covered("gnn_train_step_composite_ex: no composite arc-label gradient (d_arc_labels): such stacks train through the building blocks");
    return landed_on_failure(ta, train_step_composite(ta, x, cx));
}

}  // extern "C"

