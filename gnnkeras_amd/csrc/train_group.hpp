// Host side of the grouped training-mode forward (C ABI 10; kernels_train_group.hpp): coverage, group tables, workspace, launches.
// Included behind train_loop.hpp and train_composite.hpp in gnnloop.hip (shares their plans and helpers).  Heterogeneous models (one state
// network per node type) take the *_types kernels of kernels_train_group_types.hpp.  Each kind has its own plan (workspace carve), coverage
// rule, constants kernel and argument struct; what the two forwards share exists once, in the first half of this file: the group tables and
// their upload, the refusals (train_group_checks), the launcher of the forward kernel, the shared argument fields and the output head.
#pragma once
#include "kernels_train_group.hpp"
#include "kernels_train_group_types.hpp"

namespace {

static_assert(GNN_TRAIN_GROUP_MAX_NODES == gnn::GROUP_CAP, "include/gnnloop.h and kernels_train_group.hpp disagree on the group size");

// ---- both kinds ------------------------------------------------------------------------------------------------------------------------------
// the host tables: 0 fine, -2 malformed (message set when `say`), g + 1: group g is too large
int train_group_tables(const gnn_train_args_t &ta, int N, int M, bool say, int *max_nodes) {
    const int G = ta.n_groups;
    if (max_nodes) *max_nodes = 0;
    if (!ta.group_node_begin || !ta.group_out_begin) { if (say) fail("group_node_begin / group_out_begin is NULL"); return GNN_TRAIN_GROUPS_MALFORMED; }
    if (ta.group_node_begin[0] != 0 || ta.group_node_begin[G] != N) { if (say) fail("group_node_begin must span [0, n_nodes]"); return GNN_TRAIN_GROUPS_MALFORMED; }
    if (ta.group_out_begin[0] != 0 || ta.group_out_begin[G] != M) { if (say) fail("group_out_begin must span [0, n_out]"); return GNN_TRAIN_GROUPS_MALFORMED; }
    int too_large = 0, mx = 0;
    for (int g = 0; g < G; ++g) {
        const int n = ta.group_node_begin[g + 1] - ta.group_node_begin[g];
        if (n <= 0) { if (say) fail("group %d is empty or group_node_begin is not ascending", g); return GNN_TRAIN_GROUPS_MALFORMED; }
        if (ta.group_out_begin[g + 1] < ta.group_out_begin[g]) { if (say) fail("group_out_begin is not ascending at group %d", g); return GNN_TRAIN_GROUPS_MALFORMED; }
        if (n > gnn::GROUP_CAP && !too_large) too_large = g + 1;
        mx = std::max(mx, n);
    }
    if (max_nodes) *max_nodes = mx;
    return too_large;
}

// gnn_train_groups_supported for one kind: its plan from dims alone, its coverage rule, the tables
template <class Plan, class Make, class Covered>
int train_groups_supported(const gnn_train_args_t &ta, Make make, Covered covered) {
    Plan p;
    if (make(ta, nullptr, p) || !covered(ta, p)) return GNN_TRAIN_GROUPS_UNCOVERED;
    return train_group_tables(ta, p.N, p.M, false, nullptr);
}

// Everything a grouped forward refuses before its first launch, in this order.  GP is the kind's group plan (GroupPlan / GroupTypesPlan:
// p with N, M, E, A; max_nodes; bytes), `make` carves it from ta.tape, `covered` is the kind's coverage rule and `inputs` the kind's own
// checks of its input arrays (between the arcnode CSR and state0).
template <class GP, class Make, class Covered, class Inputs>
int train_group_checks(const gnn_train_args_t &ta, GP &gp, Make make, Covered covered, Inputs inputs) {
    const gnn_loop_args_t &a = ta.loop;
    if (!ta.forward_only) return not_covered("gnn_train_step: convergence groups need forward_only (a grouped training step is not implemented)");
    if (ta.prev_grads_ok_host) return fail("gnn_train_step(forward_only): prev_grads_ok_host must be NULL");
    if (ta.n_groups < 0) return fail("n_groups < 0");
    TRY(make(ta, ta.tape, gp));
    const auto &p = gp.p;
    if (!covered(ta, p)) return not_covered("gnn_train_step: convergence groups do not cover this shape (gnn_train_groups_supported() == %d)", GNN_TRAIN_GROUPS_UNCOVERED);
    const int tab = train_group_tables(ta, p.N, p.M, true, &gp.max_nodes);
    if (tab < 0) return 1;
    if (tab > 0) return not_covered("group %d has %d nodes (at most %d per convergence group: gnn_train_groups_supported())", tab - 1,
                                    ta.group_node_begin[tab] - ta.group_node_begin[tab - 1], gnn::GROUP_CAP);
    if (ta.tape_bytes < gp.bytes) return fail("tape too small: %zu < %zu bytes", ta.tape_bytes, gp.bytes);
    TRY(check_csr(a.adjacency, "adjacency", p.N, p.N));
    TRY(check_csr(a.arcnode, "arcnode", p.N, p.E));
    TRY(inputs());
    if (a.state_dim > 0 && !a.state0) return fail("state0 is required when state_dim > 0");
    if (p.M > 0 && !a.out_index) return fail("out_index is NULL");
    if (a.focus == GNN_FOCUS_ARC && p.E > 0 && (!a.arc_src || !a.arc_dst)) return fail("arc focus needs arc_src / arc_dst");
    if ((p.M > 0 && !ta.y_pred) || !ta.state || !ta.k_groups) return fail("y_pred / state / k_groups is NULL");
    return 0;
}

// the group tables go to the device through a pinned staging buffer of this thread; its event says when the previous call's copy has left it
int upload_group_tables(const gnn_train_args_t &ta, int *gbeg, int *obeg, hipStream_t st) {
    static thread_local struct { int *buf; size_t cap; hipEvent_t ev; } stage = {nullptr, 0, nullptr};
    const int G = ta.n_groups;
    const size_t n_tab = 2 * ((size_t)G + 1);
    if (stage.ev) HIP_OK(hipEventSynchronize(stage.ev));
    else HIP_OK(hipEventCreateWithFlags(&stage.ev, hipEventDisableTiming));
    if (stage.cap < n_tab) {
        if (stage.buf) HIP_OK(hipHostFree(stage.buf));
        stage.buf = nullptr; stage.cap = 0;
        HIP_OK(hipHostMalloc((void **)&stage.buf, std::max<size_t>(n_tab, 4096) * sizeof(int), hipHostMallocDefault));
        stage.cap = std::max<size_t>(n_tab, 4096);
    }
    memcpy(stage.buf, ta.group_node_begin, ((size_t)G + 1) * sizeof(int));
    memcpy(stage.buf + G + 1, ta.group_out_begin, ((size_t)G + 1) * sizeof(int));
    HIP_OK(hipMemcpyAsync(gbeg, stage.buf, ((size_t)G + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(obeg, stage.buf + G + 1, ((size_t)G + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_OK(hipEventRecord(stage.ev, st));
    return 0;
}

// the argument fields both forward kernels read (S = the padded width, Sw the real one)
void fill_train_group_common(gnn::TrainGroupCommon &fa, const gnn_train_args_t &ta, int S, int Sw, int K, const int *gbeg, float *agg, const float *cc) {
    const gnn_loop_args_t &a = ta.loop;
    fa.S = S; fa.Sw = Sw; fa.K = K;
    fa.rowptr = a.adjacency.rowptr; fa.src = a.adjacency.src; fa.w = a.adjacency.w; fa.row_scale = a.adjacency.row_scale;
    fa.gbeg = gbeg;
    fa.state0 = a.state_dim > 0 ? a.state0 : a.nodes; fa.ld0 = a.state_dim > 0 ? Sw : a.ld_nodes;
    fa.state_out = ta.state; fa.agg = agg; fa.Cc = cc; fa.thr = a.state_threshold; fa.k_groups = ta.k_groups;
}

// One launcher for both forward kernels.  A kernel family F names its argument struct, its instantiations and their LDS:
//     using Args; template <int SQ, bool HAS_W> static constexpr void (*fn)(Args); template <int SQ> static size_t lds(int rows)
//     static constexpr int MAX_SQ: the widest instantiation the family has (the hidden-layer forms stop at padded width 32)
struct TrainGroupKernel {
    using Args = gnn::TrainGroupFwd;
    static constexpr int MAX_SQ = 4;
    template <int SQ, bool HAS_W> static constexpr void (*fn)(Args) = gnn::k_train_group_fwd<SQ, HAS_W>;
    template <int SQ> static size_t lds(int rows) { return gnn::train_group_fwd_lds<SQ>(rows); }
};
struct TrainGroupTypesKernel {
    using Args = gnn::TrainGroupFwdTypes;
    static constexpr int MAX_SQ = 4;
    template <int SQ, bool HAS_W> static constexpr void (*fn)(Args) = gnn::k_train_group_fwd_types<SQ, HAS_W>;
    template <int SQ> static size_t lds(int rows) { return gnn::train_group_fwd_types_lds<SQ>(rows); }
};
struct TrainGroupKernelH {
    using Args = gnn::TrainGroupFwdH;
    static constexpr int MAX_SQ = 2;
    template <int SQ, bool HAS_W> static constexpr void (*fn)(Args) = gnn::k_train_group_fwd<SQ, HAS_W, true>;
    template <int SQ> static size_t lds(int rows) { return gnn::train_group_fwd_lds<SQ, true>(rows); }
};
struct TrainGroupTypesKernelH {
    using Args = gnn::TrainGroupFwdTypesH;
    static constexpr int MAX_SQ = 2;
    template <int SQ, bool HAS_W> static constexpr void (*fn)(Args) = gnn::k_train_group_fwd_types<SQ, HAS_W, true>;
    template <int SQ> static size_t lds(int rows) { return gnn::train_group_fwd_types_lds<SQ, true>(rows); }
};

template <class F, int SQ, bool HAS_W>
int launch_train_group_fwd_one(const typename F::Args &fa, int G, int max_nodes, hipStream_t st) {
    constexpr auto kern = F::template fn<SQ, HAS_W>;
    // (the limit is raised to what the largest group allowed needs, once per kernel)
    static std::mutex m;
    static bool raised = false;
    {
        std::lock_guard<std::mutex> lock(m);
        if (!raised) {
            HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)F::template lds<SQ>(gnn::GROUP_CAP)));
            raised = true;
        }
    }
    kern<<<G, gnn::TS_NT, F::template lds<SQ>(max_nodes), st>>>(fa);
    LAUNCH_OK();
    return 0;
}

template <class F>
int launch_train_group_fwd(const typename F::Args &fa, int G, int max_nodes, hipStream_t st) {
    const bool has_w = fa.w != nullptr;
    switch (fa.S) {
        case 16: return has_w ? launch_train_group_fwd_one<F, 1, true>(fa, G, max_nodes, st) : launch_train_group_fwd_one<F, 1, false>(fa, G, max_nodes, st);
        case 32: return has_w ? launch_train_group_fwd_one<F, 2, true>(fa, G, max_nodes, st) : launch_train_group_fwd_one<F, 2, false>(fa, G, max_nodes, st);
        default:
            if constexpr (F::MAX_SQ >= 4) return has_w ? launch_train_group_fwd_one<F, 4, true>(fa, G, max_nodes, st) : launch_train_group_fwd_one<F, 4, false>(fa, G, max_nodes, st);
            else return fail("grouped forward: no kernel of padded width %d in this form", fa.S);       // (the coverage rule refuses the width first)
    }
}

int launch_train_group_head(const gnn::TrainGroupHead &h, int G, hipStream_t st) {
    const size_t lds = gnn::train_group_head_lds(h.in_o, h.T);
    static std::mutex m;
    static bool raised = false;
    {
        std::lock_guard<std::mutex> lock(m);
        if (!raised) {
            HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void *>(&gnn::k_train_group_head), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)gnn::train_group_head_lds(gnn::GROUP_HEAD_MAX_IN, gnn::GROUP_HEAD_MAX_UNITS)));
            raised = true;
        }
    }
    gnn::k_train_group_head<<<G, 256, lds, st>>>(h);
    LAUNCH_OK();
    return 0;
}

// The output network on every group's output rows, then its moving statistics in group order.  Input row: [state] (node focus),
// [state_src | state_dst | arc label] (arc focus); `with_labels`: every state is followed by the node's L label columns (homogeneous models
// with a state of its own - composite models filter on the state alone).
int train_group_output(const gnn_train_args_t &ta, int G, int S, int L, int A, int M, int T, bool with_labels, const int *obeg, int *isrc, int *idst,
                       float *stats_o, hipStream_t st) {
    const gnn_loop_args_t &a = ta.loop;
    const gnn_mlp_t &no = a.net_output;
    const bool bn_o = no.has_bn != 0;
    if (M < 1) return 0;
    gnn::TrainGroupHead h;
    memset(&h, 0, sizeof(h));
    int n = 0;
    auto seg = [&](const float *ptr, const int *idx, int ld, int width) { h.sg.ptr[n] = ptr; h.sg.idx[n] = idx; h.sg.ld[n] = ld; h.sg.width[n] = width; ++n; };
    if (a.focus == GNN_FOCUS_ARC) {
        k_arc_endpoints<<<cdiv(M, 256), 256, 0, st>>>(a.out_index, a.arc_src, a.arc_dst, M, isrc, idst);
        LAUNCH_OK();
        const int *ends[2] = {isrc, idst};
        for (int e = 0; e < 2; ++e) {
            seg(ta.state, ends[e], S, S);
            if (with_labels) seg(a.nodes, ends[e], a.ld_nodes, L);
        }
        if (A > 0) seg(a.arc_labels, a.out_index, a.ld_arcs, A);
    } else {
        seg(ta.state, a.out_index, S, S);
        if (with_labels) seg(a.nodes, a.out_index, a.ld_nodes, L);
    }
    h.sg.n = n;
    h.obeg = obeg; h.in_o = no.in_dim; h.T = T; h.act = no.activation[0];
    h.W = no.kernel[0]; h.b = no.bias[0]; h.gamma = bn_o ? no.bn_gamma : nullptr; h.beta = no.bn_beta; h.eps = no.bn_eps;
    h.stats_o = stats_o; h.out = ta.y_pred;
    TRY(launch_train_group_head(h, G, st));
    if (bn_o) {
        gnn::k_bn_moving_groups<<<cdiv(no.in_dim, 64), 64, 0, st>>>(stats_o, 1, no.in_dim, ta.k_groups, obeg, G, const_cast<float *>(no.bn_mean),
                                                                  const_cast<float *>(no.bn_var), ta.bn_momentum, 0);
        LAUNCH_OK();
    }
    return 0;
}

// ---- homogeneous models ----------------------------------------------------------------------------------------------------------------------
struct GroupPlan {
    TrainPlan p;                 // dims only (planned without a workspace)
    int G, max_nodes;
    int *gbeg, *obeg;            // device copies of the host tables
    float *agg_arcs, *agg_nodes, *cc, *agg, *stats_s, *stats_o;
    int *isrc, *idst;
    size_t bytes;
};

// The hidden-layer form of the grouped forward kernels (opt-in: GNN_FLAG_TRAIN_GROUPS_HIDDEN; both model kinds, every type's network on its
// own): what hidden_dense_of_state_width() (train_loop.hpp) accepts - Dense(H) - Dense(S), 1 <= H <= the padded state width `SPs`, neither
// activation softmax, padded width 16 or 32.  At 64 the one-layer instantiations already hold 256 VGPRs and up to 209 AGPRs, and a W2 block
// [64][68] with its bias next to a 256-row state would take the workgroup's LDS to 157 KB of 160 KB: that width is refused.  (A state network
// with Dropout is refused by the callers, as in the one-layer rule.)
inline bool train_groups_hidden_net(const gnn_train_args_t &ta, const gnn_mlp_t &m, int S, int SPs) {
    return (ta.loop.flags & GNN_FLAG_TRAIN_GROUPS_HIDDEN) != 0 && hidden_dense_of_state_width(m, S, SPs);
}

// what the grouped kernels cover (dims and network descriptions only)
bool train_groups_covered(const gnn_train_args_t &ta, const TrainPlan &p) {
    const gnn_loop_args_t &a = ta.loop;
    const gnn_mlp_t &ns = a.net_state[0], &no = a.net_output;
    if (a.composite || a.n_types > 1) return false;
    if (ta.drop_state[0].n > 0 || ta.drop_output.n > 0) return false;
    if (a.focus != GNN_FOCUS_NODE && a.focus != GNN_FOCUS_ARC) return false;
    if (!train_groups_hidden_net(ta, ns, p.S, p.SPs) && (ns.n_layers != 1 || ns.units[0] != p.S || ns.activation[0] == GNN_ACT_SOFTMAX)) return false;
    if (p.S > 64 || p.Kc > 32 || p.K < 1) return false;
    if (no.n_layers != 1 || no.units[0] > gnn::GROUP_HEAD_MAX_UNITS || no.in_dim > gnn::GROUP_HEAD_MAX_IN) return false;
    return true;
}

int make_group_plan(const gnn_train_args_t &ta, void *ws, GroupPlan &gp) {
    TRY(make_train_plan(ta, nullptr, gp.p));
    const TrainPlan &p = gp.p;
    gp.G = ta.n_groups;
    Carver c(ws);
    gp.gbeg = c.take<int>((size_t)gp.G + 1); gp.obeg = c.take<int>((size_t)gp.G + 1);
    gp.agg_arcs = c.take<float>((size_t)p.N * std::max(p.A, 1));
    gp.agg_nodes = c.take<float>((size_t)p.N * std::max(p.L, 1));
    gp.cc = c.take<float>((size_t)p.N * p.SPs);
    gp.agg = c.take<float>((size_t)p.N * p.SPs);
    gp.stats_s = c.take<float>((size_t)gp.G * p.K * 2 * p.in_s);
    gp.stats_o = c.take<float>((size_t)gp.G * 2 * p.in_o);
    gp.isrc = c.take<int>(std::max(p.M, 1)); gp.idst = c.take<int>(std::max(p.M, 1));
    gp.bytes = (c.off + 255) & ~(size_t)255;
    return 0;
}

size_t group_types_workspace_bytes(const gnn_train_args_t &ta);

size_t group_train_workspace_bytes(const gnn_train_args_t &ta) {
    if (ta.n_groups < 0) { fail("n_groups < 0"); return 0; }
    if (ta.loop.composite) return group_types_workspace_bytes(ta);
    GroupPlan gp;
    if (make_group_plan(ta, nullptr, gp)) return 0;
    return gp.bytes;
}

int train_forward_groups_types(const gnn_train_args_t &ta);

int train_forward_groups(const gnn_train_args_t &ta) {
    const gnn_loop_args_t &a = ta.loop;
    if (a.composite) return train_forward_groups_types(ta);
    GroupPlan gp;
    TRY(train_group_checks(ta, gp, make_group_plan, train_groups_covered, [&]() -> int {
        if (!a.nodes || (gp.p.E > 0 && gp.p.A > 0 && !a.arc_labels)) return fail("nodes / arc_labels is NULL");
        return 0;
    }));
    const TrainPlan &p = gp.p;
    const gnn_mlp_t &ns = a.net_state[0];
    TRY(check_mlp(ns, "net_state", true));
    TRY(check_mlp(a.net_output, "net_output", true));
    const bool bn_s = ns.has_bn != 0;
    const bool hidden = train_groups_hidden_net(ta, ns, p.S, p.SPs);
    hipStream_t st = (hipStream_t)a.stream;
    const int G = gp.G;
    GNN_SET_KERNEL_NAME(hidden ? "train_step: grouped forward kernels (hidden)" : "train_step: grouped forward kernels");

    TRY(upload_group_tables(ta, gp.gbeg, gp.obeg, st));
    // aggregates of the constants over the merged graph (block-diagonal: a row sees its own group only)
    if (p.A > 0) TRY(launch_aggregate(nullptr, a.arcnode, a.arc_labels, a.ld_arcs, p.A, gp.agg_arcs, p.A, st));
    if (p.with_labels) TRY(launch_aggregate(nullptr, a.adjacency, a.nodes, a.ld_nodes, p.L, gp.agg_nodes, p.L, st));
    gnn::ConstSegs cs;
    memset(&cs, 0, sizeof(cs));
    cs.n = p.cc.n;
    for (int s = 0; s < cs.n; ++s) { cs.width[s] = p.cc.width[s]; cs.wrow[s] = p.cc.wrow[s]; }
    if (p.with_labels) {
        cs.ptr[0] = a.nodes; cs.ld[0] = a.ld_nodes;
        cs.ptr[1] = gp.agg_nodes; cs.ld[1] = p.L;
        cs.ptr[2] = gp.agg_arcs; cs.ld[2] = p.A;
    } else { cs.ptr[0] = gp.agg_arcs; cs.ld[0] = p.A; }
    gnn::k_train_group_const<<<G, 256, 0, st>>>(gp.gbeg, p.SPs, ns.units[0], cs, ns.kernel[0], ns.bias[0], bn_s ? ns.bn_gamma : nullptr, ns.bn_beta, ns.bn_eps,
                                                gp.cc, gp.stats_s, p.K, p.in_s);
    LAUNCH_OK();
    gnn::TrainGroupFwdH fa;             // (the one-layer kernels take its base)
    memset(&fa, 0, sizeof(fa));
    fill_train_group_common(fa, ta, p.SPs, p.S, p.K, gp.gbeg, gp.agg, gp.cc);
    fa.stats = gp.stats_s; fa.in_s = p.in_s; fa.off_agg = p.off_agg;
    fa.W = ns.kernel[0]; fa.gamma = bn_s ? ns.bn_gamma : nullptr; fa.beta = ns.bn_beta; fa.eps = ns.bn_eps; fa.act = ns.activation[0];
    if (hidden) {
        fa.Hw = ns.units[0]; fa.W2 = ns.kernel[1]; fa.b2 = ns.bias[1]; fa.act2 = ns.activation[1];
        TRY(launch_train_group_fwd<TrainGroupKernelH>(fa, G, gp.max_nodes, st));
    } else TRY(launch_train_group_fwd<TrainGroupKernel>(static_cast<const gnn::TrainGroupFwd &>(fa), G, gp.max_nodes, st));
    if (bn_s) {
        gnn::k_bn_moving_groups<<<cdiv(p.in_s, 64), 64, 0, st>>>(gp.stats_s, p.K, p.in_s, ta.k_groups, nullptr, G, const_cast<float *>(ns.bn_mean),
                                                                const_cast<float *>(ns.bn_var), ta.bn_momentum);
        LAUNCH_OK();
    }
    return train_group_output(ta, G, p.S, p.L, p.A, p.M, p.T, p.with_labels, gp.obeg, gp.isrc, gp.idst, gp.stats_o, st);
}


// ---- heterogeneous models ---------------------------------------------------------------------------------------------------------------------
struct GroupTypesPlan {
    CPlan p;                     // dims only (planned without a workspace)
    int G, max_nodes, SPs;
    int *gbeg, *obeg, *tbeg;     // device: the host tables, and the rows of every type per group [n_types][G + 1]
    float *agg_comp, *cc, *agg, *stats_t[GNN_MAX_TYPES], *stats_o;
    int *isrc, *idst;
    size_t bytes;
};

// what the *_types kernels cover (dims and network descriptions only).  BatchNormalization may differ between the types: every (group, type)
// is normalised on its own.  Hidden-layer form: every type's network train_groups_hidden_net() accepts (H and the activations may differ
// between the types); a model that mixes one-layer and two-layer networks is not covered.
bool train_groups_types_covered(const gnn_train_args_t &ta, const CPlan &p) {
    const gnn_loop_args_t &a = ta.loop;
    const gnn_mlp_t &no = a.net_output;
    if (!a.composite || p.n_types < 1 || p.n_types > GNN_MAX_TYPES) return false;
    if (a.focus != GNN_FOCUS_NODE && a.focus != GNN_FOCUS_ARC) return false;
    if (p.S > 64 || p.K < 1 || ta.drop_output.n > 0) return false;
    const bool hidden = train_groups_hidden_net(ta, a.net_state[0], p.S, p.SPs);
    for (int t = 0; t < p.n_types; ++t) {
        const gnn_mlp_t &ns = a.net_state[t];
        if (ta.drop_state[t].n > 0) return false;
        if (hidden ? !train_groups_hidden_net(ta, ns, p.S, p.SPs) : (ns.n_layers != 1 || ns.units[0] != p.S || ns.activation[0] == GNN_ACT_SOFTMAX)) return false;
        if (a.type_dim_label[t] + p.W_comp > gnn::GROUP_TYPES_MAX_KC) return false;
    }
    if (no.n_layers != 1 || no.units[0] > gnn::GROUP_HEAD_MAX_UNITS || no.in_dim > gnn::GROUP_HEAD_MAX_IN) return false;
    return true;
}

int make_group_types_plan(const gnn_train_args_t &ta, void *ws, GroupTypesPlan &gp) {
    TRY(make_cplan(ta, nullptr, gp.p));
    const CPlan &p = gp.p;
    gp.G = ta.n_groups;
    gp.SPs = p.S <= 16 ? 16 : p.S <= 32 ? 32 : 64;
    Carver c(ws);
    gp.gbeg = c.take<int>((size_t)gp.G + 1); gp.obeg = c.take<int>((size_t)gp.G + 1);
    gp.tbeg = c.take<int>((size_t)p.n_types * (gp.G + 1));
    gp.agg_comp = c.take<float>((size_t)p.N * std::max(p.W_comp, 1));
    gp.cc = c.take<float>((size_t)p.N * gp.SPs);
    gp.agg = c.take<float>((size_t)p.N * gp.SPs);
    for (int t = 0; t < p.n_types; ++t) gp.stats_t[t] = c.take<float>((size_t)gp.G * p.K * 2 * p.ty[t].in_dim);
    gp.stats_o = c.take<float>((size_t)gp.G * 2 * ta.loop.net_output.in_dim);
    gp.isrc = c.take<int>(std::max(p.M, 1)); gp.idst = c.take<int>(std::max(p.M, 1));
    gp.bytes = (c.off + 255) & ~(size_t)255;
    return 0;
}

size_t group_types_workspace_bytes(const gnn_train_args_t &ta) {
    GroupTypesPlan gp;
    if (make_group_types_plan(ta, nullptr, gp)) return 0;
    return gp.bytes;
}

int train_forward_groups_types(const gnn_train_args_t &ta) {
    const gnn_loop_args_t &a = ta.loop;
    GroupTypesPlan gp;
    TRY(train_group_checks(ta, gp, make_group_types_plan, train_groups_types_covered, [&]() -> int {
        for (int t = 0; t < gp.p.n_types; ++t) {
            TRY(check_csr(a.composite_adjacency[t], "composite_adjacency", gp.p.N, gp.p.N));
            TRY(check_mlp(a.net_state[t], "net_state", true));
        }
        if (!a.nodes || !a.type_nodes) return fail("nodes / type_nodes is NULL");
        if (gp.p.E > 0 && gp.p.A > 0 && !a.arc_labels) return fail("arc_labels is NULL");
        return 0;
    }));
    const CPlan &p = gp.p;
    TRY(check_mlp(a.net_output, "net_output", true));
    hipStream_t st = (hipStream_t)a.stream;
    const int G = gp.G, SPs = gp.SPs;
    const bool hidden = train_groups_hidden_net(ta, a.net_state[0], p.S, p.SPs);      // (the rule: then every type's network is)
    GNN_SET_KERNEL_NAME(hidden ? "train_step: grouped forward kernels (types, hidden)" : "train_step: grouped forward kernels (types)");

    TRY(upload_group_tables(ta, gp.gbeg, gp.obeg, st));
    // the rows of every type per group: groups are contiguous node ranges, a type's row list ascends
    {
        gnn::TypeOffsets to;
        for (int t = 0; t <= GNN_MAX_TYPES; ++t) to.off[t] = t <= p.n_types ? a.type_offsets[t] : p.N;
        gnn::k_group_type_begin<<<cdiv(p.n_types * (G + 1), 256), 256, 0, st>>>(a.type_nodes, to, p.n_types, gp.gbeg, G, gp.tbeg);
        LAUNCH_OK();
    }
    // aggregated_component over the merged graph (block-diagonal: a row sees its own group only), as train_step_composite builds it
    {
        int col = 0;
        for (int t = 0; t < p.n_types; ++t) {
            const int dt = a.type_dim_label[t];
            if (dt > 0) TRY(launch_aggregate(nullptr, a.composite_adjacency[t], a.nodes, a.ld_nodes, dt, gp.agg_comp + col, p.W_comp, st));
            col += dt;
        }
        if (p.A > 0) TRY(launch_aggregate(nullptr, a.arcnode, a.arc_labels, a.ld_arcs, p.A, gp.agg_comp + col, p.W_comp, st));
    }
    gnn::TrainGroupConstTypes ca;
    gnn::GroupTypeWidths hw;
    gnn::TrainGroupFwdTypes fa;
    gnn::TrainGroupFwdTypesH fh;
    memset(&ca, 0, sizeof(ca)); memset(&hw, 0, sizeof(hw)); memset(&fa, 0, sizeof(fa)); memset(&fh, 0, sizeof(fh));
    for (int t = 0; t < p.n_types; ++t) {
        const CType &y = p.ty[t];
        const gnn_mlp_t &ns = a.net_state[t];
        gnn::GroupTypeNet &n = ca.net[t];
        n.W = ns.kernel[0]; n.b = ns.bias[0]; n.gamma = ns.has_bn ? ns.bn_gamma : nullptr; n.beta = ns.bn_beta; n.eps = ns.bn_eps;
        n.act = ns.activation[0]; n.d_t = y.d_t; n.in_dim = y.in_dim; n.off_state = y.off_state; n.off_agg = y.off_agg; n.off_comp = y.off_comp;
        n.stats = gp.stats_t[t];
        hw.Hw[t] = ns.units[0];
        fa.net[t] = n;
        if (hidden) {
            gnn::GroupTypeNetH &h = fh.net[t];
            static_cast<gnn::GroupTypeNet &>(h) = n;
            h.Hw = ns.units[0]; h.W2 = ns.kernel[1]; h.b2 = ns.bias[1]; h.act2 = ns.activation[1];
        }
    }
    ca.n_types = p.n_types; ca.G = G; ca.S = SPs; ca.Sw = p.S; ca.K = p.K; ca.W_comp = p.W_comp;
    ca.tbeg = gp.tbeg; ca.type_nodes = a.type_nodes; ca.nodes = a.nodes; ca.ld_nodes = a.ld_nodes; ca.agg_comp = gp.agg_comp; ca.Cc = gp.cc;
    gnn::k_train_group_const_types<<<G, 256, 0, st>>>(ca, hw);
    LAUNCH_OK();
    if (hidden) {
        fill_train_group_common(fh, ta, SPs, p.S, p.K, gp.gbeg, gp.agg, gp.cc);
        fh.n_types = p.n_types; fh.G = G; fh.tbeg = gp.tbeg; fh.type_nodes = a.type_nodes;
        TRY(launch_train_group_fwd<TrainGroupTypesKernelH>(fh, G, gp.max_nodes, st));
    } else {
        fill_train_group_common(fa, ta, SPs, p.S, p.K, gp.gbeg, gp.agg, gp.cc);
        fa.n_types = p.n_types; fa.G = G; fa.tbeg = gp.tbeg; fa.type_nodes = a.type_nodes;
        TRY(launch_train_group_fwd<TrainGroupTypesKernel>(fa, G, gp.max_nodes, st));
    }
    // the moving statistics of network t: k_g steps for every group with rows of type t, group after group
    for (int t = 0; t < p.n_types; ++t) {
        const gnn_mlp_t &ns = a.net_state[t];
        if (!ns.has_bn) continue;
        const int in_t = p.ty[t].in_dim;
        gnn::k_bn_moving_groups<<<cdiv(in_t, 64), 64, 0, st>>>(gp.stats_t[t], p.K, in_t, ta.k_groups, gp.tbeg + (size_t)t * (G + 1), G, const_cast<float *>(ns.bn_mean),
                                                              const_cast<float *>(ns.bn_var), ta.bn_momentum, 1);
        LAUNCH_OK();
    }
    return train_group_output(ta, G, p.S, 0, p.A, p.M, p.T, false, gp.obeg, gp.isrc, gp.idst, gp.stats_o, st);
}

}  // namespace

extern "C" int gnn_train_groups_supported(const gnn_train_args_t *args) {
    if (!args || args->n_groups < 1 || !args->forward_only) return GNN_TRAIN_GROUPS_UNCOVERED;
    if (args->loop.composite) return train_groups_supported<CPlan>(*args, make_cplan, train_groups_types_covered);
    return train_groups_supported<TrainPlan>(*args, make_train_plan, train_groups_covered);
}
