// Convergence groups of a training-mode forward for HETEROGENEOUS models (one state network per node type; gnn_train_step(forward_only) with
// group_node_begin on composite arguments).  The homogeneous kernels of kernels_train_group.hpp with one more level: inside a group the rows
// of type t are a contiguous slice of type t's ascending row list (groups are contiguous node ranges), and everything that is "per network"
// - the BatchNormalization statistics, the weights, the activation - is per (group, type).
//
//   k_group_type_begin          tbeg[t][g] = first position in type_nodes, at or behind type t's begin, whose node id is >= gbeg[g]; the rows of
//                               type t in group g are type_nodes[tbeg[t][g] .. tbeg[t][g + 1])
//   k_train_group_const_types   per group and type: statistics of the Kc_t = d_t + W_comp constant columns over the group's rows of that type
//                               (two passes, centred) into all K slots, then the rows' constant part Cc with network t's weights
//   k_train_group_fwd_types     per group: the state of ALL rows of the group lives in LDS, indexed by node.  Per iteration
//                                 pass 1  neighbour sums of every 64-node tile from the OLD state, parked in memory (owning workgroup only)
//                                 then type after type: the type's rows in 64-row tiles that never mix types - [own | neighbour sum] -> LDS,
//                                 column sums around the tile's first row merged in double, (a (x - mean) + beta) . W_t + Cc on
//                                 v_mfma_f32_16x16x4_f32, type t's activation, the predicate, the rows back into the LDS state
//                               A row of type 1 reads its OWN old row when its turn comes (type 0 wrote type 0's rows only) and the neighbour
//                               sums of pass 1: no gather ever sees a new row of the running iteration.
// The weight block [2 S][S + 4] of the CURRENT type is (re)loaded from L2 when the walk moves to another type with rows in the group: one block
// fits next to a 256-row state at width 64 (138 KB), eight do not.  A group whose rows are all of one type loads it once.
// Hidden-layer form (HID; see kernels_train_group.hpp): every type's network is Dense(H_t) - Dense(S); H_t and both activations may differ
// between the types.  The W2 / b2 block of the current type is reloaded together with its W0 block.
// The tile body - statistics, normalisation, dense update - and the prologue / epilogue are the tg_* pieces of kernels_train_group.hpp in
// this kernel's form (TrainGroupFormTypes); what is written here is the walk: which rows a tile holds and which network is current.
#pragma once
#include "kernels_train_group.hpp"
#include "kernel_state_lds_types.hpp"

namespace gnn {

constexpr int GROUP_TYPES_MAX_KC = 64;   // constant input columns of one type's network (labels of the type + aggregated component)

// (TypeOffsets and k_group_type_begin: kernel_state_lds_types.hpp - the inference groups of heterogeneous models build the same table)

// ---- constants ---------------------------------------------------------------------------------------------------------------------------
struct GroupTypeNet {
    const float *W, *b, *gamma, *beta;     // first (only) Dense [in_dim][Sw], bias, BatchNormalization (gamma == nullptr: none)
    float eps;
    int act, d_t, in_dim, off_state, off_agg, off_comp;
    float *stats;                          // [G][K][2 in_dim]
};
// ... of the hidden-layer form: W is [in_dim][Hw], `act` the hidden activation
struct GroupTypeNetH : GroupTypeNet {
    int Hw;                                // hidden width, 1 .. the padded width
    const float *W2, *b2;                  // second Dense: [Hw][Sw], [Sw]
    int act2;                              // its activation (the state's)
};
struct GroupTypeWidths { int Hw[GNN_MAX_TYPES]; };      // row length of every type's first kernel = the real columns of its rows of Cc
struct TrainGroupConstTypes {
    int n_types, G, S, Sw, K, W_comp;
    const int *tbeg, *type_nodes;
    const float *nodes; int ld_nodes;
    const float *agg_comp;                 // [N][W_comp]
    float *Cc;                             // [N][S]
    GroupTypeNet net[GNN_MAX_TYPES];
};

__global__ void __launch_bounds__(256) k_train_group_const_types(TrainGroupConstTypes a, GroupTypeWidths hw) {
    __shared__ float red[4][65];
    __shared__ float mu[64], ak[64], ck[64];
    __shared__ int wr[64];
    const int tid = threadIdx.x, g = blockIdx.x;
    const int col = tid & 63, part = tid >> 6;
    for (int t = 0; t < a.n_types; ++t) {
        const int p0 = a.tbeg[t * (a.G + 1) + g], nt = a.tbeg[t * (a.G + 1) + g + 1] - p0;
        if (nt < 1) continue;              // (uniform: the type has no row in this group)
        const GroupTypeNet &n = a.net[t];
        const int *rows = a.type_nodes + p0;
        const int Kc = n.d_t + a.W_comp;   // <= GROUP_TYPES_MAX_KC (the host checked)
        const int Hw = hw.Hw[t];
        // this thread's constant column: the type's labels first, then the aggregated component
        const bool lab = col < n.d_t, has = col < Kc;
        const float *xp = has ? (lab ? a.nodes + col : a.agg_comp + (col - n.d_t)) : nullptr;
        const int ld = lab ? a.ld_nodes : a.W_comp;
        const int kcol = lab ? col : n.off_comp + (col - n.d_t);
        __syncthreads();                   // (the previous type's coefficients have been read)
        if (n.gamma) {
            float s1 = 0.0f;
            if (xp) for (int r = part; r < nt; r += 4) s1 += xp[(size_t)rows[r] * ld];
            red[part][col] = s1;
            __syncthreads();
            if (tid < 64) mu[tid] = (red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid]) / (float)nt;
            __syncthreads();
            const float m = mu[col];
            float s2 = 0.0f;
            if (xp) for (int r = part; r < nt; r += 4) { const float d = xp[(size_t)rows[r] * ld] - m; s2 = fmaf(d, d, s2); }
            red[part][col] = s2;
            __syncthreads();
            if (tid < 64 && has) {
                const float var = (red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid]) / (float)nt;
                wr[tid] = kcol; ak[tid] = n.gamma[kcol] / sqrtf(var + n.eps); ck[tid] = n.beta[kcol];
                for (int t_ = 0; t_ < a.K; ++t_) {
                    float *sl = n.stats + ((size_t)g * a.K + t_) * 2 * n.in_dim;
                    sl[kcol] = mu[tid]; sl[n.in_dim + kcol] = var;
                }
            }
        } else if (tid < 64) { wr[tid] = has ? kcol : 0; mu[tid] = 0.0f; ak[tid] = 1.0f; ck[tid] = 0.0f; }
        __syncthreads();
        for (int i = tid; i < nt * a.S; i += 256) {
            const int h = i % a.S, node = rows[i / a.S];
            float acc = 0.0f;
            if (h < Hw) {
                acc = n.b[h];
                for (int c = 0; c < Kc; ++c) {
                    const float xv = c < n.d_t ? a.nodes[(size_t)node * a.ld_nodes + c] : a.agg_comp[(size_t)node * a.W_comp + (c - n.d_t)];
                    acc = fmaf(fmaf(xv - mu[c], ak[c], ck[c]), n.W[(size_t)wr[c] * Hw + h], acc);
                }
            }
            a.Cc[(size_t)node * a.S + h] = acc;
        }
    }
}

// ---- the loop -------------------------------------------------------------------------------------------------------------------------------
template <class Net>
struct TrainGroupFwdTypesOf : TrainGroupCommon {
    int n_types, G;
    const int *tbeg;             // DEVICE [n_types][G + 1] positions in type_nodes
    const int *type_nodes;       // DEVICE node ids per type, ascending
    Net net[GNN_MAX_TYPES];
};
using TrainGroupFwdTypes = TrainGroupFwdTypesOf<GroupTypeNet>;
using TrainGroupFwdTypesH = TrainGroupFwdTypesOf<GroupTypeNetH>;       // the hidden-layer form (the HID instantiations)

template <int SQ, bool HID = false>
inline size_t train_group_fwd_types_lds(int rows) { return train_group_fwd_lds<SQ, HID>(rows) + 64 * sizeof(int); }

// HID: every state network has a hidden layer (see the header comment); HID = false is the one-layer kernel, unchanged
template <int SQ, bool HAS_W, bool HID = false>
__global__ void __launch_bounds__(TS_NT, 1) k_train_group_fwd_types(std::conditional_t<HID, TrainGroupFwdTypesH, TrainGroupFwdTypes> a) {
    using Csr = TileCsr<SQ, HAS_W, true>;
    using Form = TrainGroupFormTypes;
    constexpr int S = 16 * SQ, LPR = S / 4, NPP = Csr::NPP, NPASS = Csr::NPASS;
    constexpr int LDX = 2 * S + 4, LDS_ST = S + 4;
    extern __shared__ __attribute__((aligned(16))) float tgt_smem[];
    const TrainGroupLds<SQ, HID> L(tgt_smem);  // (Xs: rows of ONE type; W0: the current type's weight rows)
    float *Xs = L.Xs;
    int *rid = reinterpret_cast<int *>(L.rest());         // [64] the tile's rows inside the group
    float *St = L.rest() + 64;            // [ng][LDS_ST] the group's state, by node

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int gi = blockIdx.x;
    const int n0 = a.gbeg[gi], ng = a.gbeg[gi + 1] - n0;
    if (ng < 1 || ng > GROUP_CAP) {       // (the host never launches such a table)
        if (tid == 0) a.k_groups[gi] = -2.0f;
        return;
    }
    const int ntiles = (ng + 63) / 64;
    const bool single = ntiles == 1;

    const bool run = tg_prologue<SQ>(a, St, n0, ng, tid);

    const float no_wreg[1][4][SQ] = {};   // (Form: the weights are re-read from LDS)
    Csr csr;
    csr.bad = 0;
    if (single) csr.load_rows(n0, ng, n0, ng, a.rowptr, a.src, a.w, a.row_scale);
    const __amdgpu_buffer_rsrc_t r_none = buf_rsrc(a.agg);        // (gather<true> reads LDS only)
    int k_done = 0, loaded = -1;
    for (int it = 0; run && it < a.K; ++it) {
        // ---- pass 1: the neighbour sums of every row from the OLD state, parked ------------------------------------------------------------------
        for (int t = 0; t < ntiles; ++t) {
            const int r0 = 64 * t, nr = min(64, ng - r0);
            if (!single) csr.load_rows(n0 + r0, nr, n0, ng, a.rowptr, a.src, a.w, a.row_scale);
            const int q = csr.q, l4 = csr.l4;
            f32x4 acc[NPASS];
            csr.template gather<true>(acc, St, LDS_ST, r_none);
#pragma unroll
            for (int p = 0; p < NPASS; ++p) {
                const int rr = p * NPP + q;
                if (rr < nr) *reinterpret_cast<f32x4 *>(a.agg + (size_t)(n0 + r0 + rr) * S + 4 * l4) = acc[p];
            }
        }
        // ---- type after type: statistics of [state | agg] over the type's rows, then the type's network on them --------------------------------------
        int any = 0;
        for (int ty = 0; ty < a.n_types; ++ty) {
            const int p0 = a.tbeg[ty * (a.G + 1) + gi], nt = a.tbeg[ty * (a.G + 1) + gi + 1] - p0;
            if (nt < 1) continue;         // (uniform: no row of this type in the group - its network is skipped, its statistics stay)
            const auto &net = a.net[ty];
            int Hw = a.Sw, act2 = 0;      // width of the first layer's output (= the kernel's row length); HID: the state's activation
            if constexpr (HID) { Hw = net.Hw; act2 = net.act2; }
            const int *rows = a.type_nodes + p0;
            const int ntl = (nt + 63) / 64;
            const bool bn = net.gamma != nullptr;
            // Rows parked by THIS workgroup in pass 1 (and rows written by the previous type): the barrier orders them at workgroup scope,
            // which is all one workgroup's own stores and loads need (one CU, one vector L1); it also retires the previous type's Xs / W0 reads
            __syncthreads();
            if (loaded != ty) {
                tg_load_weights<SQ>(L.W0, net.W, net.off_state, net.off_agg, a.Sw, Hw, tid);
                if constexpr (HID) tg_load_weights2<SQ>(L, net.W2, net.b2, a.Sw, Hw, tid);
                loaded = ty;
            }
            auto load_tile = [&](int r0, int nr) {
                for (int i = tid; i < 64 * LPR; i += TS_NT) {
                    const int rr = i / LPR, ch = i % LPR;
                    f32x4 own = {0.f, 0.f, 0.f, 0.f}, ag = {0.f, 0.f, 0.f, 0.f};
                    int lr = 0;
                    if (rr < nr) {
                        lr = min(max(rows[r0 + rr] - n0, 0), ng - 1);      // (inside the group whatever the row list says)
                        own = *reinterpret_cast<const f32x4 *>(St + lr * LDS_ST + 4 * ch);
                        ag = *reinterpret_cast<const f32x4 *>(a.agg + (size_t)(n0 + lr) * S + 4 * ch);
                    }
                    *reinterpret_cast<f32x4 *>(Xs + rr * LDX + 4 * ch) = own;
                    *reinterpret_cast<f32x4 *>(Xs + rr * LDX + S + 4 * ch) = ag;
                    if (ch == 0) rid[rr] = lr;
                }
            };
            double S1 = 0.0, S2 = 0.0;
            for (int t = 0; t < ntl && (bn || ntl == 1); ++t) {
                const int r0 = 64 * t, nr = min(64, nt - r0);
                if (t > 0) __syncthreads();                 // (the previous tile's pivots have been read)
                load_tile(r0, nr);
                __syncthreads();
                if (bn) tg_tile_stats<SQ>(L, nr, tid, S1, S2);
            }
            tg_set_norm<SQ, Form>(L, bn, S1, S2, nt, a.Sw, net.off_state, net.off_agg, net.gamma, net.beta, net.eps,
                                  net.stats + ((size_t)gi * a.K + it) * 2 * net.in_dim, net.in_dim, tid);
            __syncthreads();
            for (int t = 0; t < ntl; ++t) {
                const int r0 = 64 * t, nr = min(64, nt - r0);
                if (ntl > 1) {            // (one tile: it is still in Xs, with its rows in rid)
                    if (t > 0) __syncthreads();
                    load_tile(r0, nr);
                    __syncthreads();
                }
                tg_dense_tile<SQ, Form>(L, St, no_wreg, a, n0, rid[16 * wave + c], 16 * wave + c < nr, bn, net.act, wave, c, g, any, Hw, act2);
            }
        }
        k_done = it + 1;
        if (!__syncthreads_or(any)) break;        // (also: the new state is complete before the next gather)
    }
    tg_epilogue<SQ>(a, St, csr.bad, k_done, gi, n0, ng, tid);
}

}  // namespace gnn
