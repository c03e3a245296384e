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
struct TrainGroupConstTypes {
    int n_types, G, S, Sw, K, W_comp;
    const int *tbeg, *type_nodes;
    const float *nodes; int ld_nodes;
    const float *agg_comp;                 // [N][W_comp]
    float *Cc;                             // [N][S]
    GroupTypeNet net[GNN_MAX_TYPES];
};

__global__ void __launch_bounds__(256) k_train_group_const_types(TrainGroupConstTypes a) {
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
            if (h < a.Sw) {
                acc = n.b[h];
                for (int c = 0; c < Kc; ++c) {
                    const float xv = c < n.d_t ? a.nodes[(size_t)node * a.ld_nodes + c] : a.agg_comp[(size_t)node * a.W_comp + (c - n.d_t)];
                    acc = fmaf(fmaf(xv - mu[c], ak[c], ck[c]), n.W[(size_t)wr[c] * a.Sw + h], acc);
                }
            }
            a.Cc[(size_t)node * a.S + h] = acc;
        }
    }
}

// ---- the loop -------------------------------------------------------------------------------------------------------------------------------
struct TrainGroupFwdTypes {
    int S, Sw, K, n_types, G;    // S = padded width (16 SQ), Sw the state's real width
    const int *rowptr, *src; const float *w, *row_scale;       // adjacency by destination (merged graph)
    const int *gbeg;             // DEVICE [G + 1]
    const int *tbeg;             // DEVICE [n_types][G + 1] positions in type_nodes
    const int *type_nodes;       // DEVICE node ids per type, ascending
    const float *state0; int ld0;
    float *state_out;            // [N][Sw]
    float *agg;                  // [N][S] parked neighbour sums; written and read by the owning workgroup only
    const float *Cc;             // [N][S]
    float thr;
    float *k_groups;             // [G]
    GroupTypeNet net[GNN_MAX_TYPES];
};

template <int SQ>
inline size_t train_group_fwd_types_lds(int rows) { return train_group_fwd_lds<SQ>(rows) + 64 * sizeof(int); }

template <int SQ, bool HAS_W>
__global__ void __launch_bounds__(TS_NT, 1) k_train_group_fwd_types(TrainGroupFwdTypes a) {
    using Csr = TileCsr<SQ, HAS_W, true>;
    constexpr int S = 16 * SQ, LPR = S / 4, NPP = Csr::NPP, NPASS = Csr::NPASS;
    constexpr int LDX = 2 * S + 4, LDW = S + 4, LDS_ST = S + 4;
    extern __shared__ __attribute__((aligned(16))) float tgt_smem[];
    float *Xs = tgt_smem;                 // [64][LDX]  [own | agg] of the current tile (rows of ONE type)
    float *W0 = Xs + 64 * LDX;            // [2 S][LDW] the current type's state / agg weight rows
    float *st_a = W0 + 2 * S * LDW;       // [2 S] a_k | beta_k | column means | reduction scratch [512] | tile sums [4 S]
    float *st_c = st_a + 2 * S, *piv = st_c + 2 * S, *red = piv + 2 * S, *fin = red + 512;
    int *rid = reinterpret_cast<int *>(fin + 4 * S);      // [64] the tile's rows inside the group
    float *St = fin + 4 * S + 64;         // [ng][LDS_ST] the group's state, by node

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

    for (int i = tid; i < ng * LDS_ST; i += TS_NT) {
        const int r = i / LDS_ST, h = i % LDS_ST;
        St[i] = h < a.Sw ? a.state0[(size_t)(n0 + r) * a.ld0 + h] : 0.0f;
    }
    __syncthreads();
    // the predicate of state_0 against a state of ones (reference GNN.py:256: state_old = ones_like(state))
    int any0 = 0;
    for (int r = tid; r < ng; r += TS_NT) {
        float d2 = 0.0f;
        for (int h = 0; h < a.Sw; ++h) { const float d = St[r * LDS_ST + h] - 1.0f; d2 = fmaf(d, d, d2); }
        if (sqrtf(d2) > a.thr * sqrtf((float)a.Sw)) any0 = 1;
    }
    const bool run = __syncthreads_or(any0) != 0;

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
            const GroupTypeNet &net = a.net[ty];
            const int *rows = a.type_nodes + p0;
            const int ntl = (nt + 63) / 64;
            const bool bn = net.gamma != nullptr;
            // Rows parked by THIS workgroup in pass 1 (and rows written by the previous type): the barrier orders them at workgroup scope,
            // which is all one workgroup's own stores and loads need (one CU, one vector L1); it also retires the previous type's Xs / W0 reads
            __syncthreads();
            if (loaded != ty) {
                for (int i = tid; i < 2 * S * S; i += TS_NT) {
                    const int k = i / S, h = i % S;
                    const int kk = k < S ? k : k - S;
                    W0[k * LDW + h] = (kk < a.Sw && h < a.Sw) ? net.W[(size_t)((k < S ? net.off_state : net.off_agg) + kk) * a.Sw + h] : 0.0f;
                }
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
                if (bn) {
                    const int col = tid & (2 * S - 1), part_i = tid / (2 * S);
                    constexpr int NG = TS_NT / (2 * S), RPG = 64 / NG;
                    float s1 = 0.0f, s2 = 0.0f;
                    const float pv = Xs[col];
                    float xr[RPG];
#pragma unroll
                    for (int u = 0; u < RPG; ++u) xr[u] = Xs[(part_i * RPG + u) * LDX + col];
#pragma unroll
                    for (int u = 0; u < RPG; ++u) {
                        const float x = part_i * RPG + u < nr ? xr[u] - pv : 0.0f;
                        s1 += x; s2 = fmaf(x, x, s2);
                    }
                    red[part_i * 4 * S + col] = s1; red[part_i * 4 * S + 2 * S + col] = s2;
                    __syncthreads();
                    if (tid < 4 * S) {
                        float tt = 0.0f;
#pragma unroll
                        for (int gq = 0; gq < NG; ++gq) tt += red[gq * 4 * S + tid];
                        fin[tid] = tt;
                    }
                    __syncthreads();
                    if (tid < 2 * S) {        // the tile's share moved to the origin and added in double (merge_tile_stats)
                        const double nj = (double)nr, p_ = (double)Xs[tid], a1 = (double)fin[tid];
                        S1 += a1 + nj * p_;
                        S2 += (double)fin[2 * S + tid] + p_ * (2.0 * a1 + nj * p_);
                    }
                }
            }
            if (tid < 2 * S) {
                const int kk = tid < S ? tid : tid - S;
                float ak = 1.0f, ck = 0.0f, mu = 0.0f;
                if (bn) {
                    ak = 0.0f;
                    if (kk < a.Sw) {
                        const int k = (tid < S ? net.off_state : net.off_agg) + kk;
                        const double mean = S1 / (double)nt;
                        mu = (float)mean;
                        const float va = (float)fmax(S2 / (double)nt - mean * mean, 0.0);
                        ak = net.gamma[k] / sqrtf(va + net.eps); ck = net.beta[k];
                        float *sl = net.stats + ((size_t)gi * a.K + it) * 2 * net.in_dim;
                        sl[k] = mu; sl[net.in_dim + k] = va;
                    }
                }
                st_a[tid] = ak; st_c[tid] = ck; piv[tid] = mu;
            }
            __syncthreads();
            for (int t = 0; t < ntl; ++t) {
                const int r0 = 64 * t, nr = min(64, nt - r0);
                if (ntl > 1) {            // (one tile: it is still in Xs, with its rows in rid)
                    if (t > 0) __syncthreads();
                    load_tile(r0, nr);
                    __syncthreads();
                }
                const bool oin = 16 * wave + c < nr;
                const int lrow = rid[16 * wave + c];
                f32x4 acc[SQ];
#pragma unroll
                for (int ct = 0; ct < SQ; ++ct)
                    acc[ct] = oin ? *reinterpret_cast<const f32x4 *>(a.Cc + (size_t)(n0 + lrow) * S + 16 * ct + 4 * g) : (f32x4){0.f, 0.f, 0.f, 0.f};
                const float *xrow = Xs + (16 * wave + c) * LDX + 4 * g;
#pragma unroll
                for (int qq = 0; qq < 2 * S / 16; ++qq) {
                    f32x4 xv = *reinterpret_cast<const f32x4 *>(xrow + 16 * qq);
                    const f32x4 av = *reinterpret_cast<const f32x4 *>(st_a + 16 * qq + 4 * g), cv = *reinterpret_cast<const f32x4 *>(st_c + 16 * qq + 4 * g);
                    const f32x4 mv = *reinterpret_cast<const f32x4 *>(piv + 16 * qq + 4 * g);
#pragma unroll
                    for (int e = 0; e < 4; ++e) xv[e] = fmaf(xv[e] - mv[e], av[e], cv[e]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float *wr = W0 + (16 * qq + 4 * g + e) * LDW + c;
#pragma unroll
                        for (int ct = 0; ct < SQ; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[16 * ct], xv[e], acc[ct], 0, 0, 0);
                    }
                }
                asm volatile("s_nop 15\n\ts_nop 3" ::: "memory");          // (MFMA results consumed behind a branch: see kernels_train_big.hpp)
                float d2 = 0.0f, n2 = 0.0f;
                const float *old_lds = Xs + (16 * wave + c) * LDX + 4 * g;
                float *new_lds = St + lrow * LDS_ST + 4 * g;
#pragma unroll
                for (int ct = 0; ct < SQ; ++ct) {
                    f32x4 v = acc[ct];
                    activate4(net.act, v);
                    const f32x4 o = *reinterpret_cast<const f32x4 *>(old_lds + 16 * ct);
#pragma unroll
                    for (int e = 0; e < 4; ++e) { v[e] = (oin && 16 * ct + 4 * g + e < a.Sw) ? v[e] : 0.0f; const float d = v[e] - o[e]; d2 = fmaf(d, d, d2); n2 = fmaf(o[e], o[e], n2); }
                    if (oin) *reinterpret_cast<f32x4 *>(new_lds + 16 * ct) = v;
                }
                d2 += __shfl_xor(d2, 16, 64); d2 += __shfl_xor(d2, 32, 64);
                n2 += __shfl_xor(n2, 16, 64); n2 += __shfl_xor(n2, 32, 64);
                if (oin && sqrtf(d2) > a.thr * sqrtf(n2)) any = 1;
            }
        }
        k_done = it + 1;
        if (!__syncthreads_or(any)) break;        // (also: the new state is complete before the next gather)
    }
    const int bad = __syncthreads_or(csr.bad);
    for (int i = tid; i < ng * a.Sw; i += TS_NT) {
        const int r = i / a.Sw, h = i % a.Sw;
        a.state_out[(size_t)(n0 + r) * a.Sw + h] = St[r * LDS_ST + h];
    }
    if (tid == 0) a.k_groups[gi] = bad ? -1.0f : (float)k_done;
}

}  // namespace gnn
