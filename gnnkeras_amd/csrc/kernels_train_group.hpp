// Training-mode forward with independent CONVERGENCE GROUPS (C ABI 10: gnn_train_args_t::group_node_begin with forward_only): a merged,
// block-diagonal batch of G graphs, every graph computed "as if it had been called alone" - BatchNormalization on the column statistics
// of ITS rows, its own predicate, its own k - in one launch per stage.  What a serial LGNN fit() runs between two layers on every single
// graph (reference LGNN.py:325-337).
//
// k_train_small_fwd<.., LOCAL = true> (kernels_train_small.hpp) shares two things between its tiles through a grid barrier: the
// BatchNormalization partials and the loop condition.  With one GROUP per workgroup both are workgroup-local, so these kernels have no
// cross-workgroup wait at all: no residency requirement, any number of groups per launch, no bounded wait that could expire.
//
//   k_train_group_const   per group: statistics of the constant input columns over the group's rows, then the rows' constant part Cc
//   k_train_group_fwd     per group: the state of the group (<= GROUP_CAP rows) lives in LDS for the whole loop; the workgroup walks the
//                         group's 64-row tiles in turn, twice per iteration:
//                           pass 1  [own | neighbour sum] of the tile -> LDS; column sums around the tile's first row (float32), merged
//                                   in double as merge_tile_stats does - but inside the workgroup; a group of several tiles parks the
//                                   neighbour sums in memory (the new rows of tile 0 must not be seen by the gather of tile 1)
//                           pass 2  (a (x - mean) + beta) . W + Cc on v_mfma_f32_16x16x4_f32 (operand layout of k_train_small_fwd),
//                                   activation, predicate, rows back into the LDS state - in place: row r depends on row r of pass 1 only
//   k_train_group_head    per group: column statistics of the output network's input over the group's output rows, centred
//                         normalisation, one Dense of <= 64 units, activation / softmax
//   k_bn_moving_groups    the ordered part: moving <- 0.99 moving + 0.01 batch, group after group, iteration after iteration - the literal
//                         recurrence, one thread per column
// A forward keeps no tape: the workspace is O(N S) (Cc, parked neighbour sums) plus the statistics slots [G][K][2 in_s].
//
// The body of k_train_group_fwd is written as tg_* pieces (LDS carve, prologue, tile statistics, normalisation, dense update, epilogue)
// that k_train_group_fwd_types (kernels_train_group_types.hpp: one state network per node type) is made of as well.
//
// Hidden-layer form (template parameter HID; opt-in through GNN_FLAG_TRAIN_GROUPS_HIDDEN, both model kinds; the rule is
// train_groups_hidden_net() in train_group.hpp): the state network is Dense(H) - Dense(S), 1 <= H <= the padded width, padded width 16 / 32.
// BatchNormalization sits in front of the first Dense only, so the statistics, the normalisation and the head are the one-layer form's.  The
// first kernel is [in_s][Hw] (Cc has Hw real columns); the first product leaves lane (c, g) holding columns 16 ct + 4 g .. + 3 of tile row
// c - exactly the B operand of k-step (ct, e) of a second v_mfma_f32_16x16x4_f32 product - so h . W2 runs from the first product's
// accumulators: no transposition, no trip of h through LDS, no barrier.  W2 ([S][S + 4]: rows >= Hw and columns >= Sw zero) and b2 sit in
// LDS behind `fin`, in front of the state rows.  The one-layer instantiations (HID = false) are the kernels they were: the hidden form's
// arguments travel in derived structs (TrainGroupFwdH, GroupTypeNetH), read under `if constexpr`.
#pragma once
#include "kernels_train_small.hpp"

namespace gnn {

constexpr int GROUP_CAP = 256;           // rows of a group's state in LDS: 256 x 68 floats + weights + one [own | agg] tile = 138 KB at width 64
constexpr int GROUP_HEAD_MAX_IN = 256;   // input columns of the output network (one thread per column takes the statistics)
constexpr int GROUP_HEAD_MAX_UNITS = 64;

// ---- constants ---------------------------------------------------------------------------------------------------------------------------
// One workgroup per group.  stats[g][t][wrow] / [in_s + wrow] (all K slots: the constants' statistics do not change between iterations)
// Hw: the row length of the first kernel = the real columns of Cc (the state's width; the hidden width in the hidden-layer form)
__global__ void __launch_bounds__(256)
k_train_group_const(const int *__restrict__ gbeg, int S, int Hw, ConstSegs cs, const float *__restrict__ W, const float *__restrict__ b, const float *gamma,
                    const float *beta, float eps, float *__restrict__ Cc, float *__restrict__ stats, int K, int in_s) {
    __shared__ float red[8][33];
    __shared__ float mu[32], ak[32], ck[32];
    __shared__ int wr[32];
    const int tid = threadIdx.x, g = blockIdx.x;
    const int n0 = gbeg[g], ng = gbeg[g + 1] - n0;
    int Kc = 0;
    for (int s = 0; s < cs.n; ++s) Kc += cs.width[s];
    if (gamma && Kc > 0) {
        const int col = tid & 31, part = tid >> 5;
        // this thread's constant column: segment, column inside it, BatchNorm column
        int sg = -1, j = 0, c0 = 0;
        for (int s = 0; s < cs.n; ++s) { if (col >= c0 && col < c0 + cs.width[s]) { sg = s; j = col - c0; } c0 += cs.width[s]; }
        const float *xp = sg >= 0 ? cs.ptr[sg] + (size_t)n0 * cs.ld[sg] + j : nullptr;
        const int ld = sg >= 0 ? cs.ld[sg] : 0;
        float s1 = 0.0f;
        if (xp) for (int r = part; r < ng; r += 8) s1 += xp[(size_t)r * ld];
        red[part][col] = s1;
        __syncthreads();
        if (tid < 32) { float t = 0.0f; for (int p = 0; p < 8; ++p) t += red[p][tid]; mu[tid] = t / (float)ng; }
        __syncthreads();
        const float m = mu[col];
        float s2 = 0.0f;
        if (xp) for (int r = part; r < ng; r += 8) { const float d = xp[(size_t)r * ld] - m; s2 = fmaf(d, d, s2); }
        red[part][col] = s2;
        __syncthreads();
        if (tid < 32 && tid < Kc) {
            float t = 0.0f;
            for (int p = 0; p < 8; ++p) t += red[p][tid];
            const float var = t / (float)ng;
            const int k = cs.wrow[sg] + j;             // (tid == col for these threads)
            wr[tid] = k; ak[tid] = gamma[k] / sqrtf(var + eps); ck[tid] = beta[k];
            for (int t_ = 0; t_ < K; ++t_) {
                float *sl = stats + ((size_t)g * K + t_) * 2 * in_s;
                sl[k] = mu[tid]; sl[in_s + k] = var;
            }
        }
        __syncthreads();
    } else {
        if (tid < 32) {
            int sg = 0, j = 0, c0 = 0;
            for (int s = 0; s < cs.n; ++s) { if (tid >= c0 && tid < c0 + cs.width[s]) { sg = s; j = tid - c0; } c0 += cs.width[s]; }
            wr[tid] = tid < Kc ? cs.wrow[sg] + j : 0; mu[tid] = 0.0f; ak[tid] = 1.0f; ck[tid] = 0.0f;
        }
        __syncthreads();
    }
    for (int i = tid; i < ng * S; i += 256) {
        const int h = i % S, n = n0 + i / S;
        float acc = 0.0f;
        if (h < Hw) {
            acc = b[h];
            int col = 0;
            for (int s = 0; s < cs.n; ++s)
                for (int j = 0; j < cs.width[s]; ++j, ++col) {
                    const float x = fmaf(cs.ptr[s][(size_t)n * cs.ld[s] + j] - mu[col], ak[col], ck[col]);
                    acc = fmaf(x, W[(size_t)wr[col] * Hw + h], acc);
                }
        }
        Cc[(size_t)n * S + h] = acc;
    }
}

// ---- the loop -------------------------------------------------------------------------------------------------------------------------------
// What k_train_group_fwd and k_train_group_fwd_types (kernels_train_group_types.hpp) are both made of: the tg_* pieces below.  The two kernels
// differ in which rows a tile holds (a contiguous range of the group, or a type's row list), in which network is current, and in the
// compile-time FORM of each side:
//     WREG               the weight block sits in registers (SQ <= 2) - otherwise every product re-reads it from LDS
//     NORM_WITHOUT_BN    a network without BatchNormalization still runs the normalisation, with a = 1, c = 0, mean = 0 - otherwise it is skipped
//     DIVIDE_BY_ROWS     mean = S1 / rows - otherwise S1 * (1 / rows)
// Each kernel keeps the form it has always had: the results are the same bits as before the pieces were shared.
struct TrainGroupFormRange { static constexpr bool NORM_WITHOUT_BN = false, DIVIDE_BY_ROWS = false; template <int SQ> static constexpr bool WREG = SQ <= 2; };
struct TrainGroupFormTypes { static constexpr bool NORM_WITHOUT_BN = true, DIVIDE_BY_ROWS = true; template <int SQ> static constexpr bool WREG = false; };

struct TrainGroupCommon {        // the fields both argument structs share
    int S, Sw, K;                // S = padded width (16 SQ), Sw the state's real width
    const int *rowptr, *src; const float *w, *row_scale;       // adjacency by destination (merged graph)
    const int *gbeg;             // DEVICE [G + 1]
    const float *state0; int ld0;// [N][ld0]: state_0 in the first Sw columns
    float *state_out;            // [N][Sw]
    float *agg;                  // [N][S] parked neighbour sums; written and read by the owning workgroup only
    const float *Cc;             // [N][S]
    float thr;
    float *k_groups;             // [G]: iterations executed; -1: an arc leaves the group (every result of the group is invalid)
};
struct TrainGroupFwd : TrainGroupCommon {
    float *stats;                // [G][K][2 in_s]
    int in_s, off_agg;
    const float *W, *gamma, *beta; float eps;
    int act;
};
// ... of the hidden-layer form (the HID instantiations): W is [in_s][Hw], Cc has Hw real columns, `act` is the hidden activation
struct TrainGroupFwdH : TrainGroupFwd {
    int Hw;                      // hidden width, 1 .. 16 SQ
    const float *W2, *b2;        // second Dense: [Hw][Sw], [Sw]
    int act2;                    // its activation (the state's)
};

template <int SQ, bool HID = false>
inline size_t train_group_fwd_lds(int rows) {          // rows = the largest group of the launch (<= GROUP_CAP)
    constexpr int S = 16 * SQ;
    return sizeof(float) * (64 * (2 * S + 4) + (2 * S) * (S + 4) + 3 * 2 * S + 512 + 4 * S + (HID ? S * (S + 4) + S : 0) + (size_t)rows * (S + 4));
}

// the LDS of a workgroup in the order of train_group_fwd_lds: everything but the state, which follows at rest()
template <int SQ, bool HID = false>
struct TrainGroupLds {
    static constexpr int S = 16 * SQ, LDX = 2 * S + 4, LDW = S + 4, LDS_ST = S + 4;
    float *Xs;                   // [64][LDX]  [own | agg] of the current tile
    float *W0;                   // [2 S][LDW] the current network's state / agg weight rows
    float *st_a, *st_c, *piv;    // [2 S] each: a_k | beta_k | column means
    float *red, *fin;            // reduction scratch [512] | tile sums [4 S]
    __device__ __forceinline__ explicit TrainGroupLds(float *smem)
        : Xs(smem), W0(Xs + 64 * LDX), st_a(W0 + 2 * S * LDW), st_c(st_a + 2 * S), piv(st_c + 2 * S), red(piv + 2 * S), fin(red + 512) {}
    __device__ __forceinline__ float *W2s() const { return fin + 4 * S; }        // HID: [S][LDW] the current network's second kernel
    __device__ __forceinline__ float *b2s() const { return W2s() + S * LDW; }    // HID: [S] its bias
    __device__ __forceinline__ float *rest() const { return fin + 4 * S + (HID ? S * LDW + S : 0); }
};

// the [2 S][LDW] weight block of one network: its state rows, then its neighbour-sum rows.  Hw: the kernel's row length (the state's width
// Sw; the hidden width in the hidden-layer form)
template <int SQ>
__device__ __forceinline__ void tg_load_weights(float *W0, const float *W, int off_state, int off_agg, int Sw, int Hw, int tid) {
    constexpr int S = 16 * SQ, LDW = S + 4;
    for (int i = tid; i < 2 * S * S; i += TS_NT) {
        const int k = i / S, h = i % S;
        const int kk = k < S ? k : k - S;
        W0[k * LDW + h] = (kk < Sw && h < Hw) ? W[(size_t)((k < S ? off_state : off_agg) + kk) * Hw + h] : 0.0f;
    }
}
// hidden-layer form: the second kernel [Hw][Sw] as [S][LDW] rows (rows >= Hw and columns >= Sw zero) and its bias - the pitch of W0, for
// the same conflict-free A-operand reads
template <int SQ>
__device__ __forceinline__ void tg_load_weights2(const TrainGroupLds<SQ, true> &L, const float *W2, const float *b2, int Sw, int Hw, int tid) {
    constexpr int S = 16 * SQ, LDW = S + 4;
    float *W2s = L.W2s(), *b2s = L.b2s();
    for (int i = tid; i < S * S; i += TS_NT) {
        const int k = i / S, h = i % S;
        W2s[k * LDW + h] = (k < Hw && h < Sw) ? W2[(size_t)k * Sw + h] : 0.0f;
    }
    if (tid < S) b2s[tid] = tid < Sw ? b2[tid] : 0.0f;
}

// state_0 of the group into LDS; whether the loop runs at all
template <int SQ>
__device__ __forceinline__ bool tg_prologue(const TrainGroupCommon &a, float *St, int n0, int ng, int tid) {
    constexpr int LDS_ST = 16 * SQ + 4;
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
    return __syncthreads_or(any0) != 0;
}

// the tile in Xs (nr rows) adds its share to the column sums S1 / S2 of thread tid < 2 S: float32 sums around the tile's first row, moved
// to the origin and added in double (merge_tile_stats)
template <int SQ, bool HID>
__device__ __forceinline__ void tg_tile_stats(const TrainGroupLds<SQ, HID> &L, int nr, int tid, double &S1, double &S2) {
    constexpr int S = 16 * SQ, LDX = 2 * S + 4;
    const int col = tid & (2 * S - 1), part_i = tid / (2 * S);
    constexpr int NG = TS_NT / (2 * S), RPG = 64 / NG;
    float s1 = 0.0f, s2 = 0.0f;
    const float pv = L.Xs[col];
    float xr[RPG];
#pragma unroll
    for (int u = 0; u < RPG; ++u) xr[u] = L.Xs[(part_i * RPG + u) * LDX + col];
#pragma unroll
    for (int u = 0; u < RPG; ++u) {
        const float x = part_i * RPG + u < nr ? xr[u] - pv : 0.0f;
        s1 += x; s2 = fmaf(x, x, s2);
    }
    L.red[part_i * 4 * S + col] = s1; L.red[part_i * 4 * S + 2 * S + col] = s2;
    __syncthreads();
    if (tid < 4 * S) {
        float tt = 0.0f;
#pragma unroll
        for (int gq = 0; gq < NG; ++gq) tt += L.red[gq * 4 * S + tid];
        L.fin[tid] = tt;
    }
    __syncthreads();
    if (tid < 2 * S) {
        const double nj = (double)nr, p_ = (double)L.Xs[tid], a1 = (double)L.fin[tid];
        S1 += a1 + nj * p_;
        S2 += (double)L.fin[2 * S + tid] + p_ * (2.0 * a1 + nj * p_);
    }
}

// S1 / S2 over `rows` rows -> the normalisation st_a (x - piv) + st_c of the current network, and the iteration's statistics slot `sl`
// [2 in_dim].  Column tid < S is weight row off_state + tid, column S + kk weight row off_agg + kk.
template <int SQ, class Form, bool HID>
__device__ __forceinline__ void tg_set_norm(const TrainGroupLds<SQ, HID> &L, bool bn, double S1, double S2, int rows, int Sw, int off_state, int off_agg,
                                            const float *gamma, const float *beta, float eps, float *sl, int in_dim, int tid) {
    constexpr int S = 16 * SQ;
    if (!Form::NORM_WITHOUT_BN && !bn) return;
    if (tid < 2 * S) {
        const int kk = tid < S ? tid : tid - S;
        float ak = bn ? 0.0f : 1.0f, ck = 0.0f, mu = 0.0f;
        if (bn && kk < Sw) {
            const int k = (tid < S ? off_state : off_agg) + kk;
            const double inv_rows = 1.0 / (double)rows;
            const double mean = Form::DIVIDE_BY_ROWS ? S1 / (double)rows : S1 * inv_rows;
            mu = (float)mean;
            const float va = (float)fmax((Form::DIVIDE_BY_ROWS ? S2 / (double)rows : S2 * inv_rows) - mean * mean, 0.0);
            ak = gamma[k] / sqrtf(va + eps); ck = beta[k];
            sl[k] = mu; sl[in_dim + k] = va;
        }
        L.st_a[tid] = ak; L.st_c[tid] = ck; L.piv[tid] = mu;
    }
}

// The dense update of the tile in Xs: (a (x - mean) + beta) . W + Cc on v_mfma_f32_16x16x4_f32 (operand layout of k_train_small_fwd),
// activation, predicate; this lane's row (row 16 wave + c of the tile, `oin`: it is a row) goes back into the LDS state at row lrow of the
// group - in place: it depends on the same row of the old state only.
// HID: `act` is the hidden activation, h = act(..) with the columns at or past Hw zeroed, then act2(h . W2 + b2) from the block at L.W2s().
template <int SQ, class Form, bool HID>
__device__ __forceinline__ void tg_dense_tile(const TrainGroupLds<SQ, HID> &L, float *St, const float (&wreg)[Form::template WREG<SQ> ? 2 * SQ : 1][4][SQ],
                                              const TrainGroupCommon &a, int n0, int lrow, bool oin, bool bn, int act, int wave, int c, int g, int &any,
                                              int Hw = 0, int act2 = 0) {
    constexpr int S = 16 * SQ, LDX = 2 * S + 4, LDW = S + 4, LDS_ST = S + 4;
    constexpr bool WREG = Form::template WREG<SQ>;
    f32x4 acc[SQ];
#pragma unroll
    for (int ct = 0; ct < SQ; ++ct)
        acc[ct] = oin ? *reinterpret_cast<const f32x4 *>(a.Cc + (size_t)(n0 + lrow) * S + 16 * ct + 4 * g) : (f32x4){0.f, 0.f, 0.f, 0.f};
    const float *xrow = L.Xs + (16 * wave + c) * LDX + 4 * g;
#pragma unroll
    for (int qq = 0; qq < 2 * S / 16; ++qq) {
        f32x4 xv = *reinterpret_cast<const f32x4 *>(xrow + 16 * qq);
        if (Form::NORM_WITHOUT_BN || bn) {
            const f32x4 av = *reinterpret_cast<const f32x4 *>(L.st_a + 16 * qq + 4 * g), cv = *reinterpret_cast<const f32x4 *>(L.st_c + 16 * qq + 4 * g);
            const f32x4 mv = *reinterpret_cast<const f32x4 *>(L.piv + 16 * qq + 4 * g);
#pragma unroll
            for (int e = 0; e < 4; ++e) xv[e] = fmaf(xv[e] - mv[e], av[e], cv[e]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float *wr = L.W0 + (16 * qq + 4 * g + e) * LDW + c;
#pragma unroll
            for (int ct = 0; ct < SQ; ++ct)
                acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(WREG ? wreg[WREG ? qq : 0][e][ct] : wr[16 * ct], xv[e], acc[ct], 0, 0, 0);
        }
    }
    asm volatile("s_nop 15\n\ts_nop 3" ::: "memory");          // (MFMA results consumed behind a branch: see kernels_train_big.hpp)
    if constexpr (HID) {
        // lane (c, g) holds columns 16 qq + 4 g + e of row c of ITS wave - the B operand of k-step (qq, e): h goes from the accumulators
        // into the second product as it is.  Columns at or past Hw are zeroed (act(0) != 0 for sigmoid / softplus), whatever W2's rows hold
        const float *W2s = L.W2s(), *b2s = L.b2s();
        f32x4 hv[SQ];
#pragma unroll
        for (int ct = 0; ct < SQ; ++ct) {
            hv[ct] = acc[ct];
            activate4(act, hv[ct]);
#pragma unroll
            for (int e = 0; e < 4; ++e) hv[ct][e] = 16 * ct + 4 * g + e < Hw ? hv[ct][e] : 0.0f;
            acc[ct] = *reinterpret_cast<const f32x4 *>(b2s + 16 * ct + 4 * g);
        }
#pragma unroll
        for (int qq = 0; qq < SQ; ++qq)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float *wr = W2s + (16 * qq + 4 * g + e) * LDW + c;
#pragma unroll
                for (int ct = 0; ct < SQ; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[16 * ct], hv[qq][e], acc[ct], 0, 0, 0);
            }
        asm volatile("s_nop 15\n\ts_nop 3" ::: "memory");
    }
    const int act_out = HID ? act2 : act;
    float d2 = 0.0f, n2 = 0.0f;
    const float *old_lds = L.Xs + (16 * wave + c) * LDX + 4 * g;
    float *new_lds = St + lrow * LDS_ST + 4 * g;
#pragma unroll
    for (int ct = 0; ct < SQ; ++ct) {
        f32x4 v = acc[ct];
        activate4(act_out, v);
        const f32x4 o = *reinterpret_cast<const f32x4 *>(old_lds + 16 * ct);
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[e] = (oin && 16 * ct + 4 * g + e < a.Sw) ? v[e] : 0.0f; const float d = v[e] - o[e]; d2 = fmaf(d, d, d2); n2 = fmaf(o[e], o[e], n2); }
        if (oin) *reinterpret_cast<f32x4 *>(new_lds + 16 * ct) = v;
    }
    d2 += __shfl_xor(d2, 16, 64); d2 += __shfl_xor(d2, 32, 64);
    n2 += __shfl_xor(n2, 16, 64); n2 += __shfl_xor(n2, 32, 64);
    if (oin && sqrtf(d2) > a.thr * sqrtf(n2)) any = 1;
}

// the group's state and its k go out; `csr_bad`: this thread met an arc that leaves the group
template <int SQ>
__device__ __forceinline__ void tg_epilogue(const TrainGroupCommon &a, const float *St, int csr_bad, int k_done, int gi, int n0, int ng, int tid) {
    constexpr int LDS_ST = 16 * SQ + 4;
    const int bad = __syncthreads_or(csr_bad);
    for (int i = tid; i < ng * a.Sw; i += TS_NT) {
        const int r = i / a.Sw, h = i % a.Sw;
        a.state_out[(size_t)(n0 + r) * a.Sw + h] = St[r * LDS_ST + h];
    }
    if (tid == 0) a.k_groups[gi] = bad ? -1.0f : (float)k_done;
}

// HID: the state network has a hidden layer (see the header comment); HID = false is the one-layer kernel, unchanged
template <int SQ, bool HAS_W, bool HID = false>
__global__ void __launch_bounds__(TS_NT, 1) k_train_group_fwd(std::conditional_t<HID, TrainGroupFwdH, TrainGroupFwd> a) {
    using Csr = TileCsr<SQ, HAS_W, true>;
    using Form = TrainGroupFormRange;
    constexpr int S = 16 * SQ, LPR = S / 4, NPP = Csr::NPP, NPASS = Csr::NPASS;
    constexpr int LDX = 2 * S + 4, LDW = S + 4, LDS_ST = S + 4;
    extern __shared__ __attribute__((aligned(16))) float tg_smem[];
    const TrainGroupLds<SQ, HID> L(tg_smem);
    float *Xs = L.Xs, *W0 = L.W0;
    float *St = L.rest();                 // [ng][LDS_ST] the group's state
    int Hw = a.Sw, act2 = 0;              // width of the first layer's output (= the kernel's row length); HID: the state's activation
    if constexpr (HID) { Hw = a.Hw; act2 = a.act2; }

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
    const bool bn = a.gamma != nullptr;

    tg_load_weights<SQ>(W0, a.W, 0, a.off_agg, a.Sw, Hw, tid);
    if constexpr (HID) tg_load_weights2<SQ>(L, a.W2, a.b2, a.Sw, Hw, tid);
    if (tid < 2 * S) { L.piv[tid] = 0.0f; L.st_a[tid] = 1.0f; L.st_c[tid] = 0.0f; }
    const bool run = tg_prologue<SQ>(a, St, n0, ng, tid);

    constexpr bool WREG = Form::WREG<SQ>;
    float wreg[WREG ? 2 * S / 16 : 1][4][SQ];
    if (WREG) {
#pragma unroll
        for (int qq = 0; qq < 2 * S / 16; ++qq)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int ct = 0; ct < SQ; ++ct) wreg[WREG ? qq : 0][e][ct] = W0[(16 * qq + 4 * g + e) * LDW + c + 16 * ct];
    }
    Csr csr;
    csr.bad = 0;
    if (single) csr.load_rows(n0, ng, n0, ng, a.rowptr, a.src, a.w, a.row_scale);
    const __amdgpu_buffer_rsrc_t r_none = buf_rsrc(a.agg);        // (gather<true> reads LDS only)
    int k_done = 0;
    for (int it = 0; run && it < a.K; ++it) {
        // ---- pass 1: neighbour sums of every tile from the OLD state; column statistics of [state | agg] over the group's rows -----------------
        double S1 = 0.0, S2 = 0.0;
        for (int t = 0; t < ntiles; ++t) {
            const int r0 = 64 * t, nr = min(64, ng - r0);
            if (!single) csr.load_rows(n0 + r0, nr, n0, ng, a.rowptr, a.src, a.w, a.row_scale);
            const int q = csr.q, l4 = csr.l4;
            f32x4 acc[NPASS];
            csr.template gather<true>(acc, St, LDS_ST, r_none);
            if (t > 0) __syncthreads();                     // (the previous tile's pivots have been read)
#pragma unroll
            for (int p = 0; p < NPASS; ++p) {
                const int rr = p * NPP + q;
                float *xr = Xs + rr * LDX + 4 * l4;
                f32x4 own = {0.f, 0.f, 0.f, 0.f};
                if (rr < nr) own = *reinterpret_cast<const f32x4 *>(St + (r0 + rr) * LDS_ST + 4 * l4);
                *reinterpret_cast<f32x4 *>(xr) = own;
                *reinterpret_cast<f32x4 *>(xr + S) = acc[p];
                if (!single && rr < nr) *reinterpret_cast<f32x4 *>(a.agg + (size_t)(n0 + r0 + rr) * S + 4 * l4) = acc[p];
            }
            __syncthreads();
            if (bn) tg_tile_stats<SQ>(L, nr, tid, S1, S2);
        }
        tg_set_norm<SQ, Form>(L, bn, S1, S2, ng, a.Sw, 0, a.off_agg, a.gamma, a.beta, a.eps, a.stats + ((size_t)gi * a.K + it) * 2 * a.in_s, a.in_s, tid);
        __syncthreads();
        // ---- pass 2: (a (x - mean) + beta) . W + Cc, activation, predicate; the new rows replace the old ones in the LDS state -----------------
        int any = 0;
        for (int t = 0; t < ntiles; ++t) {
            const int r0 = 64 * t, nr = min(64, ng - r0);
            if (!single) {
                // Rows parked by THIS workgroup in pass 1: the barriers in between order them at workgroup scope, which is all one
                // workgroup's own stores and loads need (one CU, one vector L1)
                if (t > 0) __syncthreads();
                for (int i = tid; i < 64 * LPR; i += TS_NT) {
                    const int rr = i / LPR, ch = i % LPR;
                    f32x4 own = {0.f, 0.f, 0.f, 0.f}, ag = {0.f, 0.f, 0.f, 0.f};
                    if (rr < nr) {
                        own = *reinterpret_cast<const f32x4 *>(St + (r0 + rr) * LDS_ST + 4 * ch);
                        ag = *reinterpret_cast<const f32x4 *>(a.agg + (size_t)(n0 + r0 + rr) * S + 4 * ch);
                    }
                    *reinterpret_cast<f32x4 *>(Xs + rr * LDX + 4 * ch) = own;
                    *reinterpret_cast<f32x4 *>(Xs + rr * LDX + S + 4 * ch) = ag;
                }
                __syncthreads();
            }
            tg_dense_tile<SQ, Form>(L, St, wreg, a, n0, r0 + 16 * wave + c, 16 * wave + c < nr, bn, a.act, wave, c, g, any, Hw, act2);
        }
        k_done = it + 1;
        if (!__syncthreads_or(any)) break;        // (also: the new state is complete before the next gather)
    }
    tg_epilogue<SQ>(a, St, csr.bad, k_done, gi, n0, ng, tid);
}

// ---- output head ----------------------------------------------------------------------------------------------------------------------------
struct GroupHeadSegs { const float *ptr[5]; const int *idx[5]; int ld[5], width[5]; int n; };
struct TrainGroupHead {
    GroupHeadSegs sg;            // input row m = [ptr[s][idx[s][m]][0 : width[s]] for s] (idx over ALL output rows of the call)
    const int *obeg;             // DEVICE [G + 1]: output rows of group g = [obeg[g], obeg[g + 1])
    int in_o, T, act;
    const float *W, *b, *gamma, *beta; float eps;
    float *stats_o;              // [G][2 in_o] (BatchNormalization; untouched for a group without output rows)
    float *out;                  // [M][T]
};
inline size_t train_group_head_lds(int in_o, int T) { return sizeof(float) * ((size_t)64 * (in_o + 1) + 64 * (T + 1) + 3 * (size_t)in_o); }

__global__ void __launch_bounds__(256) k_train_group_head(TrainGroupHead a) {
    extern __shared__ __attribute__((aligned(16))) float th_smem[];
    const int in_o = a.in_o, T = a.T, LDXH = in_o + 1, LDZ = T + 1;
    float *xs = th_smem;                   // [64][in_o + 1] normalised input rows of a chunk
    float *zs = xs + 64 * LDXH;            // [64][T + 1]
    float *mu = zs + 64 * LDZ, *ak = mu + in_o, *ck = ak + in_o;
    const int tid = threadIdx.x, gi = blockIdx.x;
    const int m0 = a.obeg[gi], mg = a.obeg[gi + 1] - m0;
    if (mg < 1) return;                    // no output row: the output network is skipped
    // this thread's input column
    int sgi = -1, j = 0;
    { int c0 = 0; for (int s = 0; s < a.sg.n; ++s) { if (tid >= c0 && tid < c0 + a.sg.width[s]) { sgi = s; j = tid - c0; } c0 += a.sg.width[s]; } }
    if (tid < in_o) {
        float m = 0.0f, aa = 1.0f, cc = 0.0f;
        if (a.gamma && sgi >= 0) {
            const float *xp = a.sg.ptr[sgi]; const int *ix = a.sg.idx[sgi]; const int ld = a.sg.ld[sgi];
            float s1 = 0.0f;
            for (int r = 0; r < mg; ++r) s1 += xp[(size_t)ix[m0 + r] * ld + j];
            m = s1 / (float)mg;
            float s2 = 0.0f;
            for (int r = 0; r < mg; ++r) { const float d = xp[(size_t)ix[m0 + r] * ld + j] - m; s2 = fmaf(d, d, s2); }
            const float var = s2 / (float)mg;
            aa = a.gamma[tid] / sqrtf(var + a.eps); cc = a.beta[tid];
            a.stats_o[(size_t)gi * 2 * in_o + tid] = m; a.stats_o[(size_t)gi * 2 * in_o + in_o + tid] = var;
        }
        mu[tid] = m; ak[tid] = aa; ck[tid] = cc;
    }
    __syncthreads();
    for (int c0 = 0; c0 < mg; c0 += 64) {
        const int nr = min(64, mg - c0);
        for (int s = 0, col0 = 0; s < a.sg.n; col0 += a.sg.width[s], ++s) {
            const int w = a.sg.width[s];
            for (int i = tid; i < nr * w; i += 256) {
                const int r = i / w, jj = i % w, col = col0 + jj;
                const float x = a.sg.ptr[s][(size_t)a.sg.idx[s][m0 + c0 + r] * a.sg.ld[s] + jj];
                xs[r * LDXH + col] = fmaf(x - mu[col], ak[col], ck[col]);
            }
        }
        __syncthreads();
        const int r = tid >> 2, hq = tid & 3;
        if (r < nr) {
            for (int h = hq; h < T; h += 4) {
                float acc = a.b[h];
                for (int k = 0; k < in_o; ++k) acc = fmaf(xs[r * LDXH + k], a.W[(size_t)k * T + h], acc);
                if (a.act == GNN_ACT_SOFTMAX) zs[r * LDZ + h] = acc;
                else a.out[(size_t)(m0 + c0 + r) * T + h] = activate(a.act, acc);
            }
        }
        __syncthreads();
        if (a.act == GNN_ACT_SOFTMAX && tid < nr) {
            float mx = zs[tid * LDZ];
            for (int h = 1; h < T; ++h) mx = fmaxf(mx, zs[tid * LDZ + h]);
            float sum = 0.0f;
            for (int h = 0; h < T; ++h) { const float e = expf(zs[tid * LDZ + h] - mx); zs[tid * LDZ + h] = e; sum += e; }
            for (int h = 0; h < T; ++h) a.out[(size_t)(m0 + c0 + tid) * T + h] = zs[tid * LDZ + h] / sum;
        }
        __syncthreads();
    }
}

// ---- moving statistics, in group order -------------------------------------------------------------------------------------------------------
// moving <- momentum moving + (1 - momentum) batch for g = 0 .. G - 1, slot after slot: `slots` = K, steps of group g = k_groups[g] (state
// network) - or slots = 1 with one step where the group has output rows (output network, obeg given).  A group whose k is negative
// (invalid) moves nothing.  The literal recurrence: the result does not depend on how the graphs were cut into calls.
// `rows_k_steps` (with obeg; heterogeneous state networks, obeg = the type's rows per group): k_groups[g] steps where the group has rows of
// the type, none where it has not.
__global__ void __launch_bounds__(64)
k_bn_moving_groups(const float *__restrict__ stats, int slots, int ncols, const float *__restrict__ k_groups, const int *__restrict__ obeg, int G,
                   float *moving_mean, float *moving_var, float momentum, int rows_k_steps = 0) {
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= ncols) return;
    float mm = moving_mean[col], mv = moving_var[col];
    for (int g = 0; g < G; ++g) {
        const int kg = (int)k_groups[g];
        const int steps = kg < 0 ? 0 : obeg ? (obeg[g + 1] > obeg[g] ? (rows_k_steps ? min(kg, slots) : 1) : 0) : min(kg, slots);
        const float *sl = stats + (size_t)g * slots * 2 * ncols;
        for (int t = 0; t < steps; ++t) {
            mm = mm * momentum + sl[(size_t)t * 2 * ncols + col] * (1.0f - momentum);
            mv = mv * momentum + sl[(size_t)t * 2 * ncols + ncols + col] * (1.0f - momentum);
        }
    }
    moving_mean[col] = mm; moving_var[col] = mv;
}

}  // namespace gnn
