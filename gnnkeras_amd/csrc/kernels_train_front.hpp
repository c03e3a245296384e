// Dropout / AlphaDropout in FRONT of the first Dense of a network (position 0; reference MLP.py:58-71 with dropout_pos = 0:
// BatchNormalization -> Dropout -> Dense 0) on the general training kernels (opt-in: GNN_FLAG_TRAIN_DROPOUT_FRONT).
// The forward launch makes the virtual concatenation real once per network call - normalised on load, dropped out - as X0 [M x in_dim];
// Dense 0 then is a plain layer over X0 (k_segdense / the thin-dense kernel, raw weights, no fold).  The backward launch takes
// dX0 = dZ . W0^T through the masks (regenerated from the call's key) and leaves, with BatchNormalization, one partial per row chunk of
// S1 = sum_r dxn and S2 = sum_r dxn (x - mean) per input column: the first-layer algebra with W = I (kernels_train.hpp
// k_first_layer_param_grads: S1 = q, S2 = diag(P)).  The partials meet in chunk order (k_front_bn_finish): no atomics, a step repeats bitwise.
// Both kernels stream rows: a wave reads 64 consecutive columns of a row (256 contiguous bytes inside a segment), the columns' constants
// stay in registers for all its rows.
#pragma once
#include "kernels_train.hpp"

namespace gnn {

struct FrontSegs { Seg seg[GNN_MAX_SEGS]; int n; };

// the segment `sg` of virtual column kv and the column's offset `off` inside it, resolved in the kernel's own body from its by-value
// argument block `fs` (static indices only: a runtime-indexed - or referenced - kernel-argument array is copied to scratch memory)
#define GNN_FRONT_SEG_OF(fs, kv, sg, off)                                             \
    Seg sg = (fs).seg[0];                                                             \
    int off;                                                                          \
    {                                                                                 \
        int sbeg_ = 0, start_ = (fs).seg[0].width;                                    \
        _Pragma("unroll") for (int s_ = 1; s_ < GNN_MAX_SEGS; ++s_) {                 \
            if (s_ < (fs).n && (kv) >= start_) { sg = (fs).seg[s_]; sbeg_ = start_; } \
            if (s_ < (fs).n) start_ += (fs).seg[s_].width;                            \
        }                                                                             \
        off = (kv) - sbeg_;                                                           \
    }

// X0[m, k] = drop(bn(x[m, k])):  bn(x) = gamma (x - mean) rsqrt(var + eps) + beta (gamma == NULL: x), drop(v) = keep ? v mul + add : fill
// with keep = dropout_keep(key, m, k, thr) - row m of the network call, input column k = seg.wrow + offset: what gnn_dropout draws on
// the materialised [M x K] matrix.  One wave per 4 rows and step (their loads issued together); grid-stride over the rows.
struct FrontFwdArgs {
    const int *gate;
    FrontSegs in; int M, K;
    const float *gamma, *beta, *mean, *var; float eps;
    unsigned key, thr; float mul, add, fill;
    float *X0;                                          // [M x K]
};
constexpr int FRONT_ROWS = 4;

__global__ void __launch_bounds__(256) k_front_input(FrontFwdArgs a) {
    if (gate_closed(a.gate)) return;
    const int lane = threadIdx.x & 63;
    const size_t first = ((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * FRONT_ROWS, step = (size_t)gridDim.x * 4 * FRONT_ROWS;
    for (int c0 = 0; c0 < a.K; c0 += 64) {
        const int kv = c0 + lane;
        if (kv >= a.K) continue;
        GNN_FRONT_SEG_OF(a.in, kv, sg, off)
        const int k = sg.wrow + off;
        float bn_a = 1.0f, bn_c = 0.0f, bn_m = 0.0f;
        if (a.gamma) { bn_a = a.gamma[k] / sqrtf(a.var[k] + a.eps); bn_c = a.beta[k]; bn_m = a.mean[k]; }
        for (size_t m0 = first; m0 < (size_t)a.M; m0 += step) {
            float x[FRONT_ROWS];
#pragma unroll
            for (int u = 0; u < FRONT_ROWS; ++u) {
                const size_t m = m0 + u;
                x[u] = m < (size_t)a.M ? sg.ptr[(sg.rowidx ? (size_t)sg.rowidx[m] : m) * sg.ld + off] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < FRONT_ROWS; ++u) {
                const size_t m = m0 + u;
                if (m >= (size_t)a.M) break;
                const float xn = a.gamma ? fmaf(x[u] - bn_m, bn_a, bn_c) : x[u];      // (the mean leaves first: see SegDenseArgs::in_gamma)
                a.X0[m * a.K + k] = dropout_keep(a.key, (unsigned)m, (unsigned)k, a.thr) ? fmaf(xn, a.mul, a.add) : a.fill;
            }
        }
    }
}

// dxn[m, k] = keep ? dX0[m, k] mul : 0 (the layer's backward; the same key as the forward call), written to the columns of it the caller
// wants: [col_a, col_a + half) -> dx[:, 0 : half), [col_b, col_b + half) -> dx[:, half : 2 half) (col_b < 0: none) - the state / aggregate
// columns of a state network, every column of an output network.  `mean` != NULL (BatchNormalization): the chunk's column sums
// part[chunk][k] = sum_r dxn, part[chunk][K + k] = sum_r dxn (x - mean_k) over the input segments.
// grid = (row chunks, ceil(K / 64)); 64 columns x 4 row groups, 4 rows of a group in flight; the groups meet in LDS in group order.
struct FrontBwdArgs {
    FrontSegs in; int M, K, rows_per_chunk;
    const float *mean;
    unsigned key, thr; float mul;
    const float *dX0;                                   // [M x K]
    float *dx; int ld_dx, half, col_a, col_b;           // dx NULL: no input gradient wanted
    float *part;                                        // [chunk][2 K]
};

__global__ void __launch_bounds__(256) k_front_input_grad(FrontBwdArgs a) {
    __shared__ float red[2][4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int m_beg = blockIdx.x * a.rows_per_chunk, m_end = min(a.M, m_beg + a.rows_per_chunk);
    const int kv = blockIdx.y * 64 + tx;
    float s1 = 0.0f, s2 = 0.0f;
    int k = 0;
    if (kv < a.K) {
        GNN_FRONT_SEG_OF(a.in, kv, sg, off)
        k = sg.wrow + off;
        const float mu = a.mean ? a.mean[k] : 0.0f;
        int oc = -1;                                    // the column of dx this input column goes to
        if (a.dx && k >= a.col_a && k < a.col_a + a.half) oc = k - a.col_a;
        else if (a.dx && a.col_b >= 0 && k >= a.col_b && k < a.col_b + a.half) oc = a.half + k - a.col_b;
        for (int m0 = m_beg + ty; m0 < m_end; m0 += 4 * FRONT_ROWS) {
            float g[FRONT_ROWS], x[FRONT_ROWS];
#pragma unroll
            for (int u = 0; u < FRONT_ROWS; ++u) {
                const int m = m0 + 4 * u;
                g[u] = m < m_end ? a.dX0[(size_t)m * a.K + k] : 0.0f;
                x[u] = (a.mean && m < m_end) ? sg.ptr[(sg.rowidx ? (size_t)sg.rowidx[m] : (size_t)m) * sg.ld + off] : mu;
            }
#pragma unroll
            for (int u = 0; u < FRONT_ROWS; ++u) {
                const int m = m0 + 4 * u;
                if (m >= m_end) break;
                const float d = dropout_keep(a.key, (unsigned)m, (unsigned)k, a.thr) ? g[u] * a.mul : 0.0f;
                if (oc >= 0) a.dx[(size_t)m * a.ld_dx + oc] = d;
                s1 += d;
                s2 = fmaf(d, x[u] - mu, s2);
            }
        }
    }
    if (!a.mean) return;
    red[0][ty][tx] = s1; red[1][ty][tx] = s2;
    __syncthreads();
    if (ty == 0 && kv < a.K) {
        float *p = a.part + (size_t)blockIdx.x * 2 * a.K;
        p[k] = ((red[0][0][tx] + red[0][1][tx]) + red[0][2][tx]) + red[0][3][tx];
        p[a.K + k] = ((red[1][0][tx] + red[1][1][tx]) + red[1][2][tx]) + red[1][3][tx];
    }
}

// The chunk partials of k_front_input_grad summed like k_reduce_partials sums (contiguous quarters of the chunks, each in chunk order, the
// quarters in order: a fixed tree), then what k_first_layer_param_grads does with W = I and centred rows:
//   dbeta_k (+)= S1_k    dgamma_k (+)= rstd_k S2_k    m1_k = S1_k / M    m2_k = rstd_k S2_k / M    (m1 / m2: k_bn_input_grad_segs)
// grid = ceil(K / 64).
__global__ void __launch_bounds__(256)
k_front_bn_finish(const float *__restrict__ part, int n_chunks, int K, const float *__restrict__ var, float eps, float inv_m,
                  float *dgamma, float *dbeta, float *__restrict__ m1, float *__restrict__ m2, int accumulate) {
    __shared__ float red[2][4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int k = blockIdx.x * 64 + tx;
    const int per = (n_chunks + 3) / 4, c_beg = ty * per, c_end = min(n_chunks, c_beg + per);
    float s1 = 0.0f, s2 = 0.0f;
    if (k < K)
        for (int c = c_beg; c < c_end; ++c) { s1 += part[(size_t)c * 2 * K + k]; s2 += part[(size_t)c * 2 * K + K + k]; }
    red[0][ty][tx] = s1; red[1][ty][tx] = s2;
    __syncthreads();
    if (ty != 0 || k >= K) return;
    const float S1 = ((red[0][0][tx] + red[0][1][tx]) + red[0][2][tx]) + red[0][3][tx];
    const float S2 = ((red[1][0][tx] + red[1][1][tx]) + red[1][2][tx]) + red[1][3][tx];
    const float dg = (1.0f / sqrtf(var[k] + eps)) * S2;
    dgamma[k] = accumulate ? dgamma[k] + dg : dg;
    dbeta[k] = accumulate ? dbeta[k] + S1 : S1;
    m1[k] = S1 * inv_m; m2[k] = dg * inv_m;
}

#undef GNN_FRONT_SEG_OF

}  // namespace gnn
