// Label gradients of an in-library training step (gnn_train_step_ex: d_nodes / d_arc_labels; docs/joint_lgnn_step.md).
//
// The constant input columns of the state network - the node labels, the aggregated labels, the aggregated arc labels - are the same in
// every iteration, and so are their BatchNormalization statistics.  Their gradient is therefore linear in the first layer's dZ: with
// DZ = sum_t dZ_t (the persistent small-graph kernel keeps it in registers; the general path accumulates it per iteration) and
// g_c[n] = sum_j W[c][j] DZ[n][j],
//     without BatchNormalization   d x_c[n] = g_c[n]
//     with BatchNormalization      d x_c[n] = gamma_c rstd_c (g_c[n] - mean(g_c) - xhat_c[n] mean(g_c xhat_c))
// and the two column means need no reduction of their own: sum_n g_c[n] = sum_j W[c][j] q_j is the step's d beta_c and
// sum_n g_c[n] xhat_c[n] = sum_j W[c][j] Phat[c][j] its d gamma_c (both summed over the iterations, as DZ is), which the step has
// just reduced.  One pass over the rows replaces the k products per segment of the building blocks.
#pragma once
#include "kernels_train_small.hpp"

namespace gnn {

constexpr int LG_ROWS = 16;                 // rows of DZ a workgroup stages at once
constexpr int LG_MAX_H = 960;               // ... of at most this many columns (rows of H + 1 floats: 60 KiB of LDS)

struct LabelGradArgs {
    int N, H, ldz;                          // DZ [N][ldz], H valid columns
    const float *DZ;
    const float *W;                         // [in_dim][H] the first layer's kernel
    ConstSegs cs;                           // the constant segments: values (BatchNormalization: for xhat), widths, first weight row
    float *out[3]; int ldo[3];              // where segment s's gradient goes ([N][width[s]], row stride ldo[s]); NULL: not wanted
    const float *gamma, *mean, *var;        // NULL gamma: no BatchNormalization; mean / var by weight row
    const float *dgamma, *dbeta;            // the step's reduced [in_dim] gradients (unscaled): N mean(g xhat), N mean(g)
    float eps, inv_n;
};

__global__ void __launch_bounds__(256) k_label_grads(LabelGradArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lg_dz[];      // [LG_ROWS][H + 1] (odd stride: the rows of a column group sit in different banks)
    const int tid = threadIdx.x, ldl = a.H + 1;
    const int Kc = (a.cs.n > 0 ? a.cs.width[0] : 0) + (a.cs.n > 1 ? a.cs.width[1] : 0) + (a.cs.n > 2 ? a.cs.width[2] : 0);
    for (int r0 = blockIdx.x * LG_ROWS; r0 < a.N; r0 += gridDim.x * LG_ROWS) {
        const int nr = min(LG_ROWS, a.N - r0);
        __syncthreads();                    // (the previous tile's readers are done)
        for (int i = tid; i < nr * a.H; i += 256) lg_dz[(i / a.H) * ldl + i % a.H] = a.DZ[(size_t)(r0 + i / a.H) * a.ldz + i % a.H];
        __syncthreads();
        for (int i = tid; i < nr * Kc; i += 256) {
            const int jc = i / nr, rr = i % nr;       // the nr lanes of one constant column read the SAME row of W (one request), each its own row of DZ
            int sg = 0, j = jc;
            while (sg + 1 < a.cs.n && j >= a.cs.width[sg]) { j -= a.cs.width[sg]; ++sg; }
            float *dst = a.out[sg];
            if (!dst) continue;
            const int k = a.cs.wrow[sg] + j;
            const float *w = a.W + (size_t)k * a.H, *z = lg_dz + rr * ldl;
            float g = 0.0f;
            for (int h = 0; h < a.H; ++h) g = fmaf(w[h], z[h], g);
            const size_t n = (size_t)(r0 + rr);
            if (a.gamma) {
                const float rstd = 1.0f / sqrtf(a.var[k] + a.eps);
                const float xhat = (a.cs.ptr[sg][n * a.cs.ld[sg] + j] - a.mean[k]) * rstd;
                g = a.gamma[k] * rstd * (g - a.dbeta[k] * a.inv_n - xhat * (a.dgamma[k] * a.inv_n));
            }
            dst[n * a.ldo[sg] + j] = g;
        }
    }
}

// ---- heterogeneous models (gnn_train_step_composite_ex): ONE launch for the networks of all node types ----------------------------------------
// A composite layer has one state network per node type; DZ is in POSITION order (position i = node type_nodes[i], every type a contiguous
// range of positions), the outputs in the caller's node order.  Type t's constant inputs are [nodes[:, :d_t] | aggregated_component[:, :W_comp]]
// (weight rows 0 .. and wrow_comp ..).  A workgroup takes 16 positions of ONE type; the tile's type is found by a linear search over the
// <= GNN_MAX_TYPES prefix sums of the per-type tile counts.  Every node has exactly one type: every row of both outputs is written once,
// the own-label columns [d_t, L) of a row with zeros - no memset in front of the launch.
struct LabelGradType {
    int pos0, count;                        // first position, rows
    int ldz, H;                             // DZ [count][ldz], H valid columns
    int d_t, wrow_comp;                     // own label columns (weight rows 0 ..), first weight row of the aggregated component
    const float *DZ;                        // the type's first row
    const float *W;                         // [in_dim_t][H] the first layer's kernel
    const float *gamma, *mean, *var;        // NULL gamma: no BatchNormalization; mean / var by weight row (the constant columns' statistics)
    const float *dgamma, *dbeta;            // the step's finished [in_dim_t] gradients (unscaled)
    float eps, inv_n;                       // inv_n = 1 / count
};
struct LabelGradTypesArgs {
    int n_types, L, W_comp;
    int tile_begin[GNN_MAX_TYPES + 1];      // prefix sums of ceil(count_t / LG_ROWS)
    const int *type_nodes;                  // [N] position -> node
    const float *nodes; int ld_nodes;       // the labels (xhat of the own columns: the value at the NODE's row)
    const float *agg_comp;                  // [N][W_comp] by node
    float *lab_own; int ld_own;             // OUT [N][L] by node (row stride ld_own): columns [0, d_t) of the node's type, zeros behind them
    float *g_comp;                          // OUT [N][W_comp] by node
    LabelGradType t[GNN_MAX_TYPES];
};

__global__ void __launch_bounds__(256) k_label_grads_types(LabelGradTypesArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lgt_dz[];     // [LG_ROWS][H + 1] (odd stride, as in k_label_grads)
    const int tid = threadIdx.x, n_tiles = a.tile_begin[a.n_types], C = a.L + a.W_comp;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        int ty = 0;
        while (ty + 1 < a.n_types && tile >= a.tile_begin[ty + 1]) ++ty;
        const LabelGradType &y = a.t[ty];
        const int r0 = (tile - a.tile_begin[ty]) * LG_ROWS, nr = min(LG_ROWS, y.count - r0);
        const int H = y.H, ldz = y.ldz, ldl = H + 1;
        const float *dz = y.DZ + (size_t)r0 * ldz;
        __syncthreads();                    // (the previous tile's readers are done)
        // whole 16-byte pieces of a row where its stride and the base allow them, the H % 4 last columns (widths such as 7 or 9) one by one
        const int hq = ((ldz & 3) == 0 && (reinterpret_cast<uintptr_t>(y.DZ) & 15) == 0) ? H >> 2 : 0;
        for (int i = tid; i < nr * hq; i += 256) {
            const int rr = i / hq, c4 = 4 * (i % hq);
            const float4 v = *reinterpret_cast<const float4 *>(dz + (size_t)rr * ldz + c4);
            float *d = lgt_dz + rr * ldl + c4;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
        const int tail0 = 4 * hq, nt = H - tail0;
        for (int i = tid; i < nr * nt; i += 256) lgt_dz[(i / nt) * ldl + tail0 + i % nt] = dz[(size_t)(i / nt) * ldz + tail0 + i % nt];
        __syncthreads();
        for (int i = tid; i < nr * C; i += 256) {
            const int jc = i / nr, rr = i % nr;       // the nr lanes of one column read the SAME row of W, each its own row of DZ
            const size_t node = (size_t)a.type_nodes[y.pos0 + r0 + rr];
            const bool own = jc < a.L;
            const int j = own ? jc : jc - a.L;
            float *dst = own ? a.lab_own + node * a.ld_own + j : a.g_comp + node * a.W_comp + j;
            if (own && j >= y.d_t) { *dst = 0.0f; continue; }
            const int k = own ? j : y.wrow_comp + j;
            const float *w = y.W + (size_t)k * H, *z = lgt_dz + rr * ldl;
            float g = 0.0f;
            for (int h = 0; h < H; ++h) g = fmaf(w[h], z[h], g);
            if (y.gamma) {
                const float rstd = 1.0f / sqrtf(y.var[k] + y.eps);
                const float x = own ? a.nodes[node * a.ld_nodes + j] : a.agg_comp[node * a.W_comp + j];
                const float xhat = (x - y.mean[k]) * rstd;
                g = y.gamma[k] * rstd * (g - y.dbeta[k] * y.inv_n - xhat * (y.dgamma[k] * y.inv_n));
            }
            *dst = g;
        }
    }
}

// *gate = 1 when every one of the n validity words holds 1, else 0 (a joint step's optimizer update is all or nothing: one word per layer)
constexpr int GATE_MAX_WORDS = 16;
struct GateWords { const int *w[GATE_MAX_WORDS]; int n; };
__global__ void k_gate_all(GateWords g, int *gate) {
    int ok = 1;
    for (int i = 0; i < g.n; ++i) if (*g.w[i] == 0) ok = 0;
    *gate = ok;
}

}  // namespace gnn
