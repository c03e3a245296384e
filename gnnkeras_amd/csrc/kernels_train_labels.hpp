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

// *gate = 1 when every one of the n validity words holds 1, else 0 (a joint step's optimizer update is all or nothing: one word per layer)
constexpr int GATE_MAX_WORDS = 16;
struct GateWords { const int *w[GATE_MAX_WORDS]; int n; };
__global__ void k_gate_all(GateWords g, int *gate) {
    int ok = 1;
    for (int i = 0; i < g.n; ++i) if (*g.w[i] == 0) ok = 0;
    *gate = ok;
}

}  // namespace gnn
