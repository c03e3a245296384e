// The one-CU-per-group whole-loop kernel (kernel_state_lds.hpp) for HETEROGENEOUS models: one state network per node type
// (gnn_loop_args_t::composite with group_node_begin).  k_state_lds feeds the matrix core with the folded first-layer weights as the A
// operand and 16 node rows as the B operand of v_mfma_f32_16x16x4_f32, so the 16 rows of a tile share ONE weight matrix: with a network
// per type a tile must hold rows of one type only.
//
//   * the group's state sits in LDS in POSITION order: the rows of type 0 first, then type 1, .. - each (group, type) range padded to a
//     multiple of 16 rows.  A group is a contiguous node range and type t's row list (type_nodes) is ascending, so the rows of type t in
//     group g are the slice type_nodes[tbeg[t][g] .. tbeg[t][g + 1]) (k_group_type_begin, shared with the training-mode group kernels).
//     positions <= n_g + 15 n_types: what the host's "fits" test and the staging rows are sized by;
//   * Orig[position] = local node id (-1: pad row), Inv[local node] = position, both in LDS: the neighbour ids of the per-node record are
//     translated to positions when the records are built, the ids of rows with more than 4 arcs (read from the CSR) as they are read;
//   * pad rows are zero, are never a neighbour, never enter the predicate and are not written back;
//   * a wave owns a CONTIGUOUS run of tiles and holds the weights of its current tile's type in registers: they are reloaded (from L2,
//     32 dwords per lane at width 32) only when the walk crosses into another type - at most n_types - 1 + 16 reloads per iteration over
//     the whole workgroup, none at all in a group of one type.  (All types' blocks in LDS instead would take 8 KB per type at width 32 and
//     one LDS read per weight register and TILE: 32 ds_read_b32 against the tile's 32 MFMAs.)  The hidden-layer form (GNN_FLAG_LDS_HIDDEN:
//     every type Dense(H_t) - Dense(S)) does keep every type's SECOND layer in LDS - 4 KB per type at width 32, read as four ds_read_b128
//     per tile - because W1 leaves no registers for it; W1 stays in registers as here;
//   * the per-node constant C (setup_constants writes it per type, indexed by node), state_0 and the per-arc weights are read by original
//     node id; the result goes back to state_out in node order;
//   * what is this kernel's own: the prologue (rows per type, positions, Orig / Inv, records by position), the row policy LdsRowsTyped, the
//     walk over a contiguous run of tiles with the weight reload, and the result copy in node order.  The update of a tile, the end of an
//     iteration (flag words, copy back), group sets, no_exit, k and the launcher are kernel_state_lds.hpp's pieces, instantiated with that
//     policy - the double-buffered form included.  state_0's predicate comes from k_pred0_groups, one word per GROUP (the arithmetic of
//     k_converge, row by row).
#pragma once
#include "kernel_state_lds.hpp"

namespace gnn {

struct TypeOffsets { int off[GNN_MAX_TYPES + 1]; };

// tbeg[t][g] = first position in type_nodes, at or behind type t's begin, whose node id is >= gbeg[g]
__global__ void __launch_bounds__(256)
k_group_type_begin(const int *__restrict__ type_nodes, TypeOffsets to, int n_types, const int *__restrict__ gbeg, int G, int *__restrict__ tbeg) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_types * (G + 1)) return;
    const int t = i / (G + 1), g = i % (G + 1);
    const int key = gbeg[g];
    int lo = to.off[t], hi = to.off[t + 1];
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (type_nodes[mid] < key) lo = mid + 1; else hi = mid; }
    tbeg[i] = lo;
}

// pred0[g] = does any node of group g still move between state_old = ones and state_0?  (16 lanes per node, as k_converge)
__global__ void __launch_bounds__(256)
k_pred0_groups(const int *__restrict__ node_begin, const float *__restrict__ s, int ld_s, int S, float thr, int *__restrict__ pred0) {
    const int g = blockIdx.x, nb = node_begin[g], ne = node_begin[g + 1];
    const int lane = threadIdx.x & 15;
    int any = 0;
    for (int j0 = nb; j0 < ne; j0 += 16) {
        const int j = j0 + threadIdx.x / 16;
        float d2 = 0.0f, n2 = 0.0f;
        if (j < ne) {
            for (int f = lane; f < S; f += 16) {
                const float d = s[(size_t)j * ld_s + f] - 1.0f;
                d2 = fmaf(d, d, d2);
                n2 = fmaf(1.0f, 1.0f, n2);
            }
        }
#pragma unroll
        for (int off = 8; off >= 1; off >>= 1) {
            d2 += __shfl_xor(d2, off, 16);
            n2 += __shfl_xor(n2, off, 16);
        }
        if (j < ne && sqrtf(d2) > thr * sqrtf(n2)) any = 1;
    }
    any = __syncthreads_or(any);
    if (threadIdx.x == 0) pred0[g] = any;
}

// The row policy of the typed kernel (kernel_state_lds.hpp): LDS rows are POSITIONS; Orig / Inv translate.  Pad rows exist and stay zero,
// and an arc's source may be no row of the group (a node that no type lists, a source outside the group's range).
struct LdsRowsTyped {
    static constexpr bool PAD_ROWS = true, ALL_ARCS_ARE_ROWS = false;
    const int *Orig, *Inv; int n;
    __device__ __forceinline__ int node(int row) const { return Orig[row]; }
    __device__ __forceinline__ bool on(int, int j) const { return j >= 0; }
    __device__ __forceinline__ bool has_row(int l) const { return (unsigned)l < (unsigned)n; }
    __device__ __forceinline__ int row_of(int l) const { return Inv[l]; }
};

struct LdsTypeNet { const float *Wf; int wrow_state, wrow_agg, act; };

struct LdsTypesArgs {
    LdsArgs l;                      // as for k_state_lds; unused: tile64_begin, Wf, wrow_*, H, act.  pred0: one word per GROUP
    LdsTypeNet tp[GNN_MAX_TYPES];
    int n_types;
    const int *type_nodes;          // device [N]: node ids grouped by type, ascending inside a type
    const int *tbeg;                // device [n_types][n_groups + 1] (k_group_type_begin)
    int n_groups;
};

// LDS of a group of n nodes in at most `rows` positions: state rows (twice: DB), records, Orig per position; Inv per node
inline int lds_types_rows(int n_nodes, int n_types) { return n_nodes + 15 * n_types; }
// (`hidden`: the hidden-layer form - a W2 / b2 block per type out of the same budget)
inline size_t lds_types_bytes(int n_nodes, int n_types, int SP, bool db = false, bool hidden = false) {
    return (size_t)lds_types_rows(n_nodes, n_types) * ((db ? 2 : 1) * SP * sizeof(float) + sizeof(LdsRec) + sizeof(int)) + (size_t)n_nodes * sizeof(int) +
           lds_hidden_bytes(SP, hidden ? n_types : 0);
}
inline bool lds_types_group_fits(int n_nodes, int n_types, int SP, bool hidden = false) {
    return lds_types_bytes(n_nodes, n_types, SP, false, hidden) <= LDS_BUDGET_BYTES && lds_types_rows(n_nodes, n_types) < 65536;
}
inline bool lds_types_group_fits_twice(int n_nodes, int n_types, int SP, bool hidden = false) {
    return lds_types_bytes(n_nodes, n_types, SP, true, hidden) <= LDS_BUDGET_BYTES;
}
// the largest group (in nodes) that fits
inline int lds_types_max_nodes(int n_types, int SP, bool hidden = false) {
    const size_t per_row = SP * sizeof(float) + sizeof(LdsRec) + sizeof(int);
    const size_t fixed = (size_t)15 * n_types * per_row + lds_hidden_bytes(SP, hidden ? n_types : 0);
    if (fixed >= LDS_BUDGET_BYTES) return 0;
    return (int)((LDS_BUDGET_BYTES - fixed) / (per_row + sizeof(int)));
}

// Written once over the hidden-layer operands `Hid` (kernel_state_lds.hpp).  LdsHidden: every type's state network has a hidden layer -
// LdsTypeNet::act is the hidden activation, LdsArgs::H the widest first layer, hid[t] the second Dense of type t (a struct of its own around
// the one-layer kernel's arguments, which stay what they were); every type's W2 / b2 block sits in LDS, and which one a wave reads changes
// together with the first layer's registers.
struct LdsTypesHidArgs { LdsTypesArgs t; LdsHidNet hid[GNN_MAX_TYPES]; };
__device__ __forceinline__ const LdsTypesArgs &lds_types_args(const LdsTypesArgs &a) { return a; }
__device__ __forceinline__ const LdsTypesArgs &lds_types_args(const LdsTypesHidArgs &a) { return a.t; }
__device__ __forceinline__ const LdsHidNet *lds_hid_nets(const LdsTypesArgs &) { return nullptr; }
__device__ __forceinline__ const LdsHidNet *lds_hid_nets(const LdsTypesHidArgs &a) { return a.hid; }

template <int SP, bool HAS_W, bool DB, class Hid = LdsNoHidden>
__global__ void __launch_bounds__(64 * LDS_NW, 4) k_state_lds_types(std::conditional_t<Hid::ON, LdsTypesHidArgs, LdsTypesArgs> args) {
    const LdsTypesArgs &ta = lds_types_args(args);
    const LdsHidNet *hn = lds_hid_nets(args);
    constexpr int NCT = SP / 16;
    constexpr int KS = 2 * SP / 4;
    extern __shared__ __attribute__((aligned(16))) char smem_lds[];
    __shared__ int moving_s[3];
    __shared__ int set_go;
    __shared__ int pb_s[GNN_MAX_TYPES + 1];       // first position of every type (multiples of 16); [n_types] = positions of the group
    __shared__ int cnt_s[GNN_MAX_TYPES];          // rows of every type in this group
    __shared__ int tb_s[GNN_MAX_TYPES];           // ... and where they begin in type_nodes
    __shared__ LdsTypeNet net_s[GNN_MAX_TYPES];
    LdsHidNet *hid_s = nullptr;                   // the second Dense per type: LDS of the hidden form alone
    if constexpr (Hid::ON) { __shared__ LdsHidNet hid_nets[GNN_MAX_TYPES]; hid_s = hid_nets; }

    const LdsArgs &a = ta.l;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int grp = blockIdx.x;
    const int nb = a.node_begin[grp], ne = a.node_begin[grp + 1], n = ne - nb;
    const int S = a.S, T = ta.n_types;

    // ---- the group's rows per type, their positions --------------------------------------------------------------------------------------
#pragma unroll
    for (int t = 0; t < GNN_MAX_TYPES; ++t)
        if (tid == t && t < T) {
            const int b0 = ta.tbeg[t * (ta.n_groups + 1) + grp], b1 = ta.tbeg[t * (ta.n_groups + 1) + grp + 1];
            tb_s[t] = b0; cnt_s[t] = b1 - b0;
            net_s[t] = ta.tp[t];
            if constexpr (Hid::ON) hid_s[t] = hn[t];
        }
    if (tid == 0) { moving_s[0] = 0; moving_s[1] = 0; moving_s[2] = 0; }
    __syncthreads();
    if (tid == 0) {
        int p0 = 0;
        for (int t = 0; t < T; ++t) { pb_s[t] = p0; p0 += (cnt_s[t] + 15) & ~15; }
        pb_s[T] = p0;
    }
    __syncthreads();
    const int P = pb_s[T];                        // positions of this group (<= n + 15 T), a multiple of 16
    if (P > n + 15 * T) {                         // type lists that name a node twice: more rows than LDS and staging are sized for
        if (tid == 0) a.k_out[grp] = -1.0e9f;
        return;
    }
    const int n_tiles = P >> 4;
    float *const hid_blk = reinterpret_cast<float *>(smem_lds);                      // hidden form: [T] blocks of W2 / b2 (lds_fill_hidden)
    float *St = hid_blk + (Hid::ON ? (size_t)T * lds_hidden_block_floats(SP) : 0);   // [P][SP] (DB: two of them)
    LdsRec *Rec = reinterpret_cast<LdsRec *>(St + (size_t)(DB ? 2 : 1) * P * SP);    // [P]
    int *Orig = reinterpret_cast<int *>(Rec + P);                                    // [P]: local node of a position, -1 = pad row
    int *Inv = Orig + P;                                                             // [n]: position of a local node
    float *const St_base = St;

    for (int i = tid; i < n; i += 64 * LDS_NW) Inv[i] = 0;      // (a node that no type lists: never a row; as a neighbour it reads position 0)
    if constexpr (Hid::ON)
        for (int t = 0; t < T; ++t) lds_fill_hidden<SP>(hid_blk + (size_t)t * lds_hidden_block_floats(SP), hid_s[t], S, tid);
    __syncthreads();
    for (int t = 0; t < T; ++t) {
        const int p0 = pb_s[t], c = cnt_s[t], b0 = tb_s[t], cp = (c + 15) & ~15;
        for (int i = tid; i < cp; i += 64 * LDS_NW) {
            int j = -1;
            if (i < c) {
                const unsigned l = (unsigned)(ta.type_nodes[b0 + i] - nb);
                if (l < (unsigned)n) { j = (int)l; Inv[j] = p0 + i; }
            }
            Orig[p0 + i] = j;
        }
    }
    __syncthreads();
    // ---- state_0 and the CSR records into LDS, by position ----------------------------------------------------------------------------------
    for (int i = tid; i < P * SP; i += 64 * LDS_NW) {
        const int ps = i / SP, c = i % SP, j = Orig[ps];
        St[i] = (j >= 0 && c < S) ? a.state0[(size_t)(nb + j) * a.ld_s0 + c] : 0.0f;
        if (DB) St[(size_t)P * SP + i] = 0.0f;
    }
    for (int ps = tid; ps < P; ps += 64 * LDS_NW) {
        const int j = Orig[ps];
        LdsRec rec = LdsRec{0u, 0u, 0, 1.0f};
        if (j >= 0) {
            const int beg = a.rowptr[nb + j], end = a.rowptr[nb + j + 1];
            unsigned id[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const unsigned l = beg + u < end ? (unsigned)(a.src[beg + u] - nb) : 0u;
                id[u] = beg + u >= end ? 0u : (l < (unsigned)n ? (unsigned)Inv[l] : LDS_NO_ROW);      // (positions stay below 65535)
            }
            rec = LdsRec{id[0] | (id[1] << 16), id[2] | (id[3] << 16), end - beg, a.row_scale ? a.row_scale[nb + j] : 1.0f};
        }
        Rec[ps] = rec;
    }
    const LdsRowsTyped rows{Orig, Inv, n};
    const int set_lo = a.set_bar ? a.set_first[grp] : grp, set_n = a.set_bar ? a.set_size[grp] : 1;
    unsigned moved_seen[2] = {0u, 0u};
    int timed_out = 0;
    const int run = lds_run0(a, set_lo, set_lo + set_n, lane);             // state_0's predicate: one word per group of the set
    __syncthreads();

    // rows of the staging buffer: group g's begin behind the padded sizes of the groups before it (bounded by 15 n_types each)
    const __amdgpu_buffer_rsrc_t r_C = buf_rsrc(a.C + (size_t)nb * a.ldC), r_stage = buf_rsrc(a.stage + ((size_t)nb + (size_t)15 * T * grp) * SP);
    auto load_c = [&](int t, f32x4 (&c)[NCT]) {     // C of tile t by original node
        const int j = Orig[16 * t + r];
        // (hidden form: the widest first layer of any type, LdsArgs::H - the tile masks the columns at or past its own type's H)
        lds_load_c<SP>(c, r_C, j >= 0, j, Hid::ON ? a.H : S, a.ldC, g);
    };

    // a wave's tiles: a contiguous run, so that it crosses from one type into the next as rarely as possible
    const int per = (n_tiles + LDS_NW - 1) / LDS_NW;
    const int t_lo = min(wave * per, n_tiles), t_hi = min(t_lo + per, n_tiles);
    float wreg[KS][NCT];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) wreg[ks][ct] = 0.0f;
    int cur_ty = -1, act = 0;
    Hid hid = {};                                 // (hidden form: set with the first tile's type, like wreg)

    int k_done = 0;
    for (int it = 0; run && it < a.max_iteration; ++it) {
        float *Snew = St_base;
        if (DB) { St = St_base + (size_t)(it & 1) * P * SP; Snew = St_base + (size_t)((it + 1) & 1) * P * SP; }
        f32x4 cn[NCT];
        int any = 0;
        if (t_lo < t_hi) load_c(t_lo, cn);
#pragma unroll 1
        for (int t = t_lo; t < t_hi; ++t) {
            f32x4 c[NCT];
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) c[ct] = cn[ct];
            if (t + 1 < t_hi) load_c(t + 1, cn);
            // the tile's type (wave-uniform): the weights change hands only when it differs from the previous tile's
            int ty = 0;
            for (int u = 1; u < T; ++u) ty += (16 * t >= pb_s[u]) ? 1 : 0;
            ty = __builtin_amdgcn_readfirstlane(ty);
            if (ty != cur_ty) {
                cur_ty = ty;
                const LdsTypeNet nt = net_s[ty];
                const float *Wf = static_cast<const float *>(uniform_ptr(nt.Wf));
                const int ws = __builtin_amdgcn_readfirstlane(nt.wrow_state), wa = __builtin_amdgcn_readfirstlane(nt.wrow_agg);
                act = __builtin_amdgcn_readfirstlane(nt.act);
                if constexpr (Hid::ON) {                                     // W2 / b2 change hands with W1: the type's block in LDS
                    const int H = __builtin_amdgcn_readfirstlane(hid_s[ty].H);
                    lds_fill_wreg<SP>(wreg, Wf, ws, wa, S, H, r, g);         // (the folded block is [.. x H])
                    hid = LdsHidden{hid_blk + (size_t)ty * lds_hidden_block_floats(SP), H, __builtin_amdgcn_readfirstlane(hid_s[ty].act2)};
                } else {
                    lds_fill_wreg<SP>(wreg, Wf, ws, wa, S, S, r, g);         // (the host checked units[0] == S)
                }
            }
            lds_tile<SP, HAS_W, DB>(a, rows, nb, t, r, g, St, Snew, Rec, r_stage, wreg, c, act, any, hid);
        }
        const int mv_slot = lds_iter_end<SP, DB>(moving_s, any, it, St, r_stage, P, tid);
        if (DB) St = Snew;
        k_done = it + 1;
        if (lds_leaves(a, moving_s, &set_go, mv_slot, it, set_lo, set_n, moved_seen, timed_out, tid)) break;
    }
    // ---- result rows to the caller's compact buffer in node order, k of this group ------------------------------------------------------
    for (int i = tid; i < P * S; i += 64 * LDS_NW) {
        const int ps = i / S, c = i % S, j = Orig[ps];
        if (j >= 0) a.state_out[(size_t)(nb + j) * S + c] = St[ps * SP + c];
    }
    if (tid == 0) a.k_out[grp] = timed_out ? -1.0e9f : (float)k_done;
}

struct LdsTypesKernel {         // (launch_lds_one, kernel_state_lds.hpp)
    using Args = LdsTypesArgs;
    static LdsArgs &common(Args &a) { return a.l; }
    static constexpr const char *name = "k_state_lds_types", *tail = "";
    template <int SP, bool HAS_W, bool DB> static constexpr void (*fn)(Args) = k_state_lds_types<SP, HAS_W, DB>;
};
struct LdsTypesHidKernel {
    using Args = LdsTypesHidArgs;
    static LdsArgs &common(Args &a) { return a.t.l; }
    static constexpr const char *name = "k_state_lds_types", *tail = ",hidden";
    template <int SP, bool HAS_W, bool DB> static constexpr void (*fn)(Args) = k_state_lds_types<SP, HAS_W, DB, LdsHidden>;
};

// max_nodes: nodes of the largest group (every workgroup requests LDS for its bound of positions)
inline int launch_lds_types(const LdsTypesArgs &la, int SP, int max_nodes, hipStream_t st) {
    const bool db = lds_types_group_fits_twice(max_nodes, la.n_types, SP);
    return launch_lds_family<LdsTypesKernel>(la, SP, db, la.n_groups, lds_types_bytes(max_nodes, la.n_types, SP, db), st);
}
inline int launch_lds_types_hidden(const LdsTypesHidArgs &ha, int SP, int max_nodes, hipStream_t st) {
    const bool db = lds_types_group_fits_twice(max_nodes, ha.t.n_types, SP, true);
    return launch_lds_family<LdsTypesHidKernel>(ha, SP, db, ha.t.n_groups, lds_types_bytes(max_nodes, ha.t.n_types, SP, db, true), st);
}

}  // namespace gnn
