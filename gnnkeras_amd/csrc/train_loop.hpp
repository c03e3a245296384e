// gnn_train_step: one whole training step of a homogeneous model inside the library (reference GNN/Models/GNN.py:277-306:
// `self(x, training=True)`, `compiled_loss`, `tape.gradient` through the unrolled loop, `dwbS / k`).  Included at the end of
// gnnloop.hip, after train_api.hpp (shares the launchers).  Declared in include/gnnloop.h.
//
// Same algebra as gnnkeras_amd/Models/training.py (which stays the general path: composite models, LGNN label gradients):
// the tape is the k + 1 state matrices plus per-iteration BatchNormalization statistics and folded first-layer weights;
// aggregates and hidden activations are recomputed in the backward sweep; the first layer never materialises the
// N x in_dim concatenation (P = X^T dZ per segment, dW = a (.) P + c q^T, BN input-gradient moments from W, P, q).
// What moves into the library is the ORCHESTRATION: ~14 launches per iteration pair instead of ~36, no Python between them.
#pragma once
#include "kernels_train.hpp"
#include "kernels_train_big.hpp"
#include "kernels_train_small.hpp"
#include "kernels_train_labels.hpp"
#include "kernels_train_front.hpp"

namespace {

struct NetCtx {
    const gnn_mlp_t *m;
    const gnn_mlp_grads_t *g;
    float *Wt[GNN_MAX_LAYERS];      // kernel transposes [units[l]][fan_in]
    float *P, *q, *m1, *m2;         // first-layer scratch: [in_dim x H1], [H1], [in_dim], [in_dim]
    float *G[2];                    // gradient ping-pong [rows x max units]
    float *hid[GNN_MAX_LAYERS];     // layer outputs [rows x units[l]] (the last one may alias a caller buffer)
    float *dropbuf[GNN_MAX_LAYERS + 1];   // [q]: what the Dense at position q consumes when Dropout layers sit there ([rows x units[q - 1]]); else NULL
};

// ---- Dropout / AlphaDropout layers of a network call (ABI 8: gnn_dropout_spec_t; reference MLP.py:60-66) -------------------------------------
// The masks are the counter hash of gnn_dropout keyed by (step seed, network, call, layer): nothing is stored, the backward pass of a call
// regenerates them.  Positions 1 .. n_layers (behind a Dense layer's activation); position 0 (in front of the first Dense) is refused by the
// plans - but for ONE layer per network of a homogeneous model under GNN_FLAG_TRAIN_DROPOUT_FRONT (kernels_train_front.hpp; `front_ok` below).
inline unsigned lowbias32_host(unsigned h) { h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16; return h; }
inline unsigned drop_key(unsigned seed, unsigned net_id, unsigned call, unsigned index) {
    unsigned h = 0x9E3779B9u;
    const unsigned v[4] = {seed, net_id, call, index};
    for (int i = 0; i < 4; ++i) h = lowbias32_host(h ^ v[i]);
    return h;
}
struct DropRun {
    const gnn_dropout_spec_t *d;           // NULL or n == 0: no Dropout layers
    unsigned seed; int call;
    float *buf[GNN_MAX_LAYERS + 1];        // [q]: destination of the dropped-out copy for position q (forward)
};
inline bool drop_at_position(const gnn_dropout_spec_t &d, int q) {
    for (int i = 0; i < d.n; ++i) if (d.pos[i] == q) return true;
    return false;
}
inline bool drop_at(const DropRun *r, int q) { return r && r->d && drop_at_position(*r->d, q); }
// every Dropout layer at position q: forward x -> y (list order; later layers in place on y), backward in place on y = x (reverse order)
int run_dropout(const DropRun &r, int q, const float *x, int ldx, float *y, int ldy, int M, int H, bool backward, hipStream_t st) {
    const gnn_dropout_spec_t &d = *r.d;
    const float *src = x;
    for (int ii = 0; ii < d.n; ++ii) {
        const int i = backward ? d.n - 1 - ii : ii;
        if (d.pos[i] != q) continue;
        TRY(gnn_dropout(src, src == x ? ldx : ldy, y, ldy, M, H, d.rate[i], drop_key(r.seed, (unsigned)d.net_id, (unsigned)r.call, (unsigned)d.index[i]), d.alpha,
                        backward ? 1 : 0, (void *)st));
        src = y;
    }
    return 0;
}
// GNN_FLAG_TRAIN_DROPOUT_FRONT as a plan reads it: whole calls of homogeneous models (no convergence groups)
inline bool dropout_front_asked(const gnn_train_args_t &ta) {
    return (ta.loop.flags & GNN_FLAG_TRAIN_DROPOUT_FRONT) != 0 && !ta.loop.composite && ta.n_groups == 0;
}
int check_dropout(const gnn_dropout_spec_t &d, const gnn_mlp_t &m, const char *name, bool front_ok = false) {
    if (d.n < 0 || d.n > GNN_MAX_DROPOUT) return fail("%s: %d dropout layers (0 .. %d)", name, d.n, GNN_MAX_DROPOUT);
    for (int i = 0; i < d.n; ++i) {
        if (d.pos[i] == 0 && !front_ok) return not_covered("%s: Dropout in front of the first Dense layer (position 0): such networks train through the building blocks", name);
        if (d.pos[i] == 0 && i > 0 && d.pos[i - 1] == 0) return not_covered("%s: two Dropout layers in front of the first Dense layer (position 0): such networks train through the building blocks", name);
        if (d.pos[i] < 0 || d.pos[i] > m.n_layers || (i > 0 && d.pos[i] < d.pos[i - 1])) return fail("%s: dropout positions must ascend within [1, n_layers]", name);
        if (!(d.rate[i] > 0.0f && d.rate[i] < 1.0f)) return fail("%s: dropout rate %g outside (0, 1)", name, (double)d.rate[i]);
    }
    return 0;
}

// Bytes of neighbour sums the tape may keep (one N x S matrix per iteration) instead of recomputing each in the backward sweep.
// Sized for a 288 GB device: 32 GiB by default (C4 with 50 iterations is 12.8 GB), GNN_TRAIN_TAPE_MB overrides.
inline size_t agg_tape_budget() {
    static size_t v = 0;
    if (v == 0) { const char *e = getenv("GNN_TRAIN_TAPE_MB"); v = (e ? (size_t)atol(e) : (size_t)32 * 1024) << 20; v = std::max<size_t>(v, 1); }
    return v;
}

// Which kernels run the iterations of a step: one launch per layer (and node type) and iteration; the persistent small-graph kernels
// (kernels_train_small.hpp: all iterations of a sweep in one launch); the row-streaming large-graph kernels (kernels_train_big.hpp).
// Decided by homogeneous_train_path() below and composite_train_path() (train_composite.hpp), from the conditions written out here.
enum class TrainPath { general, small, big };

// What the plans of both model kinds hold alike (TrainPlan below, CPlan in train_composite.hpp): the phases both steps share take this.
struct StepPlan {
    int N, E, S, L, A, M, R, T, K, G;
    bool pooled, agg_taped;      // agg_taped: every iteration's neighbour sum is kept (small graphs) instead of recomputed
    TrainPath path;
    bool head_fast;              // large graphs: thin output head (one Dense of <= 4 units over EVERY node) on the row-streaming head kernels;
                                 // demoted at run time (read_k: out_index is not the identity) and in phase 2
    int *grads_ok;               // FIRST word of the tape: validity of the step's gradients (gnn_train_args_t::grads_ok_dev)
    int *flags; float *k_dev, *states, *agg;
    int SPs, ldS, n_wg;          // small path: the padded state width the persistent kernels run (16 / 32 / 64), the tape's row stride, the tiles
    float *sm_cc, *sm_part; unsigned long long *sm_bar;
    bool hid_small;              // small path, hidden-layer form (GNN_FLAG_TRAIN_HIDDEN_SMALL; homogeneous models): the state network is two Dense layers
    float *sm_hid, *sm_partW2;   // ... its hidden rows on the tape [K][N][ldS], every workgroup's share of the second layer's gradients
    bool drop_small;             // small path, Dropout form (GNN_FLAG_TRAIN_DROPOUT_SMALL; homogeneous models): Dropout layers behind the state network's Dense layers
    float *sm_ypre;              // ... with one behind the LAST Dense: its un-dropped input on the tape [K][N][ldS] (the state is the dropped-out copy)
    float *stats_o, *Wf_o, *bf_o, *dx_o_all, *G_state, *G_out, *dpred, *loss_rows, *loss_part;
    int *isrc, *idst;            // arc focus: the end nodes of the masked arcs
    float *part, *part_h; size_t part_floats;
    NetCtx co;
    size_t bytes;
};
// state t and the neighbour sum of iteration t on the tape (rows of ldS floats: padded on the persistent small-graph path)
inline float *state_at(const StepPlan &p, int t) { return p.states + (size_t)t * p.N * p.ldS; }
inline float *agg_at(const StepPlan &p, int t) { return p.agg + (p.agg_taped ? (size_t)t * p.N * p.ldS : 0); }

struct TrainPlan : StepPlan {
    int d, in_s, in_o, H1s, H1o, kdx_s, off_agg;
    bool with_labels, tiled;
    bool front;                           // a Dropout layer in front of a first Dense (GNN_FLAG_TRAIN_DROPOUT_FRONT): the general path, no phases
    float *agg_arcs, *agg_nodes;
    int ld_agg_arcs, ld_agg_nodes;        // A / L for arrays of their own; 32 where they are columns of the constants line (big, Kc > 0)
    float *stats_s, *stats_tpl, *Wf_s, *bf_s, *dx_s_all;
    NetCtx cs;
    // large graphs (kernels_train_big.hpp): constant inputs packed 32 per node, statistics partials of the two producers
    int Kc; gnn::ConstCols cc;
    float *xc, *part_a, *part_y, *part_w;
    // small graphs (kernels_train_small.hpp): the forward / backward iterations as one persistent launch each
    float *sm_partW, *sm_partBN;
    // label gradients (gnn_train_step_ex, not on the row-streaming path): sum_t dZ_t of the first state layer [N][ld_dz], d loss / d state_0
    // [N][SPs] (persistent kernels), the gradients of the own / aggregated label columns [N][L] and of the aggregated arc labels [N][A]
    float *dz_sum, *g0, *lab_own, *lab_agg, *arc_agg; int ld_dz;
};

// ---- the conditions of the two fast paths that both model kinds share (the knobs are read at every call: tests switch them inside one process)
// From this many nodes on a training iteration is bandwidth work and runs the row-streaming kernels (GNN_TRAIN_BIG_MIN_NODES).
inline int train_big_min_nodes() { const char *e = getenv("GNN_TRAIN_BIG_MIN_NODES"); return e ? atoi(e) : 32768; }
constexpr int BIG_AGG_BLOCKS = 4096, BIG_FWD_BLOCKS = 1024, BIG_WGRAD_BLOCKS = 512, BIG_HEAD_BLOCKS = 2048;
// The persistent small-graph kernels need every workgroup resident: one 64-node tile per CU (GNN_TRAIN_SMALL=0 switches them off).
inline bool train_small_enabled() { const char *e = getenv("GNN_TRAIN_SMALL"); return !(e && e[0] == '0'); }
// both fast paths run state networks of ONE Dense layer of the state's width, not softmax
inline bool one_dense_of_state_width(const gnn_mlp_t &m, int S) { return m.n_layers == 1 && m.units[0] == S && m.activation[0] != GNN_ACT_SOFTMAX; }
// the persistent kernels: switched on, below the large-graph threshold, no Dropout in a state network (`drop_s`; their Dropout form asks with false:
// homogeneous_train_path), the padded width at most 64, every tile resident at once (the workgroups meet at grid barriers), every iteration's
// neighbour sum within the aggregate-tape budget (`taped` matrices of N x SPs floats per iteration: the neighbour sums, the hidden rows of the
// hidden-layer form, the un-dropped output of the Dropout form)
inline bool train_small_fits(const StepPlan &p, bool drop_s, int taped = 1) {
    return train_small_enabled() && p.N < train_big_min_nodes() && !drop_s && p.S <= 64 && p.n_wg <= device_cus() &&
           (size_t)taped * std::max(p.K, 1) * p.N * p.SPs * sizeof(float) <= agg_tape_budget();
}
// the hidden-layer form of the persistent kernels (opt-in: GNN_FLAG_TRAIN_HIDDEN_SMALL): Dense(H) - Dense(S), 1 <= H <= the padded state
// width `SPs` the kernels run, neither activation softmax (BatchNormalization sits in front of the first Dense only: the second is local to a tile).
// Padded widths 16 and 32 only: at 64 the backward kernel's second set of accumulators does not fit the register file (it would spill to scratch).
inline bool hidden_dense_of_state_width(const gnn_mlp_t &m, int S, int SPs) {
    return SPs <= 32 && m.n_layers == 2 && m.units[1] == S && m.units[0] >= 1 && m.units[0] <= SPs && m.activation[0] != GNN_ACT_SOFTMAX && m.activation[1] != GNN_ACT_SOFTMAX;
}
// the Dropout form of the persistent kernels (opt-in: GNN_FLAG_TRAIN_DROPOUT_SMALL): at most ONE Dropout / AlphaDropout layer behind each Dense
// layer (positions 1 .. n_layers; position 0 never reaches a plan: check_dropout), padded widths 16 and 32 only - at 64 the one-layer LOCAL
// backward kernel is at 256 + 256 registers with scratch already.  `last` (out): a layer sits behind the last Dense - its un-dropped input is taped.
inline bool dropout_small_form(const gnn_dropout_spec_t &d, int n_layers, int SPs, bool &last) {
    last = false;
    if (SPs > 32 || d.n < 1 || d.n > n_layers) return false;
    for (int i = 0; i < d.n; ++i) {
        if (d.pos[i] < 1 || d.pos[i] > n_layers || (i > 0 && d.pos[i] <= d.pos[i - 1])) return false;
        last |= d.pos[i] == n_layers;
    }
    return true;
}

size_t grad_part_floats(int K, int H, int M) { int nc; rows_per_chunk_for(std::max(M, 1), &nc); return (size_t)nc * ((size_t)K * H + H); }

void carve_net(Carver &c, NetCtx &x, const gnn_mlp_t &m, int rows, size_t &part_floats, const gnn_dropout_spec_t *drop = nullptr) {
    int fan_in = m.in_dim;
    DropRun dr{drop, 0u, 0, {}};
    for (int q = 0; q <= GNN_MAX_LAYERS; ++q) x.dropbuf[q] = nullptr;
    if (drop_at(&dr, 0)) {      // (GNN_FLAG_TRAIN_DROPOUT_FRONT) X0, the normalised and dropped-out input [rows x in_dim] - in the backward pass d loss / d X0; the column partials
        x.dropbuf[0] = c.take<float>((size_t)std::max(rows, 1) * m.in_dim);
        int nc; rows_per_chunk_for(std::max(rows, 1), &nc);
        part_floats = std::max(part_floats, (size_t)nc * 2 * m.in_dim);
    }
    for (int q = 1; q <= m.n_layers; ++q)
        if (drop_at(&dr, q)) x.dropbuf[q] = c.take<float>((size_t)std::max(rows, 1) * m.units[q - 1]);
    for (int l = 0; l < m.n_layers; ++l) {
        x.Wt[l] = c.take<float>((size_t)fan_in * m.units[l]);
        x.hid[l] = c.take<float>((size_t)std::max(rows, 1) * m.units[l]);
        part_floats = std::max(part_floats, grad_part_floats(fan_in, m.units[l], rows));
        fan_in = m.units[l];
    }
    x.P = c.take<float>((size_t)m.in_dim * m.units[0]); x.q = c.take<float>(m.units[0]);
    x.m1 = c.take<float>(m.in_dim); x.m2 = c.take<float>(m.in_dim);
    const int mu = std::max(max_units(m), 1);
    x.G[0] = c.take<float>((size_t)std::max(rows, 1) * mu); x.G[1] = c.take<float>((size_t)std::max(rows, 1) * mu);
}

// Which path a homogeneous step takes (dims, Kc, SPs and n_wg of `p` are set).  Both fast paths want one Dense layer without Dropout, at least one
// iteration and at most 32 constant input columns (one line per node); the row-streaming kernels exist for state widths 16 / 32 / 64 and address the
// state through 4 GiB windows; the persistent kernels pad the width to 16 / 32 / 64 inside the tape (the starter configuration's 14 label columns).
// `hidden` (out): the persistent kernels in their hidden-layer form - asked for by GNN_FLAG_TRAIN_HIDDEN_SMALL, a network
// hidden_dense_of_state_width() accepts, and every condition of the persistent path with the hidden rows counted on the tape beside the
// neighbour sums; with the flag set every other shape is routed exactly as without it.
// `dropped` (out): the persistent kernels in their Dropout form - asked for by GNN_FLAG_TRAIN_DROPOUT_SMALL, Dropout layers dropout_small_form()
// accepts behind one Dense of the state width (or, with GNN_FLAG_TRAIN_HIDDEN_SMALL as well, behind the layers of a network
// hidden_dense_of_state_width() accepts), and every condition of the persistent path with what the form tapes counted: the neighbour sums, the hidden
// rows, the un-dropped input of a layer behind the last Dense.  Every other shape with Dropout is routed exactly as without the flag.
TrainPath homogeneous_train_path(const gnn_train_args_t &ta, const TrainPlan &p, bool &hidden, bool &dropped) {
    const bool drop_s = ta.drop_state[0].n > 0;
    const gnn_mlp_t &m = ta.loop.net_state[0];
    hidden = dropped = false;
    // a layer in front of a first Dense (GNN_FLAG_TRAIN_DROPOUT_FRONT; either network): the general kernels, whatever else is asked for
    if (drop_at_position(ta.drop_state[0], 0) || drop_at_position(ta.drop_output, 0)) return TrainPath::general;
    if (drop_s && (ta.loop.flags & GNN_FLAG_TRAIN_DROPOUT_SMALL) != 0 && p.K >= 1 && p.Kc <= 32) {
        const bool hid = (ta.loop.flags & GNN_FLAG_TRAIN_HIDDEN_SMALL) != 0 && hidden_dense_of_state_width(m, p.S, p.SPs);
        bool last = false;
        if ((hid || one_dense_of_state_width(m, p.S)) && dropout_small_form(ta.drop_state[0], m.n_layers, p.SPs, last) &&
            train_small_fits(p, false, 1 + (hid ? 1 : 0) + (last ? 1 : 0))) {
            hidden = hid; dropped = true;
            return TrainPath::small;
        }
    }
    hidden = (ta.loop.flags & GNN_FLAG_TRAIN_HIDDEN_SMALL) != 0 && hidden_dense_of_state_width(ta.loop.net_state[0], p.S, p.SPs) && !drop_s && p.K >= 1 &&
             p.Kc <= 32 && train_small_fits(p, drop_s, 2);
    if (hidden) return TrainPath::small;
    if (!one_dense_of_state_width(ta.loop.net_state[0], p.S) || drop_s || p.K <= 0 || p.Kc > 32) return TrainPath::general;
    if (p.N >= train_big_min_nodes())
        return ((p.S == 16 || p.S == 32 || p.S == 64) && (size_t)p.N * p.S * 4 < ((size_t)1 << 32)) ? TrainPath::big : TrainPath::general;
    return train_small_fits(p, drop_s) ? TrainPath::small : TrainPath::general;
}

int make_train_plan(const gnn_train_args_t &ta, void *ws, TrainPlan &p) {
    const gnn_loop_args_t &a = ta.loop;
    memset(&p, 0, sizeof(p));
    if (a.abi_version != GNN_ABI_VERSION) return fail("abi_version %d != %d", a.abi_version, GNN_ABI_VERSION);
    if (a.composite) return not_covered("gnn_train_step: homogeneous models only");
    if (a.n_nodes < 1) return not_covered("gnn_train_step: empty graph");
    // (a.n_heavy_segments > 0: the training kernels walk the plain adjacency all the same)
    p.N = a.n_nodes; p.E = a.n_arcs; p.L = a.dim_node_label; p.A = a.dim_arc_label; p.d = a.state_dim;
    p.S = a.state_dim > 0 ? a.state_dim : a.dim_node_label;
    p.K = a.max_iteration; p.M = a.n_out;
    TRY(check_mlp(a.net_state[0], "net_state", ws != nullptr));
    TRY(check_mlp(a.net_output, "net_output", ws != nullptr));
    const gnn_mlp_t &ns = a.net_state[0], &no = a.net_output;
    TRY(check_dropout(ta.drop_state[0], ns, "net_state", dropout_front_asked(ta)));
    TRY(check_dropout(ta.drop_output, no, "net_output", dropout_front_asked(ta)));
    p.front = drop_at_position(ta.drop_state[0], 0) || drop_at_position(ta.drop_output, 0);
    p.with_labels = a.state_dim > 0;
    p.in_s = ns.in_dim; p.in_o = no.in_dim; p.H1s = ns.units[0]; p.H1o = no.units[0];
    const int expect_s = a.state_dim > 0 ? 2 * p.S + 2 * p.L + p.A : 2 * p.S + p.A;
    if (ns.in_dim != expect_s) return fail("net_state.in_dim %d != %d expected from the graph dims", ns.in_dim, expect_s);
    if (ns.units[ns.n_layers - 1] != p.S) return fail("net_state output width %d != state width %d", ns.units[ns.n_layers - 1], p.S);
    const int node_part = p.with_labels ? p.S + p.L : p.S;
    const int expect_o = a.focus == GNN_FOCUS_ARC ? 2 * node_part + p.A : node_part;
    if (no.in_dim != expect_o) return fail("net_output.in_dim %d != %d expected for this focus", no.in_dim, expect_o);
    p.T = no.units[no.n_layers - 1];
    p.pooled = a.focus == GNN_FOCUS_GRAPH;
    p.G = p.pooled ? a.nodegraph.n_dst : 0;
    p.R = p.pooled ? p.G : p.M;
    p.off_agg = p.with_labels ? p.S + p.L : p.S;          // first-layer row (= BN column) of the aggregated-state segment
    p.kdx_s = 2 * p.S;                                     // d loss / d [state | agg] only, 16-B aligned halves: the label columns between them are never needed

    p.Kc = (p.with_labels ? 2 * p.L : 0) + p.A;
    p.SPs = p.S <= 16 ? 16 : p.S <= 32 ? 32 : 64;
    p.tiled = ta.n_tiles > 0 && ta.tile_node_begin != nullptr;
    p.n_wg = p.tiled ? ta.n_tiles : cdiv(p.N, 64);
    if (p.tiled && p.n_wg > 256) { p.tiled = false; p.n_wg = cdiv(p.N, 64); }
    p.path = homogeneous_train_path(ta, p, p.hid_small, p.drop_small);
    const bool big = p.path == TrainPath::big, small = p.path == TrainPath::small;
    // every node is an output row (out_index ascending and n_out == n_nodes: the identity), one thin Dense: kernels_train_big.hpp
    p.head_fast = big && no.n_layers == 1 && no.units[0] <= 4 && a.focus != GNN_FOCUS_ARC && p.M == p.N && p.S % 4 == 0 &&
                  p.S / 4 + ((p.with_labels ? p.L : 0) + 3) / 4 <= 32 && ta.drop_output.n == 0;
    p.ldS = small ? p.SPs : p.S;

    Carver c(ws);
    p.grads_ok = c.take<int>(4);                           // (offset 0 whatever the plan: the next call on this tape reads it back)
    p.flags = c.take<int>(p.K + 8);
    p.k_dev = c.take<float>(4);
    p.states = c.take<float>((size_t)(p.K + 1) * p.N * p.ldS);
    p.agg_taped = (size_t)std::max(p.K, 1) * p.N * p.ldS * sizeof(float) <= agg_tape_budget();
    p.agg = c.take<float>((size_t)(p.agg_taped ? std::max(p.K, 1) : 1) * p.N * p.ldS);
    p.agg_arcs = c.take<float>((size_t)p.N * std::max(p.A, 1));
    p.agg_nodes = c.take<float>((size_t)p.N * std::max(p.L, 1));
    p.ld_agg_arcs = p.A; p.ld_agg_nodes = p.L;
    p.stats_s = c.take<float>((size_t)(std::max(p.K, 1) + 1) * 2 * p.in_s);      // (+ 1: the statistics of the LAST state, for the output head's BatchNormalization)
    p.stats_tpl = c.take<float>(2 * (size_t)p.in_s);
    p.Wf_s = c.take<float>((size_t)std::max(p.K, 1) * p.in_s * p.H1s);
    p.bf_s = c.take<float>((size_t)std::max(p.K, 1) * p.H1s);
    p.stats_o = c.take<float>(2 * (size_t)p.in_o);
    p.Wf_o = c.take<float>((size_t)p.in_o * p.H1o); p.bf_o = c.take<float>(p.H1o);
    p.dx_s_all = c.take<float>((size_t)p.N * std::max(p.kdx_s, small ? p.SPs : 0));      // (also the persistent backward kernel's [N, SPs] exchange rows)
    p.dx_o_all = c.take<float>((size_t)std::max(p.M, 1) * p.in_o);
    p.G_state = c.take<float>((size_t)p.N * p.S);
    p.G_out = c.take<float>((size_t)std::max(p.M, 1) * p.T);
    p.dpred = c.take<float>((size_t)std::max(p.R, 1) * p.T);
    p.loss_rows = c.take<float>(std::max(p.R, 1));
    p.isrc = c.take<int>(std::max(p.M, 1)); p.idst = c.take<int>(std::max(p.M, 1));
    p.part_floats = 0;
    carve_net(c, p.cs, ns, p.N, p.part_floats, &ta.drop_state[0]);
    carve_net(c, p.co, no, p.M, p.part_floats, &ta.drop_output);
    {   // column-statistics partials of the large-batch path: (chunks + 1) x widest segment
        int nc; rows_per_chunk_for(std::max(p.N, 1), &nc);
        p.part_floats = std::max(p.part_floats, (size_t)(nc + 1) * std::max(p.in_s, p.in_o));
    }
    p.part = c.take<float>(p.part_floats);
    memset(&p.cc, 0, sizeof(p.cc));
    if (p.with_labels) {
        p.cc.n = p.A > 0 ? 3 : 2;
        p.cc.width[0] = p.L; p.cc.wrow[0] = p.S;
        p.cc.width[1] = p.L; p.cc.wrow[1] = 2 * p.S + p.L;
        p.cc.width[2] = p.A; p.cc.wrow[2] = 2 * p.S + 2 * p.L;
    } else {
        p.cc.n = p.A > 0 ? 1 : 0;
        p.cc.width[0] = p.A; p.cc.wrow[0] = 2 * p.S;
    }
    p.xc = c.take<float>(big && p.Kc > 0 ? (size_t)p.N * 32 : 0);
    if (big && p.Kc > 0) {       // the large-graph kernels read a node's constant inputs as one line (fill_constants_line), the caller's if there
        if (ta.loop.xc) p.xc = ta.loop.xc;      // is one (gnn_loop_args_t::xc); whoever still wants an aggregate as a segment reads its columns of the line
        const int L0 = p.with_labels ? p.L : 0;
        p.agg_nodes = p.xc + L0; p.agg_arcs = p.xc + 2 * L0;
        p.ld_agg_arcs = p.ld_agg_nodes = 32;
    }
    p.part_a = c.take<float>(big ? (size_t)BIG_AGG_BLOCKS * 2 * p.S : 0);
    p.part_y = c.take<float>(big ? (size_t)BIG_FWD_BLOCKS * 2 * std::max(p.S, 32) : 0);      // (also the one-pass statistics of the 32-wide constants line)
    p.loss_part = c.take<float>(256);
    p.part_w = c.take<float>(big ? (size_t)BIG_WGRAD_BLOCKS * ((size_t)p.in_s * p.S + p.S) : 0);      // k_train_wgrad: one partial per workgroup
    p.part_h = c.take<float>(p.head_fast ? (size_t)BIG_HEAD_BLOCKS * ((size_t)p.in_o * p.H1o + p.H1o) : 0);             // k_head_wgrad: one partial per workgroup
    p.sm_cc = c.take<float>(small ? (size_t)p.N * p.SPs : 0);
    p.sm_part = c.take<float>(small ? (size_t)2 * p.n_wg * 8 * p.SPs : 0);
    p.sm_partW = c.take<float>(small ? (size_t)p.n_wg * (p.in_s + 1) * p.H1s : 0);
    p.sm_partBN = c.take<float>(small ? (size_t)p.n_wg * 2 * p.in_s : 0);
    p.sm_bar = c.take<unsigned long long>(small ? 4 : 0);
    p.sm_hid = c.take<float>(p.hid_small ? (size_t)p.K * p.N * p.ldS : 0);
    p.sm_partW2 = c.take<float>(p.hid_small ? (size_t)p.n_wg * (p.H1s + 1) * p.S : 0);
    p.sm_ypre = c.take<float>(p.drop_small && drop_at_position(ta.drop_state[0], ns.n_layers) ? (size_t)p.K * p.N * p.ldS : 0);
    p.ld_dz = small ? p.SPs : p.H1s;
    p.dz_sum = c.take<float>(big ? 0 : (size_t)p.N * p.ld_dz);
    p.g0 = c.take<float>(small ? (size_t)p.N * p.SPs : 0);
    p.lab_own = c.take<float>(big ? 0 : (size_t)p.N * std::max(p.L, 1));
    p.lab_agg = c.take<float>(big ? 0 : (size_t)p.N * std::max(p.L, 1));
    p.arc_agg = c.take<float>(big ? 0 : (size_t)p.N * std::max(p.A, 1));
    p.cs.m = &ns; p.cs.g = &ta.grad_state; p.co.m = &no; p.co.g = &ta.grad_output;
    p.bytes = (c.off + 255) & ~(size_t)255;
    return 0;
}

// ---- column statistics of the listed segments into mean / var (positions seg.wrow) --------------------------------------
int colstats_segs(const int *gate, const gnn::Seg *segs, int n, int M, float *mean, float *var, float *part, hipStream_t st) {
    if (n == 0) return 0;
    if (M <= 8192) {
        gnn::StatSegs ss{};
        ss.n = n; ss.col_begin[0] = 0;
        for (int s = 0; s < n; ++s) { ss.seg[s] = segs[s]; ss.col_begin[s + 1] = ss.col_begin[s] + segs[s].width; }
        gnn::k_colstats_segs_small<<<ss.col_begin[n], 256, 0, st>>>(gate, ss, M, mean, var);
        LAUNCH_OK();
        return 0;
    }
    int n_chunks;
    const int rpc = rows_per_chunk_for(M, &n_chunks);
    for (int s = 0; s < n; ++s) {       // large batches: two passes per segment (launch count does not matter there)
        const gnn::Seg &g = segs[s];
        gnn::k_colstats_partial<<<n_chunks, 256, 0, st>>>(g.ptr, g.ld, g.rowidx, g.width, M, rpc, nullptr, part);
        LAUNCH_OK();
        gnn::k_reduce_partials<<<cdiv(g.width, 64), 256, 0, st>>>(part, n_chunks, g.width, mean + g.wrow, 0, 1.0f / (float)M, g.width, nullptr);
        LAUNCH_OK();
        gnn::k_colstats_partial<<<n_chunks, 256, 0, st>>>(g.ptr, g.ld, g.rowidx, g.width, M, rpc, mean + g.wrow, part);
        LAUNCH_OK();
        gnn::k_reduce_partials<<<cdiv(g.width, 64), 256, 0, st>>>(part, n_chunks, g.width, var + g.wrow, 0, 1.0f / (float)M, g.width, nullptr);
        LAUNCH_OK();
    }
    return 0;
}

int fold_with_stats(const gnn_mlp_t &m, const float *stats, float *Wf, float *bf, hipStream_t st, bool centred = false) {
    FoldList fl;
    gnn::FoldJob &j = fl.fa.job[fl.fa.n_jobs++];
    j.centred = centred ? 1 : 0;
    j.W = m.kernel[0]; j.b = m.bias[0]; j.K = m.in_dim; j.H = m.units[0];
    j.gamma = m.bn_gamma; j.beta = m.bn_beta; j.mean = stats; j.var = stats + m.in_dim; j.eps = m.bn_eps;
    j.Wf = Wf; j.bf = bf; j.blk_begin = 0;
    fl.blocks = j.H;
    return launch_fold_list(fl, st);
}

// ---- a Dropout layer in front of the first Dense (position 0, GNN_FLAG_TRAIN_DROPOUT_FRONT; kernels_train_front.hpp) -----------------------
// the one layer at position 0 of the run's network: its key for this call and the scalars gnn_dropout() derives for it
struct FrontLayer { unsigned key; DropScalars sc; };
inline FrontLayer front_layer_of(const DropRun &r, bool backward) {
    const gnn_dropout_spec_t &d = *r.d;
    int i = 0;
    while (i < d.n - 1 && d.pos[i] != 0) ++i;
    return FrontLayer{drop_key(r.seed, (unsigned)d.net_id, (unsigned)r.call, (unsigned)d.index[i]), drop_scalars(d.rate[i], d.alpha, backward)};
}
inline gnn::FrontSegs front_segs(const gnn::Seg *segs, int nseg) {
    gnn::FrontSegs fs{};
    fs.n = nseg;
    for (int s = 0; s < nseg; ++s) fs.seg[s] = segs[s];
    return fs;
}
// forward: X0 = r.buf[0] [M x in_dim] from the segments, BatchNormalization on `bn_stats` (mean | var; NULL: none) applied on load
int front_input(const gnn_mlp_t &m, const gnn::Seg *segs, int nseg, int M, const float *bn_stats, const DropRun &r, const int *gate, hipStream_t st) {
    if (M == 0) return 0;
    if (!r.buf[0]) return fail("front_input: no buffer for the dropped-out input");
    const FrontLayer f = front_layer_of(r, false);
    gnn::FrontFwdArgs a{};
    a.gate = gate; a.in = front_segs(segs, nseg); a.M = M; a.K = m.in_dim;
    if (m.has_bn && bn_stats) { a.gamma = m.bn_gamma; a.beta = m.bn_beta; a.mean = bn_stats; a.var = bn_stats + m.in_dim; a.eps = m.bn_eps; }
    a.key = f.key; a.thr = f.sc.thr; a.mul = f.sc.mul; a.add = f.sc.add; a.fill = f.sc.fill;
    a.X0 = r.buf[0];
    gnn::k_front_input<<<std::min(cdiv(M, 4 * gnn::FRONT_ROWS), 2048), 256, 0, st>>>(a);
    LAUNCH_OK();
    return 0;
}
// backward: dX0 [M x in_dim] through the masks into the wanted columns of dx_all (see k_front_input_grad), and - BatchNormalization on
// `stats` - d gamma, d beta and the moments m1 / m2 of the input gradient from the chunk partials in `part`
int front_input_grad(NetCtx &x, const gnn::Seg *segs, int nseg, int M, const float *stats, const DropRun &r, const float *dX0, bool accumulate,
                     float *dx_all, int kdx, int first_col, int second_row, float *part, hipStream_t st) {
    const gnn_mlp_t &m = *x.m;
    const FrontLayer f = front_layer_of(r, true);
    const bool bn = m.has_bn && stats;
    int n_chunks;
    const int rpc = rows_per_chunk_for(std::max(M, 1), &n_chunks);
    gnn::FrontBwdArgs a{};
    a.in = front_segs(segs, nseg); a.M = M; a.K = m.in_dim; a.rows_per_chunk = rpc;
    a.mean = bn ? stats : nullptr;
    a.key = f.key; a.thr = f.sc.thr; a.mul = f.sc.mul;
    a.dX0 = dX0;
    if (dx_all && kdx > 0) {
        a.dx = dx_all; a.ld_dx = kdx; a.col_a = first_col;
        if (second_row < 0) { a.half = kdx; a.col_b = -1; } else { a.half = kdx / 2; a.col_b = second_row; }
    }
    a.part = part;
    gnn::k_front_input_grad<<<dim3(n_chunks, cdiv(m.in_dim, 64)), 256, 0, st>>>(a);
    LAUNCH_OK();
    if (bn) {
        gnn::k_front_bn_finish<<<cdiv(m.in_dim, 64), 256, 0, st>>>(part, n_chunks, m.in_dim, stats + m.in_dim, m.bn_eps, 1.0f / (float)M, x.g->dgamma, x.g->dbeta,
                                                                 x.m1, x.m2, accumulate ? 1 : 0);
        LAUNCH_OK();
    }
    return 0;
}

// layers of `m` over a virtual concatenation; first layer with (W0, b0); outputs into hs[l] (ld = units[l])
struct PredFuse { const float *old; int ld; float thr; int *flag; float *k_out; float k_val; bool fused; };

// `bn_stats` (mean | var of the first layer's input columns): the training-mode BatchNormalization is applied to the inputs as
// the first layer stages them (k_segdense), with (W0, b0) the raw kernel / bias; NULL: (W0, b0) are used as they are.
// `center` (the column means, by weight row): (W0, b0) is a CENTRED fold (fold_with_stats(.., true)) and the first layer subtracts
// the means from its inputs as it stages them (layers whose kernel wants folded weights: the thin-output kernel).
// `drop`: the network's Dropout layers (positions >= 1): hs[l] stay the layers' own outputs, what the next Dense consumes is drop->buf[l + 1];
// the network's output is then drop->buf[n_layers] when a layer sits behind the last Dense (`skip_last_drop`: a backward recompute, which
// does not need it).
// A Dropout layer in FRONT of the first Dense (GNN_FLAG_TRAIN_DROPOUT_FRONT): the first layer then is (W0, b0) = the raw kernel / bias over
// X0 = drop->buf[0], which front_input() makes of the segments - normalised with `bn_stats` (NULL: as they are), dropped out - in one launch.
int forward_layers(const gnn_mlp_t &m, const gnn::Seg *segs, int nseg, int M, const float *W0, const float *b0, float *const *hs,
                   const int *gate, hipStream_t st, PredFuse *pred = nullptr, const float *bn_stats = nullptr, const float *center = nullptr,
                   const DropRun *drop = nullptr, bool skip_last_drop = false) {
    for (int l = 0; l < m.n_layers; ++l) {
        gnn::SegDenseArgs a{};
        a.gate = gate; a.M = M; a.H = m.units[l];
        if (l == 0 && drop_at(drop, 0)) {
            if (center) return fail("forward_layers: a Dropout layer in front of the first Dense takes the raw first layer, not a centred fold");
            TRY(front_input(m, segs, nseg, M, bn_stats, *drop, gate, st));
            a.nseg = 1;
            a.seg[0] = gnn::Seg{drop->buf[0], nullptr, (int)m.in_dim, (int)m.in_dim, 0};
            a.W = W0; a.bias = b0;
        } else if (l == 0) {
            a.nseg = nseg;
            for (int s = 0; s < nseg; ++s) a.seg[s] = segs[s];
            a.W = W0; a.bias = b0;
            if (bn_stats) { a.in_gamma = m.bn_gamma; a.in_beta = m.bn_beta; a.in_mean = bn_stats; a.in_var = bn_stats + m.in_dim; a.in_eps = m.bn_eps; }
            else a.in_center = center;
        } else {
            const float *src = hs[l - 1];
            if (drop_at(drop, l)) {
                TRY(run_dropout(*drop, l, hs[l - 1], m.units[l - 1], drop->buf[l], m.units[l - 1], M, m.units[l - 1], false, st));
                src = drop->buf[l];
            }
            a.nseg = 1;
            a.seg[0] = gnn::Seg{src, nullptr, (int)m.units[l - 1], (int)m.units[l - 1], 0};
            a.W = m.kernel[l]; a.bias = m.bias[l];
        }
        a.ldw = a.H;
        const bool thin_softmax = m.activation[l] == GNN_ACT_SOFTMAX && thin_dense_applies(a);
        a.act = (m.activation[l] == GNN_ACT_SOFTMAX && !thin_softmax) ? GNN_ACT_LINEAR : m.activation[l];
        a.Y = hs[l]; a.ldy = m.units[l];
        if (pred && l == m.n_layers - 1 && a.H <= 64 && a.H > 4 && m.activation[l] != GNN_ACT_SOFTMAX && !drop_at(drop, m.n_layers)) {   // predicate in the epilogue
            a.pred_old = pred->old; a.ld_pred = pred->ld; a.pred_thr = pred->thr; a.pred_flag = pred->flag;
            a.pred_k = pred->k_out; a.pred_kval = pred->k_val;
            pred->fused = true;
        }
        TRY(launch_segdense(a, st));
        if (m.activation[l] == GNN_ACT_SOFTMAX && !thin_softmax) TRY(launch_softmax(gate, a.Y, a.M, a.H, a.ldy, nullptr, st));
    }
    if (!skip_last_drop && drop_at(drop, m.n_layers)) {
        const int H = m.units[m.n_layers - 1];
        TRY(run_dropout(*drop, m.n_layers, hs[m.n_layers - 1], H, drop->buf[m.n_layers], H, M, H, false, st));
    }
    return 0;
}

int dense_plain(const float *X, int ldx, int K, const float *W, int ldw, int H, int M, float *Y, int ldy, hipStream_t st) {
    gnn::SegDenseArgs a{};
    a.M = M; a.H = H; a.nseg = 1;
    a.seg[0] = gnn::Seg{X, nullptr, ldx, K, 0};
    a.W = W; a.ldw = ldw; a.act = GNN_ACT_LINEAR; a.Y = Y; a.ldy = ldy;
    return launch_segdense(a, st);
}

int act_grad_inplace(float *G, int ldg, const float *Y, int ldy, int M, int H, int act, hipStream_t st) {
    if (M == 0) return 0;
    const long total = act == GNN_ACT_SOFTMAX ? M : (long)M * H;
    gnn::k_act_grad<<<std::min(cdiv(total, 256), 256 * 16), 256, 0, st>>>(G, ldg, Y, ldy, G, ldg, M, H, act);
    LAUNCH_OK();
    return 0;
}

// Back-propagation through one network.  G = d loss / d hs[last] ([M x units_last], leading dimension ldg; overwritten).
// Parameter gradients go to x.g (accumulated when `accumulate`); dx_all (optional) receives d loss / d input columns
// [0, kdx) BEFORE the BatchNormalization input gradient (the caller applies it to the segments it needs).
// `second_row` >= 0: dx_all is [M x kdx] = columns [0, kdx/2) of the input followed by columns [second_row, second_row + kdx/2);
// `first_col`: the block starts at that input column instead of 0 (composite models: the state segment sits behind the type's labels).
// `drop`: the Dropout layers of this call (their forward copies in drop->buf[]; the masks are regenerated from the call's keys).
int net_backward(NetCtx &x, const gnn::Seg *segs, int nseg, float *const *hs, float *G, int ldg, int M, const float *stats, bool accumulate,
                 float *dx_all, int kdx, float *part, hipStream_t st, int second_row = -1, int first_col = 0, const DropRun *drop = nullptr,
                 float *dz_acc = nullptr) {
    const gnn_mlp_t &m = *x.m;
    int n_chunks;
    const int rpc = rows_per_chunk_for(std::max(M, 1), &n_chunks);
    if (drop_at(drop, m.n_layers) && M > 0) TRY(run_dropout(*drop, m.n_layers, G, ldg, G, ldg, M, m.units[m.n_layers - 1], true, st));
    for (int l = m.n_layers - 1; l >= 1; --l) {
        const int H = m.units[l], Kp = m.units[l - 1];
        TRY(act_grad_inplace(G, ldg, hs[l], H, M, H, m.activation[l], st));
        dim3 grid(n_chunks, cdiv(Kp, 64), cdiv(H, 64));
        gnn::k_dense_grad_partial<<<grid, 256, 0, st>>>(drop_at(drop, l) ? drop->buf[l] : hs[l - 1], Kp, nullptr, Kp, G, ldg, H, M, rpc, part, 1);
        LAUNCH_OK();
        const int n = Kp * H + H;
        gnn::k_reduce_partials<<<cdiv(n, 64), 256, 0, st>>>(part, n_chunks, n, x.g->dkernel[l], accumulate ? 1 : 0, 1.0f, Kp * H, x.g->dbias[l]);
        LAUNCH_OK();
        float *Gn = (G == x.G[0]) ? x.G[1] : x.G[0];
        TRY(dense_plain(G, ldg, H, x.Wt[l], Kp, Kp, M, Gn, Kp, st));      // dL/d (input of Dense l) = dZ . W[l]^T
        if (drop_at(drop, l) && M > 0) TRY(run_dropout(*drop, l, Gn, Kp, Gn, Kp, M, Kp, true, st));      // ... through the Dropout layers in front of it
        G = Gn; ldg = Kp;
    }
    const int H = m.units[0], K = m.in_dim;
    int Kv = 0;
    for (int s = 0; s < nseg; ++s) Kv += segs[s].width;
    const bool allk = Kv == K && K <= 192 && H <= 64 && n_chunks >= 256;
    TRY(act_grad_inplace(G, ldg, hs[0], H, M, H, m.activation[0], st));
    if (dz_acc && M > 0) {            // label gradients: sum over the iterations of the first layer's dZ ([M x H], kernels_train_labels.hpp)
        if (ldg != H) return fail("net_backward: dZ of the first layer is not contiguous");
        gnn::k_axpby<<<std::min(cdiv((long)M * H, 256), 1024), 256, 0, st>>>(1.0f, G, 1.0f, dz_acc, dz_acc, (size_t)M * H);
        LAUNCH_OK();
    }
    if (drop_at(drop, 0)) {
        // A Dropout layer in front of the first Dense (GNN_FLAG_TRAIN_DROPOUT_FRONT): Dense 0 is a plain layer over X0 = drop->buf[0], like the
        // layers above; d loss / d X0 = dZ . W0^T then passes the masks and meets BatchNormalization - the first-layer algebra with W = I.
        // (d loss / d X0 overwrites X0: the weight-gradient launch in front of it was X0's last reader.)
        if (M == 0) return 0;
        float *X0 = drop->buf[0];
        dim3 grid(n_chunks, cdiv(K, 64), cdiv(H, 64));
        gnn::k_dense_grad_partial<<<grid, 256, 0, st>>>(X0, K, nullptr, K, G, ldg, H, M, rpc, part, 1);
        LAUNCH_OK();
        const int n = K * H + H;
        gnn::k_reduce_partials<<<cdiv(n, 64), 256, 0, st>>>(part, n_chunks, n, x.g->dkernel[0], accumulate ? 1 : 0, 1.0f, K * H, x.g->dbias[0]);
        LAUNCH_OK();
        TRY(dense_plain(G, ldg, H, x.Wt[0], K, K, M, X0, K, st));
        return front_input_grad(x, segs, nseg, M, stats, *drop, X0, accumulate, dx_all, kdx, first_col, second_row, part, st);
    }
    {
        gnn::GradSegs gs{};
        gs.n = nseg; gs.blk_begin[0] = 0;
        gs.mean = (m.has_bn && stats) ? stats : nullptr;      // (rows centred as they are staged: see GradSegs::mean)
        for (int s = 0; s < nseg; ++s) { gs.seg[s] = segs[s]; gs.blk_begin[s + 1] = gs.blk_begin[s] + cdiv(segs[s].width, 64); }
        if (allk) {     // every column in one workgroup: dZ is read once (kernels_train.hpp)
            gnn::k_dense_grad_allk<<<n_chunks, 256, 0, st>>>(gs, K, G, ldg, H, M, rpc, part);
        } else {
            dim3 grid(n_chunks, gs.blk_begin[nseg], cdiv(H, 64));
            gnn::k_dense_grad_partial_segs<<<grid, 256, 0, st>>>(gs, K, G, ldg, H, M, rpc, part);
        }
        LAUNCH_OK();
    }
    const bool bn = m.has_bn != 0;
    const float *Pp = x.P, *qp = x.q;
    int fuse_chunks = 1;
    if (n_chunks <= 32) {                      // small batches: the chunk partials are summed inside the parameter-gradient kernel
        Pp = part; qp = part + (size_t)K * H; fuse_chunks = n_chunks;
    } else {
        const int n = K * H + H;
        gnn::k_reduce_partials<<<cdiv(n, 64), 256, 0, st>>>(part, n_chunks, n, x.P, 0, 1.0f, K * H, x.q);
        LAUNCH_OK();
    }
    gnn::k_first_layer_param_grads<<<K, 64, 0, st>>>(
        Pp, qp, m.kernel[0], K, H, bn ? m.bn_gamma : nullptr, m.bn_beta, stats, stats ? stats + K : nullptr, m.bn_eps, 1.0f / (float)M,
        x.g->dkernel[0], x.g->dbias[0], x.g->dgamma, x.g->dbeta, bn ? x.m1 : nullptr, bn ? x.m2 : nullptr, accumulate ? 1 : 0, fuse_chunks,
        (bn && stats) ? 1 : 0);
    LAUNCH_OK();
    if (dx_all && kdx > 0) {
        if (second_row < 0 || second_row == first_col + kdx / 2) {
            TRY(dense_plain(G, ldg, H, x.Wt[0] + first_col, K, kdx, M, dx_all, kdx, st));   // W^T columns [first_col, first_col + kdx) (ldw = K)
        } else {
            TRY(dense_plain(G, ldg, H, x.Wt[0] + first_col, K, kdx / 2, M, dx_all, kdx, st));
            TRY(dense_plain(G, ldg, H, x.Wt[0] + second_row, K, kdx / 2, M, dx_all + kdx / 2, kdx, st));
        }
    }
    return 0;
}

int bn_input_grads(const gnn_mlp_t &m, const NetCtx &x, const float *stats, const gnn::BnGradReq *reqs, int n, int M, hipStream_t st) {
    if (!m.has_bn || n == 0 || M == 0) return 0;
    gnn::BnGradArgs a{};
    a.n = n; a.M = M; a.gamma = m.bn_gamma; a.mean = stats; a.var = stats + m.in_dim; a.m1 = x.m1; a.m2 = x.m2; a.eps = m.bn_eps;
    long total = 0;
    for (int i = 0; i < n; ++i) { a.r[i] = reqs[i]; total = std::max(total, (long)M * reqs[i].width); }
    gnn::k_bn_input_grad_segs<<<std::min(cdiv(total, 256), 256 * 16), 256, 0, st>>>(a);
    LAUNCH_OK();
    return 0;
}

// the Dropout run of one call of network `x` (the masks' keys: step seed, network, `call`), its copies in the network's own buffers
DropRun drop_run(const gnn_dropout_spec_t *d, unsigned seed, int call, const NetCtx &x) {
    DropRun r{d, seed, call, {}};
    for (int q = 0; q <= x.m->n_layers; ++q) r.buf[q] = x.dropbuf[q];
    return r;
}

// A state network's first layer in a training-mode forward on the general kernels, BatchNormalization on this iteration's statistics of
// the state / agg segments `dyn` (slot `stats`): a thin first layer (<= 4 units: the thin-dense kernel wants folded weights) gets the
// centred fold in (Wf, bf) and subtracts the means on load; else the normalisation is applied as the layer stages its inputs (no fold launch).
// `front` (a Dropout layer in front of the first Dense): never a fold - the normalisation belongs to the launch that makes X0 (forward_layers)
struct FirstLayer { const float *W0, *b0, *bn_on_load, *centre; };
int first_layer_of(const gnn_mlp_t &ns, const int *gate, const gnn::Seg *dyn, int M, float *stats, float *Wf, float *bf, float *part, FirstLayer &f, hipStream_t st,
                   bool front = false) {
    f = FirstLayer{ns.kernel[0], ns.bias[0], nullptr, nullptr};
    if (!ns.has_bn) return 0;
    TRY(colstats_segs(gate, dyn, 2, M, stats, stats + ns.in_dim, part, st));
    if (ns.units[0] > 4 || front) { f.bn_on_load = stats; return 0; }
    TRY(fold_with_stats(ns, stats, Wf, bf, st, true));
    f = FirstLayer{Wf, bf, nullptr, stats};
    return 0;
}

// ... and in the backward sweep: hidden activations are not on the tape - recomputed (the last layer's are, unless a Dropout layer follows it: `drop_any`)
int recompute_hidden(const gnn_mlp_t &ns, const gnn::Seg *segs, int n, int M, const float *stats, const float *Wf, const float *bf, float *const *hs,
                     const DropRun &drs, bool drop_any, hipStream_t st) {
    if (ns.n_layers == 1 && !drop_any) return 0;
    const bool folded = ns.has_bn && ns.units[0] <= 4 && !drop_at(&drs, 0);      // (first_layer_of)
    gnn_mlp_t head = ns; head.n_layers = drop_any ? ns.n_layers : ns.n_layers - 1;
    return forward_layers(head, segs, n, M, folded ? Wf : ns.kernel[0], folded ? bf : ns.bias[0], hs, nullptr, st, nullptr, (ns.has_bn && !folded) ? stats : nullptr,
                          folded ? stats : nullptr, &drs, true);
}

int transposes(NetCtx &x, hipStream_t st) {
    const gnn_mlp_t &m = *x.m;
    int fan_in = m.in_dim;
    for (int l = 0; l < m.n_layers; ++l) {
        gnn::k_transpose<<<std::min(cdiv((long)fan_in * m.units[l], 256), 1024), 256, 0, st>>>(m.kernel[l], fan_in, m.units[l], x.Wt[l]);
        LAUNCH_OK();
        fan_in = m.units[l];
    }
    return 0;
}

int zero_grads(const gnn_mlp_t &m, const gnn_mlp_grads_t &g, hipStream_t st) {
    if (m.has_bn) { HIP_OK(hipMemsetAsync(g.dgamma, 0, sizeof(float) * m.in_dim, st)); HIP_OK(hipMemsetAsync(g.dbeta, 0, sizeof(float) * m.in_dim, st)); }
    int fan_in = m.in_dim;
    for (int l = 0; l < m.n_layers; ++l) {
        HIP_OK(hipMemsetAsync(g.dkernel[l], 0, sizeof(float) * (size_t)fan_in * m.units[l], st));
        HIP_OK(hipMemsetAsync(g.dbias[l], 0, sizeof(float) * m.units[l], st));
        fan_in = m.units[l];
    }
    return 0;
}

int scale_grads(const gnn_mlp_t &m, const gnn_mlp_grads_t &g, float s, hipStream_t st) {
    auto sc = [&](float *p, size_t n) -> int {
        gnn::k_axpby<<<std::min(cdiv((long)n, 256), 1024), 256, 0, st>>>(s, p, 0.0f, nullptr, p, n);
        return hipGetLastError() == hipSuccess ? 0 : 1;
    };
    if (m.has_bn) { if (sc(g.dgamma, m.in_dim) || sc(g.dbeta, m.in_dim)) return fail("scale launch failed"); }
    int fan_in = m.in_dim;
    for (int l = 0; l < m.n_layers; ++l) {
        if (sc(g.dkernel[l], (size_t)fan_in * m.units[l]) || sc(g.dbias[l], m.units[l])) return fail("scale launch failed");
        fan_in = m.units[l];
    }
    return 0;
}

int check_grads(const gnn_mlp_t &m, const gnn_mlp_grads_t &g, const char *name) {
    if (m.has_bn && (!g.dgamma || !g.dbeta)) return fail("%s: dgamma / dbeta is NULL", name);
    for (int l = 0; l < m.n_layers; ++l) if (!g.dkernel[l] || !g.dbias[l]) return fail("%s: gradient buffer of layer %d is NULL", name, l);
    return 0;
}

// segments of the state network's input at iteration t (reference GNN.py:222-231): [state | nodes | agg | agg_nodes | agg_arcs]
int state_segs(const gnn_loop_args_t &a, const TrainPlan &p, int t, gnn::Seg *segs) {
    int n = 0, col = 0;
    const float *st_t = p.states + (size_t)t * p.N * p.ldS;
    segs[n++] = gnn::Seg{st_t, nullptr, p.ldS, p.S, col}; col += p.S;
    if (p.with_labels) { segs[n++] = gnn::Seg{a.nodes, nullptr, a.ld_nodes, p.L, col}; col += p.L; }
    segs[n++] = gnn::Seg{p.agg + (p.agg_taped ? (size_t)t * p.N * p.ldS : 0), nullptr, p.ldS, p.S, col}; col += p.S;
    if (p.with_labels) { segs[n++] = gnn::Seg{p.agg_nodes, nullptr, p.ld_agg_nodes, p.L, col}; col += p.L; }
    if (p.A > 0) { segs[n++] = gnn::Seg{p.agg_arcs, nullptr, p.ld_agg_arcs, p.A, col}; col += p.A; }
    return n;
}

// ---- launchers of the large-graph kernels -------------------------------------------------------------------------------------------
// the gathers with their eight source ids, then their eight rows requested together through buffer descriptors (kernels_general.hpp
// gather_sum8<.., BUF>): the arrays must fit 4 GiB windows; GNN_GATHER_BUF=0 keeps the pointer form (a dependent pair of round trips per arc)
inline bool gather_buf_enabled() { const char *e = getenv("GNN_GATHER_BUF"); return !(e && e[0] == '0'); }      // (read at every call: tests switch it inside one process)
inline bool gather_buf_ok(const gnn_csr_t &c, int ldx) {
    return gather_buf_enabled() && (size_t)c.n_src * (size_t)ldx * 4 < 0xFFFFFFF0ull && (size_t)c.nnz * 4 < 0xFFFFFFF0ull;
}
// `grid_out` != NULL: the partials stay in `part` ([*grid_out][2 S]) for the caller's own k_stats_finish (heterogeneous models: one for all types)
int launch_aggregate_stats(const int *gate, const gnn_csr_t &c, const float *X, int S, float *out, float *part, float *mean, float *var, const float *shift,
                           hipStream_t st, int *grid_out = nullptr) {
    const int lpr = S / 4, groups = 256 / lpr;
    const int grid = std::min(cdiv(c.n_dst, groups), BIG_AGG_BLOCKS);
#define AGGS_(L, W_, B_) gnn::k_aggregate_stats<L, W_, B_><<<grid, 256, 0, st>>>(gate, c.n_dst, c.rowptr, c.src, c.w, c.row_scale, X, S, out, S, part, shift)
#define AGGS(L) (buf ? (c.w ? AGGS_(L, true, true) : AGGS_(L, false, true)) : (c.w ? AGGS_(L, true, false) : AGGS_(L, false, false)))
    const bool buf = gather_buf_ok(c, S);
    switch (lpr) { case 4: AGGS(4); break; case 8: AGGS(8); break; default: AGGS(16); break; }
#undef AGGS
#undef AGGS_
    LAUNCH_OK();
    if (grid_out) { *grid_out = grid; return 0; }
    gnn::k_stats_finish<<<S, 256, 0, st>>>(gate, part, grid, S, 1.0f / (float)c.n_dst, mean, var, shift);
    LAUNCH_OK();
    return 0;
}

// column statistics of a row-major [M][F] matrix (F = 16 / 32 / 64) in one pass; columns [c0, c0 + width) go to mean / var [dst0 ..)
int rows_stats(const int *gate, const float *X, int ld, int F, int M, float *part, hipStream_t st, int *grid_out) {
    const int lpr = F / 4, groups = 256 / lpr;
    const int grid = std::max(1, std::min(cdiv(M, groups * 4), BIG_FWD_BLOCKS));
    switch (lpr) {
        case 4: gnn::k_rows_stats<4><<<grid, 256, 0, st>>>(gate, M, X, ld, part); break;
        case 8: gnn::k_rows_stats<8><<<grid, 256, 0, st>>>(gate, M, X, ld, part); break;
        default: gnn::k_rows_stats<16><<<grid, 256, 0, st>>>(gate, M, X, ld, part); break;
    }
    LAUNCH_OK();
    *grid_out = grid;
    return 0;
}

// the batch statistics of the constant columns from one pass over a packed constants line ([M][ld], moments around its row 0): segment
// s's width[s] columns (packed one behind the other) land at the BatchNorm columns wrow[s] .. of the template (mean | var, in_dim apart)
int line_stats(const float *line, int ld, int M, float *part, const int *width, const int *wrow, int n, float *tpl, int in_dim, hipStream_t st) {
    int grid = 0, c0 = 0;
    TRY(rows_stats(nullptr, line, ld, ld, M, part, st, &grid));
    for (int s = 0; s < n; ++s) {
        gnn::k_stats_finish<<<width[s], 256, 0, st>>>(nullptr, part + c0, grid, ld, 1.0f / (float)M, tpl + wrow[s], tpl + in_dim + wrow[s], line + c0);
        LAUNCH_OK();
        c0 += width[s];
    }
    return 0;
}

// ---- the large-graph step's dense kernels (kernels_train_big.hpp): one instance per shape, a shape without one is an error ----------------
// the first Dense of the state network (H == S)
// (kernel K's dynamic-LDS limit is raised at its first launch)
template <auto K>
int allow_lds(size_t lds, const char *name) {
    static bool done = false;
    if (!done && hipFuncSetAttribute((const void *)K, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return fail("%s: cannot raise the dynamic LDS limit", name);
    done = true;
    return 0;
}

template <int SQ, int ACT>
int launch_train_fwd_b6_sa(const gnn::TrainFwdArgs &fa, int grid, hipStream_t st) {
    const size_t lds = gnn::train_fwd_b6_lds<SQ>();
    TRY((allow_lds<gnn::k_train_fwd_b6<SQ, ACT>>(lds, "k_train_fwd_b6")));
    gnn::k_train_fwd_b6<SQ, ACT><<<grid, 64 * gnn::TB_WAVES, lds, st>>>(fa);
    return hipGetLastError() == hipSuccess ? 0 : fail("k_train_fwd_b6 launch failed");
}

template <int SQ>
int launch_train_fwd_b6_s(const gnn::TrainFwdArgs &fa, int grid, hipStream_t st) {
    switch (fa.act) {
        case GNN_ACT_LINEAR: return launch_train_fwd_b6_sa<SQ, GNN_ACT_LINEAR>(fa, grid, st);
        case GNN_ACT_RELU: return launch_train_fwd_b6_sa<SQ, GNN_ACT_RELU>(fa, grid, st);
        case GNN_ACT_SELU: return launch_train_fwd_b6_sa<SQ, GNN_ACT_SELU>(fa, grid, st);
        case GNN_ACT_TANH: return launch_train_fwd_b6_sa<SQ, GNN_ACT_TANH>(fa, grid, st);
        case GNN_ACT_SIGMOID: return launch_train_fwd_b6_sa<SQ, GNN_ACT_SIGMOID>(fa, grid, st);
        case GNN_ACT_ELU: return launch_train_fwd_b6_sa<SQ, GNN_ACT_ELU>(fa, grid, st);
        case GNN_ACT_SOFTPLUS: return launch_train_fwd_b6_sa<SQ, GNN_ACT_SOFTPLUS>(fa, grid, st);
        default: return fail("k_train_fwd_b6: no instance for activation %d", fa.act);      // (softmax state networks are not on the large-graph path)
    }
}

int launch_train_fwd(const gnn::TrainFwdArgs &fa, int S, hipStream_t st, int *grid_out) {
    if (fa.H != S) return fail("k_train_fwd_b6: %d units for state width %d", fa.H, S);
    const int n_tiles16 = (fa.M + 15) / 16;
    const int grid = std::max(1, std::min(std::min(device_cus(), BIG_FWD_BLOCKS), cdiv(n_tiles16, gnn::TB_WAVES)));     // one 8-wave workgroup per CU (192 registers)
    *grid_out = grid;
    switch (S) {
        case 16: return launch_train_fwd_b6_s<1>(fa, grid, st);
        case 32: return launch_train_fwd_b6_s<2>(fa, grid, st);
        case 64: return launch_train_fwd_b6_s<4>(fa, grid, st);
        default: return fail("k_train_fwd_b6: no instance for state width %d", S);
    }
}

// d loss / d [state | agg] from dZ (the LINEAR instance: the rows arrive with the activation's derivative applied)
template <int HQ>
int launch_train_bwd_dx_h(const gnn::TrainBwdArgs &ba, int grid, hipStream_t st) {
    const size_t lds = gnn::train_bwd_b6_lds<HQ>();
    TRY((allow_lds<gnn::k_train_bwd_dx_b6<HQ, GNN_ACT_LINEAR>>(lds, "k_train_bwd_dx_b6")));
    gnn::k_train_bwd_dx_b6<HQ, GNN_ACT_LINEAR><<<grid, 256, lds, st>>>(ba);
    return hipGetLastError() == hipSuccess ? 0 : fail("k_train_bwd_dx_b6 launch failed");
}

int launch_train_bwd_dx(const gnn::TrainBwdArgs &ba, int S, hipStream_t st) {
    if (ba.Y || ba.H != S || ba.S != S || ba.ldz != S) return fail("k_train_bwd_dx_b6: the dZ form of a %d-unit layer only", S);
    const int grid = std::max(1, std::min(2 * device_cus(), cdiv((ba.M + 15) / 16, 4)));       // 256-thread workgroups, two per CU
    switch (S) {
        case 16: return launch_train_bwd_dx_h<1>(ba, grid, st);
        case 32: return launch_train_bwd_dx_h<2>(ba, grid, st);
        case 64: return launch_train_bwd_dx_h<4>(ba, grid, st);
        default: return fail("k_train_bwd_dx_b6: no instance for state width %d", S);
    }
}

// the first layer's weight gradient P = X^T dZ, one partial per workgroup: k_train_wgrad_b6 (three-term splits, rows through an LDS ring;
// rows_per_wg a multiple of 64, one workgroup per CU) at S = 32 / 64, k_train_wgrad<1> at S = 16
template <int NB>
int launch_train_wgrad_b6_nb(const gnn::TrainWgradArgs &wa, int grid, hipStream_t st) {
    const size_t lds = gnn::train_wgrad_b6_lds<NB, GNN_ACT_LINEAR>();
    TRY((allow_lds<gnn::k_train_wgrad_b6<NB, GNN_ACT_LINEAR>>(lds, "k_train_wgrad_b6")));
    gnn::k_train_wgrad_b6<NB, GNN_ACT_LINEAR><<<grid, 256, lds, st>>>(wa);
    return hipGetLastError() == hipSuccess ? 0 : fail("k_train_wgrad_b6 launch failed");
}

// ... and the input gradient with it, from one pass over the rows (k_train_wgrad_dx_b6, S = 32 / 64)
template <int NB>
int launch_train_wgrad_dx_b6_nb(const gnn::TrainWgradArgs &wa, const gnn::TrainBwdArgs &ba, int grid, hipStream_t st) {
    const size_t lds = gnn::train_wgrad_dx_b6_lds<NB>();
    TRY((allow_lds<gnn::k_train_wgrad_dx_b6<NB>>(lds, "k_train_wgrad_dx_b6")));
    gnn::k_train_wgrad_dx_b6<NB><<<grid, 256, lds, st>>>(wa, ba);
    return hipGetLastError() == hipSuccess ? 0 : fail("k_train_wgrad_dx_b6 launch failed");
}

// the weight gradient of the dZ form; ba != NULL: the input gradient in the same pass
int launch_train_wgrad(const gnn::TrainWgradArgs &wa, const gnn::TrainBwdArgs *ba, int S, int grid, hipStream_t st) {
    if (wa.Y || wa.act != GNN_ACT_LINEAR) return fail("k_train_wgrad: the dZ form only");
    if (ba) {
        // With BatchNormalization the input gradient needs m1 / m2 - column moments of dZ W^T that k_first_layer_param_grads derives from THIS
        // iteration's finished P and q - so the two products cannot share a pass there (the kernel itself takes them as given: scripts/micro/
        // rowgemm_check.hip checks it bit for bit against the two kernels on arbitrary m1 / m2).  Without it nothing global stands between them.
        if (ba->gamma || ba->Y || ba->H != S || ba->S != S || ba->ldz != S || ba->ld_state != S || ba->ld_agg != S || ba->M != wa.M || ba->dZ != wa.G ||
            ba->agg != wa.agg || (size_t)wa.rows_per_wg * (size_t)ba->ld_dx * 4 >= 0xFFFFFFF0ull)
            return fail("k_train_wgrad_dx_b6: not for these arguments");
        if (S == 64) return launch_train_wgrad_dx_b6_nb<2>(wa, *ba, grid, st);
        if (S == 32) return launch_train_wgrad_dx_b6_nb<1>(wa, *ba, grid, st);
        return fail("k_train_wgrad_dx_b6: no instance for state width %d", S);
    }
    switch (S) {
        case 16: gnn::k_train_wgrad<1><<<grid, 256, 0, st>>>(wa); LAUNCH_OK(); return 0;
        case 32: return launch_train_wgrad_b6_nb<1>(wa, grid, st);
        case 64: return launch_train_wgrad_b6_nb<2>(wa, grid, st);
        default: return fail("k_train_wgrad: no instance for state width %d", S);
    }
}

// G_{t-1} -> dZ_{t-1} in the transposed aggregate's epilogue (kernels_train_big.hpp: k_aggregate_dz); false: no instance for this shape
template <int LPR, bool HAS_W>
bool launch_aggregate_dz_lw(const gnn_csr_t &c, const float *Xa, int ldx, float *out, int ldo, const float *addend, int ld_add, const gnn::AggDzArgs &z, int act,
                            int grid, hipStream_t st) {
    const bool buf = gather_buf_ok(c, ldx);
#define AGGDZ_(A_, B_) gnn::k_aggregate_dz<LPR, HAS_W, A_, B_><<<grid, 256, 0, st>>>(c.n_dst, c.rowptr, c.src, c.w, c.row_scale, Xa, ldx, out, ldo, addend, ld_add, z)
#define AGGDZ(A_) do { if (buf) AGGDZ_(A_, true); else AGGDZ_(A_, false); } while (0)
    switch (act) {
        case GNN_ACT_LINEAR: AGGDZ(GNN_ACT_LINEAR); return true;
        case GNN_ACT_RELU: AGGDZ(GNN_ACT_RELU); return true;
        case GNN_ACT_SELU: AGGDZ(GNN_ACT_SELU); return true;
        case GNN_ACT_TANH: AGGDZ(GNN_ACT_TANH); return true;
        case GNN_ACT_SIGMOID: AGGDZ(GNN_ACT_SIGMOID); return true;
        case GNN_ACT_ELU: AGGDZ(GNN_ACT_ELU); return true;
        case GNN_ACT_SOFTPLUS: AGGDZ(GNN_ACT_SOFTPLUS); return true;
        default: return false;
    }
#undef AGGDZ
#undef AGGDZ_
}
bool launch_aggregate_dz(const gnn_csr_t &c, const float *Xa, int ldx, float *out, int ldo, const float *addend, int ld_add, const gnn::AggDzArgs &z, int act, int S,
                         hipStream_t st) {
    const int lpr = S / 4, groups = 256 / lpr, grid = std::min(cdiv(c.n_dst, groups), 256 * 16);
    switch (lpr) {
        case 4: return c.w ? launch_aggregate_dz_lw<4, true>(c, Xa, ldx, out, ldo, addend, ld_add, z, act, grid, st) : launch_aggregate_dz_lw<4, false>(c, Xa, ldx, out, ldo, addend, ld_add, z, act, grid, st);
        case 8: return c.w ? launch_aggregate_dz_lw<8, true>(c, Xa, ldx, out, ldo, addend, ld_add, z, act, grid, st) : launch_aggregate_dz_lw<8, false>(c, Xa, ldx, out, ldo, addend, ld_add, z, act, grid, st);
        case 16: return c.w ? launch_aggregate_dz_lw<16, true>(c, Xa, ldx, out, ldo, addend, ld_add, z, act, grid, st) : launch_aggregate_dz_lw<16, false>(c, Xa, ldx, out, ldo, addend, ld_add, z, act, grid, st);
        default: return false;
    }
}

gnn::ConstSegs const_segs_of(const gnn_loop_args_t &a, const TrainPlan &p) {
    gnn::ConstSegs cs{};
    gnn::Seg segs[GNN_MAX_SEGS];
    const int n0 = state_segs(a, p, 0, segs);
    for (int s = 0; s < n0; ++s)
        if (segs[s].ptr != p.states && segs[s].ptr != p.agg) { cs.ptr[cs.n] = segs[s].ptr; cs.ld[cs.n] = segs[s].ld; cs.width[cs.n] = segs[s].width; cs.wrow[cs.n] = segs[s].wrow; ++cs.n; }
    return cs;
}

template <typename Kern, typename Args, typename... Extra>
int launch_persistent(Kern kern, const Args &args, const gnn::TileTab &tt, int n_wg, size_t lds, hipStream_t st, const Extra &... extra) {
    lds = std::max(lds, gnn::TS_LDS);
    static std::vector<const void *> allowed;          // kernels whose dynamic-LDS limit has been raised
    static std::mutex allowed_mutex;                   // (callers may run steps of different models on different host threads)
    const void *fn = reinterpret_cast<const void *>(kern);
    {
        std::lock_guard<std::mutex> lock(allowed_mutex);
        if (std::find(allowed.begin(), allowed.end(), fn) == allowed.end()) {
            HIP_OK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));      // (the same for every launch of one kernel)
            allowed.push_back(fn);
        }
    }
    // every workgroup waits for the others at the grid barriers: the grid must fit the device (n_wg <= CUs by the plan; this asks the
    // runtime about THIS kernel's registers / LDS)
    if (!gnn::persistent_fits(fn, gnn::TS_NT, lds, n_wg, device_cus())) return not_resident("persistent training kernel: %d workgroups cannot be resident at once", n_wg);
    kern<<<n_wg, gnn::TS_NT, lds, st>>>(args, tt, extra...);
    LAUNCH_OK();
    return 0;
}

// `yt` (heterogeneous models: tiles cut at TYPE boundaries, arcs cross them: the general form with a tile table); yt == NULL: homogeneous -
// a tile table then means tiles cut at GRAPH boundaries that no arc leaves (the LOCAL form)
template <int SQ>
int launch_train_small_fwd_sq(const gnn::TrainSmallFwd &fa, const gnn::TileTab &tt, int n_wg, bool has_w, hipStream_t st, const gnn::TypeTab *yt = nullptr) {
    const size_t lds = gnn::train_small_fwd_lds<SQ>();
    static const gnn::TypeTab none{};
    const gnn::TypeTab &y = yt ? *yt : none;
    if (tt.n > 0 && !yt) return has_w ? launch_persistent(&gnn::k_train_small_fwd<SQ, true, true>, fa, tt, n_wg, lds, st, y)
                                      : launch_persistent(&gnn::k_train_small_fwd<SQ, false, true>, fa, tt, n_wg, lds, st, y);
    return has_w ? launch_persistent(&gnn::k_train_small_fwd<SQ, true, false>, fa, tt, n_wg, lds, st, y)
                 : launch_persistent(&gnn::k_train_small_fwd<SQ, false, false>, fa, tt, n_wg, lds, st, y);
}

template <int SQ>
int launch_train_small_bwd_sq(const gnn::TrainSmallBwd &ba, const gnn::TileTab &tt, int n_wg, bool has_w, hipStream_t st, const gnn::TypeTab *yt = nullptr,
                              const gnn::TypeConsts *yc = nullptr) {
    const bool local = tt.n > 0 && !yt;
    const size_t lds = gnn::train_small_bwd_lds<SQ>(local);
    static const gnn::TypeTab none{};
    static const gnn::TypeConsts nonec{};
    const gnn::TypeTab &y = yt ? *yt : none;
    const gnn::TypeConsts &c = yc ? *yc : nonec;
    if (ba.dz_out || ba.g0_out) {      // label gradients wanted (homogeneous models): the instantiations with the two extra stores
        if (local) return has_w ? launch_persistent(&gnn::k_train_small_bwd<SQ, true, true, true>, ba, tt, n_wg, lds, st, y, c)
                                : launch_persistent(&gnn::k_train_small_bwd<SQ, false, true, true>, ba, tt, n_wg, lds, st, y, c);
        return has_w ? launch_persistent(&gnn::k_train_small_bwd<SQ, true, false, true>, ba, tt, n_wg, lds, st, y, c)
                     : launch_persistent(&gnn::k_train_small_bwd<SQ, false, false, true>, ba, tt, n_wg, lds, st, y, c);
    }
    if (local) return has_w ? launch_persistent(&gnn::k_train_small_bwd<SQ, true, true>, ba, tt, n_wg, lds, st, y, c)
                            : launch_persistent(&gnn::k_train_small_bwd<SQ, false, true>, ba, tt, n_wg, lds, st, y, c);
    return has_w ? launch_persistent(&gnn::k_train_small_bwd<SQ, true, false>, ba, tt, n_wg, lds, st, y, c)
                 : launch_persistent(&gnn::k_train_small_bwd<SQ, false, false>, ba, tt, n_wg, lds, st, y, c);
}

// the hidden-layer form of both launches (homogeneous models; fa.W2 / ba.W2 set): LOCAL with a tile table, both HAS_W forms, LAB as above
template <int SQ>
int launch_train_small_fwd_hid_sq(const gnn::TrainSmallFwdH &fa, const gnn::TileTab &tt, int n_wg, bool has_w, hipStream_t st) {
    const size_t lds = gnn::train_small_fwd_lds<SQ, true>();
    static const gnn::TypeTab y{};
    if (tt.n > 0) return has_w ? launch_persistent(&gnn::k_train_small_fwd<SQ, true, true, true>, fa, tt, n_wg, lds, st, y)
                               : launch_persistent(&gnn::k_train_small_fwd<SQ, false, true, true>, fa, tt, n_wg, lds, st, y);
    return has_w ? launch_persistent(&gnn::k_train_small_fwd<SQ, true, false, true>, fa, tt, n_wg, lds, st, y)
                 : launch_persistent(&gnn::k_train_small_fwd<SQ, false, false, true>, fa, tt, n_wg, lds, st, y);
}

template <int SQ>
int launch_train_small_bwd_hid_sq(const gnn::TrainSmallBwdH &ba, const gnn::TileTab &tt, int n_wg, bool has_w, hipStream_t st) {
    const bool local = tt.n > 0;
    const size_t lds = gnn::train_small_bwd_lds<SQ>(local, true);
    static const gnn::TypeTab y{};
    static const gnn::TypeConsts c{};
    if (ba.dz_out || ba.g0_out) {
        if (local) return has_w ? launch_persistent(&gnn::k_train_small_bwd<SQ, true, true, true, true>, ba, tt, n_wg, lds, st, y, c)
                                : launch_persistent(&gnn::k_train_small_bwd<SQ, false, true, true, true>, ba, tt, n_wg, lds, st, y, c);
        return has_w ? launch_persistent(&gnn::k_train_small_bwd<SQ, true, false, true, true>, ba, tt, n_wg, lds, st, y, c)
                     : launch_persistent(&gnn::k_train_small_bwd<SQ, false, false, true, true>, ba, tt, n_wg, lds, st, y, c);
    }
    if (local) return has_w ? launch_persistent(&gnn::k_train_small_bwd<SQ, true, true, false, true>, ba, tt, n_wg, lds, st, y, c)
                            : launch_persistent(&gnn::k_train_small_bwd<SQ, false, true, false, true>, ba, tt, n_wg, lds, st, y, c);
    return has_w ? launch_persistent(&gnn::k_train_small_bwd<SQ, true, false, false, true>, ba, tt, n_wg, lds, st, y, c)
                 : launch_persistent(&gnn::k_train_small_bwd<SQ, false, false, false, true>, ba, tt, n_wg, lds, st, y, c);
}

// the Dropout form of both launches (homogeneous models; `dr`: the layers' scalars and the un-dropped tape), one-layer (Base = TrainSmallFwd /
// TrainSmallBwd) or hidden-layer (Base = ..H): the kernel's argument block is the base block with the Dropout arguments behind it
template <int SQ, bool HID, typename Base>
int launch_train_small_fwd_drop_sq(const Base &fa, const gnn::SmallDrop &dr, const gnn::TileTab &tt, int n_wg, bool has_w, hipStream_t st) {
    const size_t lds = gnn::train_small_fwd_lds<SQ, HID>();
    static const gnn::TypeTab y{};
    gnn::TrainSmallDrop<Base> d{};
    static_cast<Base &>(d) = fa; d.dr = dr;
    if (tt.n > 0) return has_w ? launch_persistent(&gnn::k_train_small_fwd<SQ, true, true, HID, true>, d, tt, n_wg, lds, st, y)
                               : launch_persistent(&gnn::k_train_small_fwd<SQ, false, true, HID, true>, d, tt, n_wg, lds, st, y);
    return has_w ? launch_persistent(&gnn::k_train_small_fwd<SQ, true, false, HID, true>, d, tt, n_wg, lds, st, y)
                 : launch_persistent(&gnn::k_train_small_fwd<SQ, false, false, HID, true>, d, tt, n_wg, lds, st, y);
}

template <int SQ, bool HID, typename Base>
int launch_train_small_bwd_drop_sq(const Base &ba, const gnn::SmallDrop &dr, const gnn::TileTab &tt, int n_wg, bool has_w, hipStream_t st) {
    const bool local = tt.n > 0;
    const size_t lds = gnn::train_small_bwd_lds<SQ>(local, HID);
    static const gnn::TypeTab y{};
    static const gnn::TypeConsts c{};
    gnn::TrainSmallDrop<Base> d{};
    static_cast<Base &>(d) = ba; d.dr = dr;
    if (ba.dz_out || ba.g0_out) {
        if (local) return has_w ? launch_persistent(&gnn::k_train_small_bwd<SQ, true, true, true, HID, true>, d, tt, n_wg, lds, st, y, c)
                                : launch_persistent(&gnn::k_train_small_bwd<SQ, false, true, true, HID, true>, d, tt, n_wg, lds, st, y, c);
        return has_w ? launch_persistent(&gnn::k_train_small_bwd<SQ, true, false, true, HID, true>, d, tt, n_wg, lds, st, y, c)
                     : launch_persistent(&gnn::k_train_small_bwd<SQ, false, false, true, HID, true>, d, tt, n_wg, lds, st, y, c);
    }
    if (local) return has_w ? launch_persistent(&gnn::k_train_small_bwd<SQ, true, true, false, HID, true>, d, tt, n_wg, lds, st, y, c)
                            : launch_persistent(&gnn::k_train_small_bwd<SQ, false, true, false, HID, true>, d, tt, n_wg, lds, st, y, c);
    return has_w ? launch_persistent(&gnn::k_train_small_bwd<SQ, true, false, false, HID, true>, d, tt, n_wg, lds, st, y, c)
                 : launch_persistent(&gnn::k_train_small_bwd<SQ, false, false, false, HID, true>, d, tt, n_wg, lds, st, y, c);
}

// the per-workgroup partials [grid][K H + H] of a first layer's P = X^T dZ | q summed into x.P / x.q, then its parameter gradients (and the
// BatchNorm input-gradient moments m1 / m2) over M rows; `centred`: the rows arrived centred (P is P - mean q^T)
int first_layer_grads(const NetCtx &x, const float *part, int grid, int M, const float *stats, bool accumulate, bool centred, hipStream_t st) {
    const gnn_mlp_t &m = *x.m;
    const int K = m.in_dim, H = m.units[0], n = K * H + H;
    const bool bn = m.has_bn != 0;
    gnn::k_reduce_partials<<<cdiv(n, 64), 256, 0, st>>>(part, grid, n, x.P, 0, 1.0f, K * H, x.q);
    LAUNCH_OK();
    gnn::k_first_layer_param_grads<<<K, 64, 0, st>>>(x.P, x.q, m.kernel[0], K, H, bn ? m.bn_gamma : nullptr, m.bn_beta, stats, stats ? stats + K : nullptr, m.bn_eps,
                                                     1.0f / (float)M, x.g->dkernel[0], x.g->dbias[0], x.g->dgamma, x.g->dbeta, bn ? x.m1 : nullptr, bn ? x.m2 : nullptr,
                                                     accumulate ? 1 : 0, 1, centred ? 1 : 0);
    LAUNCH_OK();
    return 0;
}

// Back-propagation through a thin output head over every node of a large graph (kernels_train_big.hpp: k_head_wgrad / k_head_dx): the
// head's parameter gradients, and d loss / d state_k written straight into the state gradient.  G = d loss / d head output [M x T].
// `labels` / `L`: the label columns behind the state in the head's input (NULL / 0: the state alone - composite models, state_0 = labels)
template <int T>
int head_backward_t(const StepPlan &p, const gnn_loop_args_t &a, const float *labels, int L, const float *state_k, int ld_state, const float *out_nodes, float *G,
                    const float *stats, hipStream_t st, int dz_act) {
    const gnn_mlp_t &m = a.net_output;
    TRY(act_grad_inplace(G, p.T, out_nodes, p.T, p.M, p.T, m.activation[0], st));
    gnn::HeadArgs h{};
    h.M = p.M; h.S = p.S; h.L = L; h.T = T;
    h.state = state_k; h.ld_state = ld_state; h.labels = labels; h.ld_labels = a.ld_nodes;
    h.dZ = G; h.ldz = p.T;
    const int grid = std::min(BIG_HEAD_BLOCKS, cdiv(p.M, 256));
    h.rows_per_wg = cdiv(p.M, grid);
    h.part = p.part_h;
    gnn::k_head_wgrad<T><<<grid, 256, 0, st>>>(h);
    LAUNCH_OK();
    TRY(first_layer_grads(p.co, p.part_h, grid, p.M, stats, false, false, st));
    h.W = m.kernel[0];
    if (m.has_bn) { h.gamma = m.bn_gamma; h.mean = stats; h.var = stats + m.in_dim; h.m1 = p.co.m1; h.m2 = p.co.m2; h.eps = m.bn_eps; }
    h.dx = p.G_state; h.ld_dx = p.S; h.dz_act = dz_act;
    const int lpr = p.S / 4 <= 4 ? 4 : p.S / 4 <= 8 ? 8 : 16;
    gnn::k_head_dx<T><<<std::min(cdiv(p.M, 256 / lpr), 256 * 16), 256, 0, st>>>(h);
    LAUNCH_OK();
    return 0;
}

// `dz_act` >= 0: the state gradient leaves as the loop's last dZ (HeadArgs::dz_act)
int head_backward(const StepPlan &p, const gnn_loop_args_t &a, const float *labels, int L, const float *state_k, int ld_state, const float *out_nodes, float *G,
                  const float *stats, hipStream_t st, int dz_act = -1) {
    const auto run = p.T == 1 ? head_backward_t<1> : p.T == 2 ? head_backward_t<2> : p.T == 3 ? head_backward_t<3> : head_backward_t<4>;
    return run(p, a, labels, L, state_k, ld_state, out_nodes, G, stats, st, dz_act);
}

// the caller's tiles (HOST array), checked: ascending, <= 64 nodes each, covering [0, N)
int tile_table(const gnn_train_args_t &ta, const TrainPlan &p, gnn::TileTab &tt) {
    memset(&tt, 0, sizeof(tt));
    if (!p.tiled) return 0;
    tt.n = ta.n_tiles;
    for (int b = 0; b <= tt.n; ++b) tt.begin[b] = ta.tile_node_begin[b];
    if (tt.begin[0] != 0 || tt.begin[tt.n] != p.N) return fail("tile_node_begin must run from 0 to n_nodes");
    for (int b = 0; b < tt.n; ++b)
        if (tt.begin[b + 1] <= tt.begin[b] || tt.begin[b + 1] - tt.begin[b] > 64) return fail("tile %d has %d nodes (1 .. 64 allowed)", b, tt.begin[b + 1] - tt.begin[b]);
    return 0;
}

// ==== the phases both model kinds share: train_step_impl() below and train_step_composite() (train_composite.hpp) call these ============

// the operands of a step, in front of its first launch (`own_loss`: the call computes a loss; `want_grads`: it writes gradients); where the
// two kinds word or order a check differently, both forms are kept
int check_step_args(const gnn_train_args_t &ta, const StepPlan &p, bool own_loss, bool want_grads) {
    const gnn_loop_args_t &a = ta.loop;
    const bool comp = a.composite != 0;
    TRY(check_csr(a.adjacency, "adjacency", p.N, p.N));
    TRY(check_csr(a.arcnode, "arcnode", p.N, p.E));
    if (!ta.forward_only) TRY(check_csr(ta.adjacency_by_source, "adjacency_by_source", p.N, p.N));
    for (int t = 0; t < a.n_types && comp; ++t) {
        TRY(check_csr(a.composite_adjacency[t], "composite_adjacency", p.N, p.N));
        if (want_grads) TRY(check_grads(a.net_state[t], ta.grad_state_types[t], "grad_state_types"));
    }
    if (comp) { if (!a.nodes || !a.type_nodes) return fail("nodes / type_nodes is NULL"); }
    else if (!a.nodes || (p.E > 0 && p.A > 0 && !a.arc_labels)) return fail("nodes / arc_labels is NULL");
    if (a.state_dim > 0 && !a.state0) return fail("state0 is required when state_dim > 0");
    if (p.M > 0 && !a.out_index) return fail("out_index is NULL");
    if (comp && p.E > 0 && p.A > 0 && !a.arc_labels) return fail("arc_labels is NULL");
    if (a.focus == GNN_FOCUS_ARC && p.E > 0 && (!a.arc_src || !a.arc_dst)) return fail("arc focus needs arc_src / arc_dst");
    if (p.pooled) {
        if (a.nodegraph.n_src != p.M && comp) return fail("graph focus: NodeGraph has %d rows but %d nodes pass the mask", a.nodegraph.n_src, p.M);
        if (a.nodegraph.n_src != p.M) return fail("graph focus: every node must pass the mask");
        TRY(check_csr(a.nodegraph, "nodegraph", p.G, p.M));
        if (!ta.forward_only) TRY(check_csr(ta.nodegraph_by_source, "nodegraph_by_source", p.M, p.G));
    }
    if (comp) { if (own_loss && p.R > 0 && !ta.targets) return fail("targets is NULL"); }
    else if (p.R < 1 || (own_loss && !ta.targets)) return fail("gnn_train_step needs at least one target row");
    if (own_loss && (ta.loss_kind < 0 || ta.loss_kind > 3)) return fail("unknown loss kind %d", ta.loss_kind);
    if (((!comp || p.R > 0) && !ta.y_pred) || (own_loss && !ta.loss) || !ta.k_host || !ta.state) return fail("y_pred / loss / k_host / state is NULL");
    if (want_grads && !comp) TRY(check_grads(a.net_state[0], ta.grad_state, "grad_state"));
    if (want_grads) TRY(check_grads(a.net_output, ta.grad_output, "grad_output"));
    return 0;
}

// the common fields of the persistent forward launch and the instance for the padded width (`fa`: zeroed, the caller's own fields set;
// p.hid_small: `fa` / `ba` below ARE the hidden-layer blocks TrainSmallFwdH / TrainSmallBwdH - forward_small / backward_small make them)
// p.drop_small: `dr` carries the Dropout form's arguments (small_drop_args below)
int launch_train_small_fwd(gnn::TrainSmallFwd &fa, const gnn_train_args_t &ta, const StepPlan &p, const gnn::TileTab &tiles, const gnn::TypeTab *yt, hipStream_t st,
                           const gnn::SmallDrop *dr = nullptr) {
    const gnn_csr_t &ad = ta.loop.adjacency;
    fa.N = p.N; fa.S = p.SPs; fa.Sw = p.S; fa.K = p.K;
    fa.rowptr = ad.rowptr; fa.src = ad.src; fa.w = ad.w; fa.row_scale = ad.row_scale;
    fa.states = p.states; fa.agg = p.agg;
    fa.Cc = p.sm_cc; fa.thr = ta.loop.state_threshold; fa.flag0 = p.flags;
    fa.bar = p.sm_bar; fa.part = p.sm_part; fa.k_out = p.k_dev; fa.wait_ticks = gnn::wait_ticks();
    if (const char *e = getenv("GNN_DEBUG_FAIL_FWD")) { if (e[0] == '1') fa.wait_ticks = 0; }      // (test hook: every barrier wait of THIS forward launch expires at once)
    if (p.drop_small) {      // (the rule: padded widths 16 / 32)
        if (!dr) return fail("persistent forward launch: the Dropout form without its arguments");
        if (p.hid_small) {
            const auto &fh = static_cast<const gnn::TrainSmallFwdH &>(fa);
            return p.SPs == 16 ? launch_train_small_fwd_drop_sq<1, true>(fh, *dr, tiles, p.n_wg, ad.w != nullptr, st)
                               : launch_train_small_fwd_drop_sq<2, true>(fh, *dr, tiles, p.n_wg, ad.w != nullptr, st);
        }
        return p.SPs == 16 ? launch_train_small_fwd_drop_sq<1, false>(fa, *dr, tiles, p.n_wg, ad.w != nullptr, st)
                           : launch_train_small_fwd_drop_sq<2, false>(fa, *dr, tiles, p.n_wg, ad.w != nullptr, st);
    }
    if (p.hid_small) {
        const auto hid = p.SPs == 16 ? launch_train_small_fwd_hid_sq<1> : launch_train_small_fwd_hid_sq<2>;      // (the rule: padded widths 16 / 32)
        return hid(static_cast<const gnn::TrainSmallFwdH &>(fa), tiles, p.n_wg, ad.w != nullptr, st);
    }
    const auto launch = p.SPs == 16 ? launch_train_small_fwd_sq<1> : p.SPs == 32 ? launch_train_small_fwd_sq<2> : launch_train_small_fwd_sq<4>;
    return launch(fa, tiles, p.n_wg, ad.w != nullptr, st, yt);
}

// ... and of the persistent backward launch: the k iterations of back-propagation; every workgroup leaves its share of the kernel gradient
int launch_train_small_bwd(gnn::TrainSmallBwd &ba, const gnn_train_args_t &ta, const StepPlan &p, int k, const gnn::TileTab &tiles, const gnn::TypeTab *yt,
                           const gnn::TypeConsts *yc, hipStream_t st, const gnn::SmallDrop *dr = nullptr) {
    const gnn_csr_t &ad = ta.loop.adjacency, &cs_ = ta.adjacency_by_source;
    const bool unit_w = !ad.w;       // entries depend on the destination only: scale the agg-half once per row, walk unit weights
    ba.N = p.N; ba.S = p.SPs; ba.Sw = p.S; ba.k = k;
    ba.rowptr_s = cs_.rowptr; ba.src_s = cs_.src; ba.w_s = unit_w ? nullptr : cs_.w; ba.row_scale_s = unit_w ? nullptr : cs_.row_scale;
    ba.row_scale = unit_w ? ad.row_scale : nullptr;
    ba.states = p.states; ba.agg = p.agg;
    ba.G0 = p.G_state; ba.bar = p.sm_bar + 2; ba.part = p.sm_part;
    ba.inv_n = 1.0f / (float)p.N; ba.err = p.k_dev; ba.wait_ticks = gnn::wait_ticks();
    if (const char *e = getenv("GNN_DEBUG_FAIL_BWD")) { if (e[0] == '1') ba.wait_ticks = 0; }      // (test hook: every barrier wait of THIS launch expires at once)
    if (p.drop_small) {
        if (!dr) return fail("persistent backward launch: the Dropout form without its arguments");
        if (p.hid_small) {
            const auto &bh = static_cast<const gnn::TrainSmallBwdH &>(ba);
            return p.SPs == 16 ? launch_train_small_bwd_drop_sq<1, true>(bh, *dr, tiles, p.n_wg, ba.w_s != nullptr, st)
                               : launch_train_small_bwd_drop_sq<2, true>(bh, *dr, tiles, p.n_wg, ba.w_s != nullptr, st);
        }
        return p.SPs == 16 ? launch_train_small_bwd_drop_sq<1, false>(ba, *dr, tiles, p.n_wg, ba.w_s != nullptr, st)
                           : launch_train_small_bwd_drop_sq<2, false>(ba, *dr, tiles, p.n_wg, ba.w_s != nullptr, st);
    }
    if (p.hid_small) {
        const auto hid = p.SPs == 16 ? launch_train_small_bwd_hid_sq<1> : launch_train_small_bwd_hid_sq<2>;
        return hid(static_cast<const gnn::TrainSmallBwdH &>(ba), tiles, p.n_wg, ba.w_s != nullptr, st);
    }
    const auto launch = p.SPs == 16 ? launch_train_small_bwd_sq<1> : p.SPs == 32 ? launch_train_small_bwd_sq<2> : launch_train_small_bwd_sq<4>;
    return launch(ba, tiles, p.n_wg, ba.w_s != nullptr, st, yt, yc);
}

// out = addend + Adj . X over F columns, arcs walked by source (the scalar walk: any width, any alignment)
int launch_aggregate_add(const gnn_csr_t &c, const float *X, int ldx, int F, const float *addend, int ld_add, float *out, int ldo, hipStream_t st) {
    int G = 4;
    while (G < F && G < 64) G <<= 1;
    const int groups = 256 / G, grid = std::min(cdiv(c.n_dst, groups), 256 * 16);
    const auto kern = G == 4 ? gnn::k_aggregate_add<4> : G == 8 ? gnn::k_aggregate_add<8> : G == 16 ? gnn::k_aggregate_add<16> : G == 32 ? gnn::k_aggregate_add<32>
                                                                                                                                      : gnn::k_aggregate_add<64>;
    kern<<<grid, 256, 0, st>>>(c.n_dst, c.rowptr, c.src, c.w, c.row_scale, X, ldx, F, addend, ld_add, out, ldo);
    LAUNCH_OK();
    return 0;
}

// the last launches of a setup: the thin-head kernels treat output row m as node m - out_index must BE the identity (read_k) -, iteration 0's gate
int finish_setup(const gnn_train_args_t &ta, const StepPlan &p, hipStream_t st) {
    if (p.head_fast) {
        gnn::k_not_identity<<<std::min(cdiv(p.M, 256), 1024), 256, 0, st>>>(ta.loop.out_index, p.M, p.k_dev + 2);
        LAUNCH_OK();
    }
    return launch_converge(nullptr, p.states, nullptr, p.N, p.S, p.ldS, 0, ta.loop.state_threshold, p.flags, nullptr, 0.f, st);
}

// k, read with the step's one host synchronisation, and what the device reported next to it: k_dev[1] the persistent kernels' error word,
// k_dev[2] != 0 a permuted / repeated out_index of length n_nodes - the general head then (gathers, scatter-add)
int read_k(const gnn_train_args_t &ta, StepPlan &p, int *k_out, hipStream_t st) {
    float k_f2[3] = {0.0f, 0.0f, 0.0f};
    HIP_OK(hipMemcpyAsync(k_f2, p.k_dev, 3 * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));                                  // the one host synchronisation of the step
    const int k = (int)k_f2[0];
    *ta.k_host = *k_out = k;
    if (k_f2[1] == 1.0f) return fail("tile_node_begin: an arc of `adjacency` leaves its tile");
    if (k_f2[1] != 0.0f) return not_resident("a workgroup of the persistent training kernel never arrived at a grid barrier (not resident?)");
    if (k < 0 || k > p.K) return fail("iteration count %d out of range", k);
    if (k_f2[2] != 0.0f) p.head_fast = false;
    return 0;
}

// The moving averages of BatchNormalization (one update per executed call) run right behind the forward on the general and the large-
// graph path.  On the persistent path they wait until the backward launch has passed its grid barriers and are gated by the step's
// validity word - a step whose backward failed changes nothing - or, for a forward alone, run ungated at its end (moving_deferred()).
// bn_moving(): `steps` updates of network m's from the slots of `stats`.  Each kind has its moving_state(ta, plan, k, gate, st).
int bn_moving(const gnn_mlp_t &m, const float *stats, int steps, float momentum, const int *gate, hipStream_t st) {
    if (!m.has_bn || steps <= 0) return 0;
    gnn::k_bn_moving_multi<<<cdiv(m.in_dim, 256), 256, 0, st>>>(stats, 2 * m.in_dim, steps, m.in_dim, const_cast<float *>(m.bn_mean), const_cast<float *>(m.bn_var), momentum, gate);
    LAUNCH_OK();
    return 0;
}
int moving_output(const gnn_train_args_t &ta, const StepPlan &p, const int *gate, hipStream_t st) {
    return bn_moving(*p.co.m, p.stats_o, p.M > 0 ? 1 : 0, ta.bn_momentum, gate, st);
}

template <typename Plan>
int moving_deferred(const gnn_train_args_t &ta, const Plan &p, int k, const int *gate, hipStream_t st) {
    if (p.path != TrainPath::small) return 0;
    TRY(moving_state(ta, p, k, gate, st));
    return moving_output(ta, p, gate, st);
}

// ---- the output network's call of a step: its input [state_k | labels] of the masked nodes, or of both end nodes of the masked arcs
// followed by the arc labels (composite models: the state alone), its layer buffers and its Dropout run - forward and backward read the same
struct HeadRun {
    gnn::Seg segs[GNN_MAX_SEGS]; int nseg;
    int n_state; int state_off[2]; const int *state_idx[2];       // the state segments: column offset inside the input, row list
    const float *state_k; int ld_state;
    DropRun drop;
    float *hs[GNN_MAX_LAYERS], *out_nodes;
};

// `L` label columns of `a.nodes` behind every state segment (0: none); `endpoints`: launch k_arc_endpoints (phase 2 finds them on the tape)
int head_segments(const gnn_train_args_t &ta, const StepPlan &p, const float *state_k, int ld_state, int L, bool endpoints, HeadRun &h, hipStream_t st) {
    const gnn_loop_args_t &a = ta.loop;
    const gnn_mlp_t &no = a.net_output;
    memset(&h, 0, sizeof(h));
    h.state_k = state_k; h.ld_state = ld_state;
    int ocol = 0;
    if (p.M > 0 && a.focus == GNN_FOCUS_ARC) {
        if (endpoints) {
            k_arc_endpoints<<<cdiv(p.M, 256), 256, 0, st>>>(a.out_index, a.arc_src, a.arc_dst, p.M, p.isrc, p.idst);
            LAUNCH_OK();
        }
        const int *ends[2] = {p.isrc, p.idst};
        for (int e = 0; e < 2; ++e) {
            h.state_off[h.n_state] = ocol; h.state_idx[h.n_state++] = ends[e];
            h.segs[h.nseg++] = gnn::Seg{state_k, ends[e], ld_state, p.S, ocol}; ocol += p.S;
            if (L > 0) { h.segs[h.nseg++] = gnn::Seg{a.nodes, ends[e], a.ld_nodes, L, ocol}; ocol += L; }
        }
        if (p.A > 0) { h.segs[h.nseg++] = gnn::Seg{a.arc_labels, a.out_index, a.ld_arcs, p.A, ocol}; ocol += p.A; }
    } else if (p.M > 0) {
        h.state_off[0] = 0; h.state_idx[0] = a.out_index; h.n_state = 1;
        h.segs[h.nseg++] = gnn::Seg{state_k, a.out_index, ld_state, p.S, ocol}; ocol += p.S;
        if (L > 0) { h.segs[h.nseg++] = gnn::Seg{a.nodes, a.out_index, a.ld_nodes, L, ocol}; ocol += L; }
    }
    h.drop = drop_run(&ta.drop_output, ta.drop_seed, 0, p.co);
    const bool drop_last = drop_at(&h.drop, no.n_layers);          // (a Dropout layer behind the last Dense: the network's output is its dropped-out copy)
    if (drop_last && !p.pooled) h.drop.buf[no.n_layers] = ta.y_pred;
    for (int l = 0; l < no.n_layers; ++l) h.hs[l] = (l == no.n_layers - 1 && !p.pooled && !drop_last) ? ta.y_pred : p.co.hid[l];
    h.out_nodes = drop_last ? h.drop.buf[no.n_layers] : h.hs[no.n_layers - 1];
    return 0;
}

// the output network in training mode: BatchNormalization statistics (`stats_ready`: already in p.stats_o), centred fold, layers, pooling
int head_forward(const gnn_train_args_t &ta, const StepPlan &p, const HeadRun &h, bool stats_ready, hipStream_t st) {
    const gnn_mlp_t &no = ta.loop.net_output;
    const bool bn_o = no.has_bn != 0;
    if (p.M > 0) {
        const float *W0 = no.kernel[0], *b0 = no.bias[0];
        const bool front = drop_at(&h.drop, 0);        // (a Dropout layer in front of the first Dense: the raw first layer over X0, normalised as X0 is made)
        if (bn_o) {
            if (!stats_ready) TRY(colstats_segs(nullptr, h.segs, h.nseg, p.M, p.stats_o, p.stats_o + no.in_dim, p.part, st));
            if (!front) TRY(fold_with_stats(no, p.stats_o, p.Wf_o, p.bf_o, st, true));      // (centred: the first layer subtracts the means on load)
            if (p.path != TrainPath::small) TRY(moving_output(ta, p, nullptr, st));
            if (!front) { W0 = p.Wf_o; b0 = p.bf_o; }
        }
        TRY(forward_layers(no, h.segs, h.nseg, p.M, W0, b0, h.hs, nullptr, st, nullptr, (bn_o && front) ? p.stats_o : nullptr, (bn_o && !front) ? p.stats_o : nullptr, &h.drop));
    }
    if (p.pooled) TRY(launch_aggregate(nullptr, ta.loop.nodegraph, h.out_nodes, p.T, p.T, ta.y_pred, p.T, st));
    return 0;
}

int add_into(float *dst, const float *src, size_t n, hipStream_t st) {      // dst += src
    gnn::k_axpby<<<std::min(cdiv((long)n, 256), 1024), 256, 0, st>>>(1.0f, dst, 1.0f, src, dst, n);
    LAUNCH_OK();
    return 0;
}

// the loss (mean over the R target rows) and d loss / d y_pred into p.dpred, scaled by `loss_scale` when it is neither 0 nor 1
int loss_and_dpred(const gnn_train_args_t &ta, const StepPlan &p, float loss_scale, hipStream_t st) {
    const int R1 = std::max(p.R, 1);
    gnn::k_loss_grad<<<cdiv(R1, 256), 256, 0, st>>>(ta.loss_kind, ta.targets, ta.y_pred, ta.sample_weight, p.R, p.T, p.dpred, p.loss_rows);
    LAUNCH_OK();
    if (p.R > 65536) {             // (one block summing a million rows took 0.9 ms)
        gnn::k_sum_partials<<<256, 256, 0, st>>>(p.loss_rows, p.R, p.loss_part);
        LAUNCH_OK();
        gnn::k_sum_scale<<<1, 256, 0, st>>>(p.loss_part, 256, 1.0f / (float)R1, ta.loss);
    } else gnn::k_sum_scale<<<1, 256, 0, st>>>(p.loss_rows, p.R, 1.0f / (float)R1, ta.loss);
    LAUNCH_OK();
    if (loss_scale != 0.0f && loss_scale != 1.0f) {
        gnn::k_axpby<<<std::min(cdiv((long)p.R * p.T, 256), 1024), 256, 0, st>>>(loss_scale, p.dpred, 0.0f, nullptr, p.dpred, (size_t)p.R * p.T);
        LAUNCH_OK();
    }
    return 0;
}

// ... with the upstream `d_pred_extra` added (`own_loss` false: no loss of its own, upstream gradients only); *G_out: d loss / d (the
// output network's rows), that is p.dpred through the pooling of a graph-focused model
int loss_gradient(const gnn_train_args_t &ta, const StepPlan &p, bool own_loss, float loss_scale, const float *d_pred_extra, float **G_out, hipStream_t st) {
    if (own_loss) TRY(loss_and_dpred(ta, p, loss_scale, st));
    else HIP_OK(hipMemsetAsync(p.dpred, 0, sizeof(float) * (size_t)p.R * p.T, st));
    if (d_pred_extra) TRY(add_into(p.dpred, d_pred_extra, (size_t)p.R * p.T, st));
    *G_out = p.dpred;
    if (p.pooled) { TRY(launch_aggregate(nullptr, ta.nodegraph_by_source, p.dpred, p.T, p.T, p.G_out, p.T, st)); *G_out = p.G_out; }
    return 0;
}

int scatter_add_rows(const float *D, int ld, const int *idx, int M, int width, float *G, int ldg, hipStream_t st) {      // G[idx[m]] += D[m]
    gnn::k_scatter_add_rows<<<std::min(cdiv((long)M * width, 256), 256 * 16), 256, 0, st>>>(D, ld, idx, M, width, G, ldg);
    LAUNCH_OK();
    return 0;
}

// back-propagation through the output network on the general kernels: its parameter gradients, its input gradient in p.dx_o_all, the
// state segments of it scatter-added into the zeroed p.G_state (an arc's two end nodes one after the other, in segment order)
int head_backward_general(const gnn_train_args_t &ta, StepPlan &p, HeadRun &h, float *G_out, hipStream_t st) {
    const gnn_mlp_t &no = ta.loop.net_output;
    HIP_OK(hipMemsetAsync(p.G_state, 0, sizeof(float) * (size_t)p.N * p.S, st));
    if (p.M == 0) return zero_grads(no, ta.grad_output, st);
    TRY(net_backward(p.co, h.segs, h.nseg, h.hs, G_out, p.T, p.M, no.has_bn ? p.stats_o : nullptr, false, p.dx_o_all, no.in_dim, p.part, st, -1, 0, &h.drop));
    gnn::BnGradReq rq[2];
    for (int i = 0; i < h.n_state; ++i) rq[i] = gnn::BnGradReq{p.dx_o_all + h.state_off[i], no.in_dim, h.state_k, h.ld_state, h.state_idx[i], p.S, h.state_off[i]};
    TRY(bn_input_grads(no, p.co, p.stats_o, rq, h.n_state, p.M, st));
    for (int i = 0; i < h.n_state; ++i) TRY(scatter_add_rows(p.dx_o_all + h.state_off[i], no.in_dim, h.state_idx[i], p.M, p.S, p.G_state, p.S, st));
    return 0;
}

// the end of a step (behind the caller's average_st_grads scaling of ITS state networks): the validity word, and the moving averages that waited for it
template <typename Plan>
int finish_step(const gnn_train_args_t &ta, const Plan &p, int k, hipStream_t st) {
    gnn::k_grads_ok<<<1, 1, 0, st>>>(p.path == TrainPath::small ? p.k_dev : nullptr, p.grads_ok);      // (only the persistent backward launch can fail)
    LAUNCH_OK();
    return moving_deferred(ta, p, k, p.grads_ok, st);
}

// ==== the homogeneous step's own phases, in the order train_step_impl() below calls them ==================================================

int moving_state(const gnn_train_args_t &ta, const TrainPlan &p, int k, const int *gate, hipStream_t st) {
    return bn_moving(ta.loop.net_state[0], p.stats_s, k, ta.bn_momentum, gate, st);
}

// ---- setup: the previous step's validity word, transposes, aggregates of the constants, state_0, iteration-invariant statistics ----------
// The validity word the previous call on this tape left is read stream-ordered behind that call's launches (on the host at this call's one
// synchronisation), then this call's is reset: 0 until the last launch of the step has been issued.
int train_setup(const gnn_train_args_t &ta, TrainPlan &p, hipStream_t st) {
    const gnn_loop_args_t &a = ta.loop;
    const gnn_mlp_t &ns = a.net_state[0];
    const bool xc_line = p.path == TrainPath::big && p.Kc > 0;      // the aggregates are columns of the constants line: filled in place, or adopted from the caller
    if (ta.prev_grads_ok_host) HIP_OK(hipMemcpyAsync(ta.prev_grads_ok_host, p.grads_ok, sizeof(int), hipMemcpyDeviceToHost, st));
    if (!ta.forward_only) {               // (a forward leaves the word of the last STEP on this tape as it is)
        HIP_OK(hipMemsetAsync(p.grads_ok, 0, sizeof(int) * 4, st));
        TRY(transposes(p.cs, st));
        TRY(transposes(p.co, st));
    }
    HIP_OK(hipMemsetAsync(p.flags, 0, sizeof(int) * (p.K + 8), st));
    HIP_OK(hipMemsetAsync(p.k_dev, 0, sizeof(float) * 4, st));
    if (xc_line) {
        if (!(a.xc && a.xc_mode == GNN_XC_VALID)) TRY(fill_constants_line(a, p.N, p.with_labels ? p.L : 0, p.A, p.xc, st));
    } else {
        if (p.A > 0) TRY(launch_aggregate(nullptr, a.arcnode, a.arc_labels, a.ld_arcs, p.A, p.agg_arcs, p.A, st));
        if (p.with_labels) TRY(launch_aggregate(nullptr, a.adjacency, a.nodes, a.ld_nodes, p.L, p.agg_nodes, p.L, st));
    }
    if (a.state_dim > 0 && p.ldS == p.S) HIP_OK(hipMemcpyAsync(p.states, a.state0, sizeof(float) * p.N * p.ldS, hipMemcpyDeviceToDevice, st));
    else if (a.state_dim > 0) TRY(launch_copy2d(nullptr, a.state0, p.S, p.states, p.ldS, p.N, p.S, p.ldS, st));
    else TRY(launch_copy2d(nullptr, a.nodes, a.ld_nodes, p.states, p.ldS, p.N, p.S, p.ldS, st));
    if (ns.has_bn && p.K > 0) {
        HIP_OK(hipMemsetAsync(p.stats_tpl, 0, sizeof(float) * 2 * p.in_s, st));
        if (xc_line) TRY(line_stats(p.xc, 32, p.N, p.part_y, p.cc.width, p.cc.wrow, p.cc.n, p.stats_tpl, p.in_s, st));
        else {
            gnn::Seg segs[GNN_MAX_SEGS], cst[GNN_MAX_SEGS];
            const int n = state_segs(a, p, 0, segs);
            int nc = 0;
            for (int s = 0; s < n; ++s) if (segs[s].ptr != p.states && segs[s].ptr != p.agg) cst[nc++] = segs[s];
            TRY(colstats_segs(nullptr, cst, nc, p.N, p.stats_tpl, p.stats_tpl + p.in_s, p.part, st));
        }
        gnn::k_replicate<<<std::min(cdiv((long)2 * p.in_s * p.K, 256), 1024), 256, 0, st>>>(p.stats_tpl, 2 * p.in_s, p.K, p.stats_s);
        LAUNCH_OK();
    }
    return finish_setup(ta, p, st);
}

// ---- training-mode forward: K gated iterations, tape = states + statistics + folded first layers -----------------------------------------
// Large graphs (kernels_train_big.hpp): the neighbour sum leaves its own column statistics, the dense kernel those of the state it writes (the next
// iteration's input); the statistics are folded into the weights (tiny launch) and the layer streams its rows straight into the matrix cores.
int forward_big(const gnn_train_args_t &ta, TrainPlan &p, hipStream_t st) {
    const gnn_loop_args_t &a = ta.loop;
    const gnn_mlp_t &ns = a.net_state[0];
    const bool bn_s = ns.has_bn != 0, bn_o = a.net_output.has_bn != 0;
    for (int t = 0; t < p.K; ++t) {
        const int *gate = p.flags + t;
        const float *s_t = state_at(p, t);
        float *agg_t = agg_at(p, t);
        float *stats = p.stats_s + (size_t)t * 2 * p.in_s;
        if (bn_s) {
            // (moments around the previous iteration's column means: one-pass sums, but nothing of the mean's size left to cancel)
            const float *prev = t > 0 ? p.stats_s + (size_t)(t - 1) * 2 * p.in_s : nullptr;
            TRY(launch_aggregate_stats(gate, a.adjacency, s_t, p.S, agg_t, p.part_a, stats + p.off_agg, stats + p.in_s + p.off_agg, prev ? prev + p.off_agg : nullptr, st));
            if (t == 0) {          // (later iterations: k_train_fwd_b6 leaves the statistics of the state it writes)
                int grid = 0;
                TRY(rows_stats(gate, s_t, p.S, p.S, p.N, p.part_y, st, &grid));
                gnn::k_stats_finish<<<p.S, 256, 0, st>>>(gate, p.part_y, grid, p.S, 1.0f / (float)p.N, stats, stats + p.in_s, s_t);
                LAUNCH_OK();
            }
        } else TRY(launch_aggregate(gate, a.adjacency, s_t, p.S, p.S, agg_t, p.S, st));
        // (the rows are centred by the kernel as they arrive - Sum a W (x - mean) + (b + Sum beta W): a folded bias b + Sum (beta - mean a) W
        //  would cancel Sum a W mean against itself, and inputs that sit far from zero - raw labels - lose that many digits of z)
        float *Wf = p.Wf_s + (size_t)t * p.in_s * p.H1s, *bf = p.bf_s + (size_t)t * p.H1s;
        if (bn_s) TRY(fold_with_stats(ns, stats, Wf, bf, st, true));
        gnn::TrainFwdArgs fa{};
        fa.in_mean = bn_s ? stats : nullptr;
        fa.gate = gate; fa.M = p.N;
        fa.state = s_t; fa.ld_state = p.S; fa.agg = agg_t; fa.ld_agg = p.S; fa.xc = p.Kc > 0 ? p.xc : nullptr;
        fa.Wf = bn_s ? Wf : ns.kernel[0]; fa.bf = bn_s ? bf : ns.bias[0]; fa.H = p.S; fa.wrow_state = 0; fa.wrow_agg = p.off_agg; fa.cs = p.cc;
        fa.act = ns.activation[0];
        fa.Y = state_at(p, t + 1); fa.ldy = p.S;
        fa.thr = a.state_threshold; fa.pred_flag = p.flags + t + 1; fa.pred_k = p.k_dev; fa.pred_kval = (float)(t + 1);
        const bool next_stats = bn_s && (t + 1 < p.K || (p.head_fast && bn_o));      // (the last state's: the output head's BatchNorm input)
        fa.stat_part = next_stats ? p.part_y : nullptr;
        fa.stat_shift = next_stats ? stats : nullptr;         // (the new state's moments around the input state's column means)
        int grid = 0;
        TRY(launch_train_fwd(fa, p.S, st, &grid));
        if (next_stats) {
            float *nxt = p.stats_s + (size_t)(t + 1) * 2 * p.in_s;
            gnn::k_stats_finish<<<p.S, 256, 0, st>>>(gate, p.part_y, grid, p.S, 1.0f / (float)p.N, nxt, nxt + p.in_s, stats);
            LAUNCH_OK();
        }
    }
    return 0;
}

// the Dropout form's arguments (p.drop_small): the layers of drop_state[0] by slot - 0 between the two Dense layers of the hidden form, 1 behind the
// last Dense - with the scalars gnn_dropout() derives for them; the kernels form every iteration's key from (seed, net_id, iteration, index) themselves
gnn::SmallDrop small_drop_args(const gnn_train_args_t &ta, const TrainPlan &p) {
    const gnn_dropout_spec_t &d = ta.drop_state[0];
    const int n_layers = ta.loop.net_state[0].n_layers;
    gnn::SmallDrop dr{};
    dr.seed = ta.drop_seed; dr.net_id = (unsigned)d.net_id; dr.ypre = p.sm_ypre;
    for (int i = 0; i < d.n; ++i) {
        const int slot = d.pos[i] == n_layers ? 1 : 0;
        const DropScalars sc = drop_scalars(d.rate[i], d.alpha, false);
        dr.on[slot] = 1; dr.index[slot] = (unsigned)d.index[i]; dr.thr[slot] = sc.thr; dr.mul[slot] = sc.mul; dr.add[slot] = sc.add; dr.fill[slot] = sc.fill;
    }
    return dr;
}

// Small graphs (kernels_train_small.hpp): all K gated iterations in one persistent launch, one workgroup per 64-node tile
int forward_small(const gnn_train_args_t &ta, TrainPlan &p, const gnn::TileTab &tiles, hipStream_t st) {
    const gnn_loop_args_t &a = ta.loop;
    const gnn_mlp_t &ns = a.net_state[0];
    const float *gamma = ns.has_bn ? ns.bn_gamma : nullptr;
    gnn::k_train_small_const<<<cdiv(p.N * p.SPs, 256), 256, 0, st>>>(p.N, p.SPs, p.H1s, const_segs_of(a, p), ns.kernel[0], ns.bias[0], gamma, ns.bn_beta, p.stats_tpl,
                                                                   p.stats_tpl + p.in_s, ns.bn_eps, p.sm_cc);
    LAUNCH_OK();
    HIP_OK(hipMemsetAsync(p.sm_bar, 0, sizeof(unsigned long long) * 4, st));
    gnn::TrainSmallFwdH fa{};      // (the one-layer launch takes its base part)
    fa.stats = p.stats_s; fa.in_s = p.in_s; fa.off_agg = p.off_agg;
    fa.W = ns.kernel[0]; fa.gamma = gamma; fa.beta = ns.bn_beta; fa.eps = ns.bn_eps; fa.act = ns.activation[0];
    if (p.hid_small) { fa.Hw = p.H1s; fa.W2 = ns.kernel[1]; fa.b2 = ns.bias[1]; fa.act2 = ns.activation[1]; fa.hid = p.sm_hid; }
    const gnn::SmallDrop dr = p.drop_small ? small_drop_args(ta, p) : gnn::SmallDrop{};
    return launch_train_small_fwd(fa, ta, p, tiles, nullptr, st, p.drop_small ? &dr : nullptr);
}

// the general path: one launch per layer and iteration
int forward_general(const gnn_train_args_t &ta, TrainPlan &p, hipStream_t st) {
    const gnn_loop_args_t &a = ta.loop;
    const gnn_mlp_t &ns = a.net_state[0];
    gnn::Seg segs[GNN_MAX_SEGS];
    for (int t = 0; t < p.K; ++t) {
        const int *gate = p.flags + t;
        const float *s_t = state_at(p, t);
        float *s_n = state_at(p, t + 1);
        TRY(launch_aggregate(gate, a.adjacency, s_t, p.S, p.S, agg_at(p, t), p.S, st));
        const int n = state_segs(a, p, t, segs);
        const gnn::Seg dyn[2] = {segs[0], segs[p.with_labels ? 2 : 1]};
        FirstLayer f;
        TRY(first_layer_of(ns, gate, dyn, p.N, p.stats_s + (size_t)t * 2 * p.in_s, p.Wf_s + (size_t)t * p.in_s * p.H1s, p.bf_s + (size_t)t * p.H1s, p.part, f, st,
                           drop_at_position(ta.drop_state[0], 0)));
        // Dropout layers (ABI 8): fresh masks every iteration (call = t); a layer behind the last Dense makes the NEW STATE the dropped-out
        // output (the tape holds it; the network's own output stays in its layer buffer for the backward recompute)
        DropRun drs = drop_run(&ta.drop_state[0], ta.drop_seed, t, p.cs);
        const bool drop_last = drop_at(&drs, ns.n_layers);
        if (drop_last) drs.buf[ns.n_layers] = s_n;
        float *hs[GNN_MAX_LAYERS];
        for (int l = 0; l < ns.n_layers; ++l) hs[l] = (l == ns.n_layers - 1 && !drop_last) ? s_n : p.cs.hid[l];
        PredFuse pf{s_t, p.S, a.state_threshold, p.flags + t + 1, p.k_dev, (float)(t + 1), false};
        TRY(forward_layers(ns, segs, n, p.N, f.W0, f.b0, hs, gate, st, &pf, f.bn_on_load, f.centre, &drs));
        if (!pf.fused) TRY(launch_converge(gate, s_n, s_t, p.N, p.S, p.S, p.S, a.state_threshold, p.flags + t + 1, p.k_dev, (float)(t + 1), st));
    }
    return 0;
}

// the thin head over every node of a large graph (p.head_fast) with BatchNormalization: the column statistics of [state_k | labels] are already on the
// tape - the state's were left by the launch that wrote it (k_train_fwd_b6's epilogue, slot k), the labels' are the state network's constant BatchNorm
// columns S .. S + L (one pass over the packed constants line) - four small copies instead of four passes over a million rows (0.76 ms of a C4-size step).
int head_stats_from_tape(const TrainPlan &p, int k, hipStream_t st) {
    const float *slot = p.stats_s + (size_t)k * 2 * p.in_s;
    HIP_OK(hipMemcpyAsync(p.stats_o, slot, sizeof(float) * p.S, hipMemcpyDeviceToDevice, st));
    HIP_OK(hipMemcpyAsync(p.stats_o + p.in_o, slot + p.in_s, sizeof(float) * p.S, hipMemcpyDeviceToDevice, st));
    if (p.with_labels) {
        HIP_OK(hipMemcpyAsync(p.stats_o + p.S, p.stats_tpl + p.S, sizeof(float) * p.L, hipMemcpyDeviceToDevice, st));
        HIP_OK(hipMemcpyAsync(p.stats_o + p.in_o + p.S, p.stats_tpl + p.in_s + p.S, sizeof(float) * p.L, hipMemcpyDeviceToDevice, st));
    }
    return 0;
}

// ---- label gradients (gnn_train_step_ex, kernels_train_labels.hpp): what the caller wants of d loss / d nodes, d loss / d arc labels ------
// `lab`: something of the constant segments' gradient is wanted (sum of dZ); `g0`: state_0 = nodes - iteration 0's input gradient IS consumed
struct LabelWants { bool nodes, arcs, lab, g0; };
LabelWants label_wants(const gnn_train_phase_args_t &px, const TrainPlan &p) {
    const bool nodes = px.d_nodes != nullptr, arcs = px.d_arc_labels != nullptr && p.A > 0 && p.E > 0;
    return LabelWants{nodes, arcs, (nodes && p.with_labels) || arcs, nodes && !p.with_labels};
}

// the label / arc-label segments of the general head's input gradient (scattered into the outputs at the end of the step)
int head_label_bn_grads(const gnn_train_args_t &ta, const TrainPlan &p, const HeadRun &h, const LabelWants &w, hipStream_t st) {
    const gnn_loop_args_t &a = ta.loop;
    const int node_part = p.with_labels ? p.S + p.L : p.S;         // columns of one endpoint / node in the output network's input
    gnn::BnGradReq lr[3]; int nl = 0;
    if (w.nodes && p.with_labels)
        for (int i = 0; i < h.n_state; ++i)
            lr[nl++] = gnn::BnGradReq{p.dx_o_all + h.state_off[i] + p.S, p.in_o, a.nodes, a.ld_nodes, h.state_idx[i], p.L, h.state_off[i] + p.S};
    if (w.arcs && a.focus == GNN_FOCUS_ARC)
        lr[nl++] = gnn::BnGradReq{p.dx_o_all + 2 * node_part, p.in_o, a.arc_labels, a.ld_arcs, a.out_index, p.A, 2 * node_part};
    return bn_input_grads(a.net_output, p.co, p.stats_o, lr, nl, p.M, st);
}

// ---- backward through the k executed iterations; p.G_state = d loss / d state_k ----------------------------------------------------------
// Small graphs: one persistent launch, then every workgroup's [kernel | bias] (and [d gamma | d beta]) share summed in workgroup order
int backward_small(const gnn_train_args_t &ta, TrainPlan &p, const gnn::TileTab &tiles, int k, const LabelWants &w, hipStream_t st) {
    const gnn_mlp_t &ns = ta.loop.net_state[0];
    gnn::TrainSmallBwdH ba{};      // (the one-layer launch takes its base part)
    ba.stats = p.stats_s; ba.in_s = p.in_s; ba.off_agg = p.off_agg;
    ba.cs = const_segs_of(ta.loop, p);
    ba.W = ns.kernel[0]; ba.gamma = ns.has_bn ? ns.bn_gamma : nullptr; ba.beta = ns.bn_beta; ba.eps = ns.bn_eps; ba.act = ns.activation[0];
    ba.dxa = p.dx_s_all; ba.partW = p.sm_partW; ba.partBN = p.sm_partBN;
    ba.dz_out = w.lab ? p.dz_sum : nullptr; ba.g0_out = w.g0 ? p.g0 : nullptr;
    if (p.hid_small) { ba.Hw = p.H1s; ba.W2 = ns.kernel[1]; ba.act2 = ns.activation[1]; ba.hid = p.sm_hid; ba.partW2 = p.sm_partW2; }
    const gnn::SmallDrop dr = p.drop_small ? small_drop_args(ta, p) : gnn::SmallDrop{};
    TRY(launch_train_small_bwd(ba, ta, p, k, tiles, nullptr, nullptr, st, p.drop_small ? &dr : nullptr));
    const int n = (p.in_s + 1) * p.H1s;
    gnn::k_reduce_partials<<<cdiv(n, 64), 256, 0, st>>>(p.sm_partW, p.n_wg, n, ta.grad_state.dkernel[0], 0, 1.0f, p.in_s * p.H1s, ta.grad_state.dbias[0]);
    LAUNCH_OK();
    if (p.hid_small) {          // the second layer's shares, in workgroup order like the first's
        const int n2 = (p.H1s + 1) * p.S;
        gnn::k_reduce_partials<<<cdiv(n2, 64), 256, 0, st>>>(p.sm_partW2, p.n_wg, n2, ta.grad_state.dkernel[1], 0, 1.0f, p.H1s * p.S, ta.grad_state.dbias[1]);
        LAUNCH_OK();
    }
    if (ns.has_bn) {
        gnn::k_reduce_partials<<<cdiv(2 * p.in_s, 64), 256, 0, st>>>(p.sm_partBN, p.n_wg, 2 * p.in_s, ta.grad_state.dgamma, 0, 1.0f, p.in_s, ta.grad_state.dbeta);
        LAUNCH_OK();
    }
    return 0;
}

// G_state = d state (own) + Adj . d agg, from the [state | agg] halves of p.dx_s_all (`c`: the arcs by source)
int transposed_state_aggregate(const gnn_csr_t &c, const TrainPlan &p, hipStream_t st) {
    const float *Xa = p.dx_s_all + p.S;
    const bool vec = (p.S == 16 || p.S == 32 || p.S == 64 || p.S == 128) && p.kdx_s % 4 == 0 &&
                     ((reinterpret_cast<uintptr_t>(Xa) | reinterpret_cast<uintptr_t>(p.dx_s_all) | reinterpret_cast<uintptr_t>(p.G_state)) & 15) == 0;
    if (!vec) return launch_aggregate_add(c, Xa, p.kdx_s, p.S, p.dx_s_all, p.kdx_s, p.G_state, p.S, st);
    // whole 16-B row pieces, 8 source rows in flight (the scalar walk is one dependent chain per arc)
    const int lpr = p.S / 4, groups = 256 / lpr, grid = std::min(cdiv(p.N, groups), 256 * 16);
    const bool buf = gather_buf_ok(c, p.kdx_s);
#define AGGV_(L, W_, B_) gnn::k_aggregate_vec<L, W_, B_><<<grid, 256, 0, st>>>(nullptr, c.n_dst, c.rowptr, c.src, c.w, c.row_scale, Xa, p.kdx_s, p.G_state, p.S, p.dx_s_all, p.kdx_s)
#define AGGV(L) (buf ? (c.w ? AGGV_(L, true, true) : AGGV_(L, false, true)) : (c.w ? AGGV_(L, true, false) : AGGV_(L, false, false)))
    switch (lpr) { case 4: AGGV(4); break; case 8: AGGV(8); break; case 16: AGGV(16); break; default: AGGV(32); break; }
#undef AGGV
#undef AGGV_
    LAUNCH_OK();
    return 0;
}

// the dZ form of a large-graph iteration's parameter gradients: P = X^T dZ and q on the matrix cores straight from the rows with their constants
// line, then the reduction and parameter-gradient kernels of net_backward.  `ba` != NULL: d loss / d [state | agg] from the same pass over the rows.
int big_dz_param_grads(TrainPlan &p, int t, bool first, const float *stats, const gnn::TrainBwdArgs *ba, hipStream_t st) {
    gnn::TrainWgradArgs wa{};
    const bool b6 = p.S != 16;                             // (k_train_wgrad_b6 / k_train_wgrad_dx_b6: one workgroup per CU, 64-row steps)
    const int n_wg = std::min(std::min((b6 ? 1 : 2) * device_cus(), BIG_WGRAD_BLOCKS), cdiv(p.N, 64));
    wa.M = p.N; wa.rows_per_wg = b6 ? cdiv(cdiv(p.N, n_wg), 64) * 64 : cdiv(cdiv(p.N, n_wg), 16) * 16;
    wa.G = p.G_state; wa.Y = nullptr; wa.act = GNN_ACT_LINEAR;      // (G_state holds dZ)
    wa.state = state_at(p, t); wa.agg = agg_at(p, t); wa.xc = p.xc;
    wa.K = p.in_s; wa.wrow_state = 0; wa.wrow_agg = p.off_agg; wa.Kc = p.Kc; wa.cs = p.cc;
    wa.part = p.part_w;
    wa.mean = stats;                       // (BatchNormalization: the rows are centred as they arrive, P arrives as P - mean q^T)
    const int grid = cdiv(p.N, wa.rows_per_wg);
    TRY(launch_train_wgrad(wa, ba, p.S, grid, st));
    return first_layer_grads(p.cs, p.part_w, grid, p.N, stats, !first, stats != nullptr, st);
}

// Large graphs (round 5): G_{t-1} leaves the transposed aggregate as dZ_{t-1} = G_{t-1} (.) act'(state_t) (k_aggregate_dz), so that the two dense kernels
// of an iteration read dZ alone; the first dZ comes from the output head (k_head_dx, or one k_act_grad pass behind the general head).  The weight gradient
// streams the rows with their constants line, whose 1 behind the Kc < 32 columns gives q = colsum(dZ): without constant inputs, or with 32, net_backward
// takes it and the plain transposed aggregate runs (`dzpath` false).  'average' / 'sum' / 'normalized' entries depend on the destination only (one scale
// per row): the input-gradient kernel scales the agg-half of a row's gradient once, and the transposed aggregate walks UNIT weights (no 4 bytes per arc).
int backward_big(const gnn_train_args_t &ta, TrainPlan &p, int k, bool dzpath, hipStream_t st) {
    const gnn_loop_args_t &a = ta.loop;
    const gnn_mlp_t &ns = a.net_state[0];
    const bool bn_s = ns.has_bn != 0, unit_w = !a.adjacency.w;
    gnn::Seg segs[GNN_MAX_SEGS];
    gnn_csr_t c = ta.adjacency_by_source;
    if (unit_w) { c.w = nullptr; c.row_scale = nullptr; }
    if (dzpath && k > 0 && !p.head_fast) TRY(act_grad_inplace(p.G_state, p.S, state_at(p, k), p.S, p.N, p.S, ns.activation[0], st));
    for (int t = k - 1; t >= 0; --t) {
        const float *s_t = state_at(p, t), *agg_t = agg_at(p, t);
        if (!p.agg_taped) TRY(launch_aggregate(nullptr, a.adjacency, s_t, p.S, p.S, p.agg, p.S, st));
        const float *stats = bn_s ? p.stats_s + (size_t)t * 2 * p.in_s : nullptr;
        gnn::TrainBwdArgs ba;                                    // d loss / d [state | agg] of this iteration
        memset(&ba, 0, sizeof(ba));
        ba.M = p.N; ba.dZ = p.G_state; ba.ldz = p.S;            // (net_backward: the activation gradient ran in place; dzpath: dZ arrived as such)
        ba.W = ns.kernel[0]; ba.ldw = p.H1s; ba.H = p.H1s; ba.S = p.S; ba.wrow_state = 0; ba.wrow_agg = p.off_agg;
        ba.state = s_t; ba.ld_state = p.S; ba.agg = agg_t; ba.ld_agg = p.S;
        if (bn_s) { ba.gamma = ns.bn_gamma; ba.mean = stats; ba.var = stats + p.in_s; ba.m1 = p.cs.m1; ba.m2 = p.cs.m2; ba.eps = ns.bn_eps; }
        ba.defer_state_bn = (dzpath && bn_s) ? 1 : 0;            // (k_aggregate_dz adds the rest of the state half's BatchNorm gradient: it reads state_t anyway)
        ba.agg_row_scale = unit_w ? a.adjacency.row_scale : nullptr;
        ba.dx = p.dx_s_all; ba.ld_dx = p.kdx_s;
        const bool dx_done = dzpath && p.S != 16 && t > 0 && !ba.gamma;      // both products from one pass over the rows
        if (dzpath) TRY(big_dz_param_grads(p, t, t == k - 1, stats, dx_done ? &ba : nullptr, st));
        else {
            float *hs[GNN_MAX_LAYERS] = {state_at(p, t + 1)};       // (one layer: its output is the next state on the tape)
            const int n = state_segs(a, p, t, segs);
            TRY(net_backward(p.cs, segs, n, hs, p.G_state, p.S, p.N, stats, t != k - 1, nullptr, 0, p.part, st, p.off_agg));
        }
        if (t == 0) break;                                       // nothing consumes d loss / d state_0: no input gradient, no transposed aggregate
        if (!dx_done) TRY(launch_train_bwd_dx(ba, p.S, st));
        if (!dzpath) { TRY(transposed_state_aggregate(c, p, st)); continue; }
        // dZ_{t-1} = (dx_state' + Adj . dx_agg + the deferred BatchNorm term) (.) act'(state_t)   (arcs walked by source)
        gnn::AggDzArgs z{};
        z.Y = s_t; z.ldy = p.S; z.wrow_state = 0;
        if (bn_s) { z.gamma = ns.bn_gamma; z.var = stats + p.in_s; z.mean = stats; z.m1 = p.cs.m1; z.m2 = p.cs.m2; z.eps = ns.bn_eps; }
        if (!launch_aggregate_dz(c, p.dx_s_all + p.S, p.kdx_s, p.G_state, p.S, p.dx_s_all, p.kdx_s, z, ns.activation[0], p.S, st))
            return fail("k_aggregate_dz: no instance for state width %d / activation %d", p.S, ns.activation[0]);
        LAUNCH_OK();
    }
    return 0;
}

// the general path: net_backward per iteration (hidden activations recomputed), then the transposed aggregate
int backward_general(const gnn_train_args_t &ta, TrainPlan &p, int k, const LabelWants &w, hipStream_t st) {
    const gnn_loop_args_t &a = ta.loop;
    const gnn_mlp_t &ns = a.net_state[0];
    const bool bn_s = ns.has_bn != 0, drop_any = ta.drop_state[0].n > 0;
    gnn::Seg segs[GNN_MAX_SEGS];
    for (int t = k - 1; t >= 0; --t) {
        const float *s_t = state_at(p, t), *agg_t = agg_at(p, t);
        if (!p.agg_taped) TRY(launch_aggregate(nullptr, a.adjacency, s_t, p.S, p.S, p.agg, p.S, st));
        const int n = state_segs(a, p, t, segs);
        const float *stats = bn_s ? p.stats_s + (size_t)t * 2 * p.in_s : nullptr;
        const DropRun drs = drop_run(&ta.drop_state[0], ta.drop_seed, t, p.cs);      // (iteration t's masks again: the same keys)
        float *hs[GNN_MAX_LAYERS];
        for (int l = 0; l < ns.n_layers; ++l) hs[l] = (l == ns.n_layers - 1 && !drop_any) ? state_at(p, t + 1) : p.cs.hid[l];
        TRY(recompute_hidden(ns, segs, n, p.N, stats, p.Wf_s + (size_t)t * p.in_s * p.H1s, p.bf_s + (size_t)t * p.H1s, hs, drs, drop_any, st));
        const bool dx_t = t > 0 || w.g0;                         // (label gradients with state_0 = nodes: iteration 0's input gradient too)
        TRY(net_backward(p.cs, segs, n, hs, p.G_state, p.S, p.N, stats, t != k - 1, dx_t ? p.dx_s_all : nullptr, dx_t ? p.kdx_s : 0, p.part, st, p.off_agg, 0, &drs,
                         w.lab ? p.dz_sum : nullptr));
        if (!dx_t) break;                                        // nothing consumes d loss / d state_0: no input gradient, no transposed aggregate
        gnn::BnGradReq rq[2] = {gnn::BnGradReq{p.dx_s_all, p.kdx_s, s_t, p.S, nullptr, p.S, 0},
                                gnn::BnGradReq{p.dx_s_all + p.S, p.kdx_s, agg_t, p.S, nullptr, p.S, p.off_agg}};
        TRY(bn_input_grads(ns, p.cs, stats, rq, 2, p.N, st));
        TRY(transposed_state_aggregate(ta.adjacency_by_source, p, st));
    }
    return 0;
}

// One row-parallel pass turns sum_t dZ_t into the gradients of the constant segments; the own-label columns plus the transposed aggregate of the aggregated-
// label columns are d loss / d nodes, the transposed ArcNode aggregate of the aggregated-arc columns d loss / d arc labels; the head's label segments on top.
int label_grads(const gnn_train_args_t &ta, const gnn_train_phase_args_t &px, const TrainPlan &p, const HeadRun &h, int k, const LabelWants &w, hipStream_t st) {
    const gnn_loop_args_t &a = ta.loop;
    const gnn_mlp_t &ns = a.net_state[0];
    const int ldn = px.ld_d_nodes > 0 ? px.ld_d_nodes : p.L;
    const int node_part = p.with_labels ? p.S + p.L : p.S;         // columns of one endpoint / node in the output network's input
    gnn::LabelGradArgs la{};
    la.N = p.N; la.H = p.H1s; la.ldz = p.ld_dz; la.DZ = p.dz_sum; la.W = ns.kernel[0];
    la.cs = const_segs_of(a, p);
    if (p.with_labels) {
        la.out[0] = w.nodes ? p.lab_own : nullptr; la.ldo[0] = p.L;
        la.out[1] = w.nodes ? p.lab_agg : nullptr; la.ldo[1] = p.L;
        la.out[2] = w.arcs ? p.arc_agg : nullptr; la.ldo[2] = p.A;
    } else { la.out[0] = w.arcs ? p.arc_agg : nullptr; la.ldo[0] = p.A; }
    if (ns.has_bn) { la.gamma = ns.bn_gamma; la.mean = p.stats_tpl; la.var = p.stats_tpl + p.in_s; la.dgamma = ta.grad_state.dgamma; la.dbeta = ta.grad_state.dbeta; la.eps = ns.bn_eps; }
    la.inv_n = 1.0f / (float)p.N;
    if (w.lab && p.Kc > 0 && p.K > 0) {
        gnn::k_label_grads<<<std::min(cdiv(p.N, gnn::LG_ROWS), 4096), 256, sizeof(float) * gnn::LG_ROWS * (p.H1s + 1), st>>>(la);
        LAUNCH_OK();
    }
    if (w.nodes && p.with_labels) {
        if (p.K > 0) TRY(launch_aggregate_add(ta.adjacency_by_source, p.lab_agg, p.L, p.L, p.lab_own, p.L, (float *)px.d_nodes, ldn, st));
        else HIP_OK(hipMemset2DAsync(px.d_nodes, sizeof(float) * ldn, 0, sizeof(float) * p.L, p.N, st));
        for (int i = 0; i < h.n_state && p.M > 0; ++i)
            TRY(scatter_add_rows(p.dx_o_all + h.state_off[i] + p.S, p.in_o, h.state_idx[i], p.M, p.L, (float *)px.d_nodes, ldn, st));
    } else if (w.nodes) {       // state_0 = nodes: d loss / d nodes is d loss / d state_0
        if (p.path == TrainPath::small && k > 0) TRY(launch_copy2d(nullptr, p.g0, p.SPs, px.d_nodes, ldn, p.N, p.L, p.L, st));
        else TRY(launch_copy2d(nullptr, p.G_state, p.S, px.d_nodes, ldn, p.N, p.L, p.L, st));
    }
    if (w.arcs) {
        if (p.K > 0) TRY(launch_aggregate(nullptr, px.arcnode_by_source, p.arc_agg, p.A, p.A, px.d_arc_labels, p.A, st));
        else HIP_OK(hipMemsetAsync(px.d_arc_labels, 0, sizeof(float) * (size_t)p.E * p.A, st));
        if (a.focus == GNN_FOCUS_ARC && p.M > 0) TRY(scatter_add_rows(p.dx_o_all + 2 * node_part, p.in_o, a.out_index, p.M, p.A, (float *)px.d_arc_labels, p.A, st));
    }
    return 0;
}

// ---- the phase block (gnn_train_phase_args_t) of gnn_train_step_ex / gnn_train_step_composite_ex: what both entry points ask of it ------
constexpr int32_t PHASE_MAGIC = 0x50483130;

// Is the phase block in use - any field but the by-source CSR, which only `d_arc_labels` reads?  An all-zero block is the plain gnn_train_step.
inline bool phase_block_used(const gnn_train_phase_args_t &px) {
    return px.phase != 0 || px.loss_scale != 0.0f || px.phase_state || px.node_out || px.d_pred_extra || px.d_out_extra || px.d_state_extra ||
           px.d_nodes || px.d_arc_labels;
}

// GNN_LOSS_NONE is phase 2's "no loss of its own"  (phase 1 with GNN_LOSS_NONE: the same args as the phase-2 call - the loss is not looked at)
inline int check_phase_loss_kind(const gnn_train_args_t &ta, const gnn_train_phase_args_t &px) {
    if (px.phase == 0 && ta.loss_kind == GNN_LOSS_NONE) return fail("GNN_LOSS_NONE is valid in phase %d only (a whole step needs a loss of its own)", GNN_TRAIN_PHASE_BACKWARD);
    return 0;
}

// The phase state against the plan's K and the leading dimension of `d_nodes` against its L; `who`: the entry point, for the message.
// (Two functions, not one: gnn_train_step_ex refuses GNN_LOSS_NONE in front of its coverage refusals and these checks behind them,
// gnn_train_step_composite_ex refuses both behind them - every caller keeps its order.)
inline int check_phase_state(const gnn_train_phase_args_t &px, int K, int L, const char *who) {
    if (px.phase != 0 && !px.phase_state) return fail("%s: phase %d needs phase_state", who, px.phase);
    if (px.phase == GNN_TRAIN_PHASE_BACKWARD && px.phase_state->magic != PHASE_MAGIC) return fail("%s: phase_state was not filled by a phase-1 call", who);
    if (px.phase == GNN_TRAIN_PHASE_BACKWARD && (px.phase_state->k < 0 || px.phase_state->k > K)) return fail("%s: phase_state holds k = %d", who, px.phase_state->k);
    if (px.d_nodes && px.ld_d_nodes != 0 && px.ld_d_nodes < L) return fail("%s: ld_d_nodes %d < dim_node_label %d", who, px.ld_d_nodes, L);
    return 0;
}

// heterogeneous models: train_composite.hpp (behind this file in the same translation unit)
int train_step_composite(const gnn_train_args_t &ta);
size_t composite_train_workspace_bytes(const gnn_train_args_t &ta);
// convergence groups of a training-mode forward (ABI 10): train_group.hpp (behind this file in the same translation unit)
int train_forward_groups(const gnn_train_args_t &ta);
size_t group_train_workspace_bytes(const gnn_train_args_t &ta);

}  // namespace

extern "C" {

size_t gnn_train_workspace_bytes(const gnn_train_args_t *args) {
    if (!args) { fail("args is NULL"); return 0; }
    if (args->n_groups != 0) return group_train_workspace_bytes(*args);
    if (args->loop.composite) return composite_train_workspace_bytes(*args);
    TrainPlan p;
    if (make_train_plan(*args, nullptr, p)) return 0;
    return p.bytes;
}

int gnn_train_xc_applies(const gnn_train_args_t *args) {
    if (!args || args->loop.composite || args->n_groups != 0) return 0;
    TrainPlan p;
    if (make_train_plan(*args, nullptr, p)) return 0;
    return p.path == TrainPath::big && p.Kc > 0 ? 1 : 0;
}

static int train_step_impl(const gnn_train_args_t &ta, const gnn_train_phase_args_t &px);

int gnn_train_step(const gnn_train_args_t *args) { return gnn_train_step_ex(args, nullptr); }

int gnn_train_phases_supported(const gnn_train_args_t *args) {
    if (!args || args->loop.composite || args->n_groups != 0 || args->forward_only) return -1;
    TrainPlan p;
    if (make_train_plan(*args, nullptr, p)) return -1;
    return (p.path == TrainPath::big || p.H1s > gnn::LG_MAX_H || p.front) ? -1 : 0;
}

int gnn_gate_all(const int32_t *const *words, int32_t n, int32_t *gate, void *stream) {
    if (!words || !gate || n < 1 || n > gnn::GATE_MAX_WORDS) return fail("gnn_gate_all: 1 .. %d words and a gate", gnn::GATE_MAX_WORDS);
    gnn::GateWords g{};
    g.n = n;
    for (int i = 0; i < n; ++i) { if (!words[i]) return fail("gnn_gate_all: word %d is NULL", i); g.w[i] = words[i]; }
    gnn::k_gate_all<<<1, 1, 0, (hipStream_t)stream>>>(g, gate);
    LAUNCH_OK();
    return 0;
}

// A call that fails behind its first launches has already fetched the previous step's validity word into *prev_grads_ok_host and reset
// the word on the tape: the copy must have LANDED when the caller looks at it (the caller's own view of the word is stale by then).  A call
// that fails in front of them leaves *prev_grads_ok_host as the caller initialised it (a sentinel) and the word on the tape untouched.
static int landed_on_failure(const gnn_train_args_t &ta, int rc) {
    if (rc != 0 && ta.prev_grads_ok_host && ta.tape) {
        const std::string msg = gnn_last_error();                 // (the synchronisation must not replace the message and its status)
        const int status = gnn_last_status();
        (void)hipStreamSynchronize((hipStream_t)ta.loop.stream);
        fail_as(status, "%s", msg.c_str());
    }
    return rc;
}

int gnn_train_step_ex(const gnn_train_args_t *args, const gnn_train_phase_args_t *px) {
    if (!args) return fail("args is NULL");
    gnn_train_phase_args_t none;
    memset(&none, 0, sizeof(none));
    return landed_on_failure(*args, train_step_impl(*args, px ? *px : none));
}

// the second argument block of gnn_train_step_ex against the plan: everything that refuses a call, before its first launch
static int check_phase_args(const gnn_train_args_t &ta, const gnn_train_phase_args_t &px, const TrainPlan &p) {
    TRY(check_phase_loss_kind(ta, px));
    if (!phase_block_used(px)) return 0;
    if (p.front) return not_covered("gnn_train_step_ex: a Dropout layer in front of a first Dense (GNN_FLAG_TRAIN_DROPOUT_FRONT) has no phases / upstream gradients / label gradients: such steps train through the building blocks");
    if (p.path == TrainPath::big) return not_covered("gnn_train_step_ex: the row-streaming path (>= GNN_TRAIN_BIG_MIN_NODES nodes) has no phases / upstream gradients / label gradients: such steps train through the building blocks");
    if (p.H1s > gnn::LG_MAX_H) return not_covered("gnn_train_step_ex: first state layer of %d units (at most %d)", p.H1s, gnn::LG_MAX_H);
    TRY(check_phase_state(px, p.K, p.L, "gnn_train_step_ex"));
    if (px.d_arc_labels && p.A > 0 && p.E > 0) {
        if (!px.arcnode_by_source.rowptr) return fail("gnn_train_step_ex: d_arc_labels needs arcnode_by_source");
        TRY(check_csr(px.arcnode_by_source, "arcnode_by_source", p.E, p.N));
    }
    return 0;
}

// The step as its phases.  Phase 1 (GNN_TRAIN_PHASE_FORWARD) stops behind the output network, in front of the loss: the tape is kept, and
// phase 2 (GNN_TRAIN_PHASE_BACKWARD) goes on from there with the k phase 1 learned at its synchronisation.
static int train_step_impl(const gnn_train_args_t &ta, const gnn_train_phase_args_t &px) {
    const gnn_loop_args_t &a = ta.loop;
    TrainPlan p;
    if (!ta.tape || ((uintptr_t)ta.tape & 255) != 0) return fail("tape must be a 256-byte aligned device buffer");
    const bool fwd_only = ta.forward_only != 0;                   // ABI 9: the training-mode forward alone (no loss, no gradients)
    const int phase = px.phase;
    if (phase < 0 || phase > GNN_TRAIN_PHASE_BACKWARD) return fail("gnn_train_step_ex: unknown phase %d", phase);
    // (this refusal has never counted a bare `phase_state`: a block with nothing else set asks for nothing, and a grouped, heterogeneous or
    // forward_only call that carries one stays the plain call - the one term of phase_block_used() left out here, explicitly)
    gnn_train_phase_args_t asked = px;
    asked.phase_state = nullptr;
    if (phase_block_used(asked) && (ta.n_groups != 0 || a.composite || fwd_only))
        return not_covered("gnn_train_step_ex: phases, upstream gradients and label gradients cover whole steps of homogeneous models only (gnn_train_phases_supported)");
    if (ta.n_groups != 0) return train_forward_groups(ta);         // ABI 10: independent convergence groups (train_group.hpp)
    if (a.composite) return train_step_composite(ta);             // one state network per node type (train_composite.hpp); honours forward_only
    if (fwd_only && ta.prev_grads_ok_host) return fail("gnn_train_step(forward_only): prev_grads_ok_host must be NULL");
    TRY(make_train_plan(ta, ta.tape, p));
    TRY(check_phase_args(ta, px, p));
    if (ta.tape_bytes < p.bytes) return fail("tape too small: %zu < %zu bytes", ta.tape_bytes, p.bytes);
    const bool big = p.path == TrainPath::big, small = p.path == TrainPath::small;
    if (big && p.Kc > 0) TRY(check_xc_args(a));
    const bool do_fwd = phase != GNN_TRAIN_PHASE_BACKWARD;        // phase 0 / 1: setup, loop, output network
    const bool no_loss = ta.loss_kind == GNN_LOSS_NONE && phase != 0;
    TRY(check_step_args(ta, p, !fwd_only && phase != GNN_TRAIN_PHASE_FORWARD && !no_loss, !fwd_only && phase != GNN_TRAIN_PHASE_FORWARD));
    const gnn_mlp_t &ns = a.net_state[0], &no = a.net_output;
    hipStream_t st = (hipStream_t)a.stream;
    GNN_SET_KERNEL_NAME(big ? "train_step: row-streaming kernels (kernels_train_big.hpp)" : p.drop_small ? (p.hid_small ? "train_step: persistent small-graph kernels (hidden layer, dropout)" : "train_step: persistent small-graph kernels (dropout)") : p.hid_small ? "train_step: persistent small-graph kernels (hidden layer)" : small ? "train_step: persistent small-graph kernels" : p.front ? "train_step: general kernels (dropout in front)" : "train_step: general kernels");
    gnn::TileTab tiles;
    TRY(tile_table(ta, p, tiles));
    if (!fwd_only && ta.grads_ok_dev) *ta.grads_ok_dev = p.grads_ok;

    // ---- forward: setup, the K gated iterations on the plan's path, k (the step's one synchronisation), the converged state -----------------
    int k = 0;
    if (do_fwd) {
        TRY(train_setup(ta, p, st));
        TRY(big ? forward_big(ta, p, st) : small ? forward_small(ta, p, tiles, st) : forward_general(ta, p, st));
        TRY(read_k(ta, p, &k, st));
        if (phase == GNN_TRAIN_PHASE_FORWARD) *px.phase_state = gnn_train_phase_state_t{PHASE_MAGIC, k, p.head_fast ? 0 : 1, 0};
        if (p.ldS == p.S) HIP_OK(hipMemcpyAsync(ta.state, state_at(p, k), sizeof(float) * p.N * p.ldS, hipMemcpyDeviceToDevice, st));
        else TRY(launch_copy2d(nullptr, state_at(p, k), p.ldS, ta.state, p.S, p.N, p.S, p.S, st));
        if (!small) TRY(moving_state(ta, p, k, nullptr, st));     // (the persistent path: moving_deferred)
    } else { k = px.phase_state->k; p.head_fast = false; }         // phase 2: what phase 1 learned at its synchronisation
    const float *state_k = state_at(p, k);

    // ---- output network, training mode ---------------------------------------------------------------------------------------------------------
    HeadRun h;
    TRY(head_segments(ta, p, state_k, p.ldS, p.with_labels ? p.L : 0, do_fwd, h, st));
    if (do_fwd) {
        const bool stats_on_tape = p.M > 0 && no.has_bn && p.head_fast && ns.has_bn && k >= 1;
        if (stats_on_tape) TRY(head_stats_from_tape(p, k, st));
        TRY(head_forward(ta, p, h, stats_on_tape, st));
        if (px.node_out && p.M > 0) HIP_OK(hipMemcpyAsync(px.node_out, h.out_nodes, sizeof(float) * (size_t)p.M * p.T, hipMemcpyDeviceToDevice, st));
    }
    if (phase == GNN_TRAIN_PHASE_FORWARD) return 0;               // THE PHASE CUT, in front of the loss: the tape is kept, phase 2 goes on from here
    if (fwd_only) return moving_deferred(ta, p, k, nullptr, st);  // the forward alone: what the persistent path keeps back for the validity word is due now

    // ---- loss and its gradient, upstream gradients added --------------------------------------------------------------------------------------
    float *G_out = nullptr;
    TRY(loss_gradient(ta, p, !no_loss, px.loss_scale, px.d_pred_extra, &G_out, st));
    if (px.d_out_extra && p.M > 0) TRY(add_into(G_out, px.d_out_extra, (size_t)p.M * p.T, st));
    const LabelWants want = label_wants(px, p);
    if (want.lab) HIP_OK(hipMemsetAsync(p.dz_sum, 0, sizeof(float) * (size_t)p.N * p.ld_dz, st));

    // ---- backward: output network, then the k iterations on the plan's path, label gradients ------------------------------------------------
    const bool dzpath = big && p.Kc > 0 && p.Kc < 32;             // (backward_big)
    if (p.head_fast) TRY(head_backward(p, a, p.with_labels ? a.nodes : nullptr, p.with_labels ? p.L : 0, state_k, p.ldS, h.out_nodes, G_out,
                                       no.has_bn ? p.stats_o : nullptr, st, (dzpath && k > 0) ? (int)ns.activation[0] : -1));
    else {
        TRY(head_backward_general(ta, p, h, G_out, st));
        if (want.lab && p.M > 0) TRY(head_label_bn_grads(ta, p, h, want, st));
    }
    if (px.d_state_extra) TRY(add_into(p.G_state, px.d_state_extra, (size_t)p.N * p.S, st));
    if (k == 0) TRY(zero_grads(ns, ta.grad_state, st));
    else TRY(big ? backward_big(ta, p, k, dzpath, st) : small ? backward_small(ta, p, tiles, k, want, st) : backward_general(ta, p, k, want, st));
    if (want.lab || want.g0) TRY(label_grads(ta, px, p, h, k, want, st));
    if (ta.average_st_grads && k > 0) TRY(scale_grads(ns, ta.grad_state, 1.0f / (float)k, st));
    return finish_step(ta, p, k, st);
}

#ifdef GNN_TS_TIMELINE
// phase times of workgroup 0 in the last persistent training launches: out[2][16] (forward, backward), ticks of 10 ns
int gnn_ts_phase_times(unsigned long long *out32) {
    return hipMemcpyFromSymbol(out32, HIP_SYMBOL(gnn::g_ts_phase), 2 * 16 * 8) == hipSuccess ? 0 : 1;
}
#endif

}  // extern "C"
