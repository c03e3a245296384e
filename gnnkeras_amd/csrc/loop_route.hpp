// Which kernel form a forward call runs - the one statement of the rule (host-only; included by gnnloop.hip behind the Plan).
// gnn_loop_forward, the per-iteration entry points (gnn_state_step, gnn_shard_*) and the queries (gnn_loop_groups_supported,
// gnn_loop_xc_applies, gnn_loop_route_name) read the LoopRoute / IterRoute computed here and decide nothing themselves;
// tests/golden/loop_routes.json records the answers over the boundaries of every condition below (no GPU needed).
// Host data only: dims, network descriptions, flags, the knobs (gnnloop.hip: knobs()), the group tables and WHETHER adjacency.w is
// NULL - never a workspace pointer, so a query that plans without a workspace answers what the launch does.
#pragma once

namespace {

enum class WholeLoop { none, lds, lds_types, small, mid };                 // the whole loop in one launch: which kernel is tried first
enum class IterKernel { unfused, fused2, fused4, wide, prefix, xwide };    // one launch (or a few) per iteration

struct IterRoute {
    IterKernel kernel;
    int fuse;           // fuse_class() of the model
    bool split_ok;      // the overlapped iteration (own-range partial sums + halo rows, gnn_shard_iteration_split*) can run
    bool fused() const { return kernel == IterKernel::fused2 || kernel == IterKernel::fused4 || kernel == IterKernel::wide; }
};

struct LoopRoute {
    WholeLoop whole;
    bool lds_hidden;    // whole == lds / lds_types: the hidden-layer form (GNN_FLAG_LDS_HIDDEN, two-layer state networks)
    bool small_setup;   // whole == small: k_setup_small builds the constants in one launch (then a 2 from the launcher is an error)
    bool try_mid;       // k_state_mid is tried: first (whole == mid), or after k_state_small answered 2 at launch
    IterRoute iter;     // what runs when no whole-loop kernel does, or when its launcher answers 2 (persistent_fits, tile budget)
    bool xc_loop;       // every iteration on the XC form of the wave-specialised kernel: C is never read
    bool xc_line;       // ... of a homogeneous graph: the constants line is filled in place / adopted (gnn_loop_args_t::xc)
    const char *refused;    // gnn_loop_forward fails with this text before its first launch (NULL: it runs); `whole` / `small_setup` then still say what the shapes alone would run
    int refused_status;     // ... and with this enum gnn_status (refuse() below)
    void refuse(int status, const char *text) { refused = text; refused_status = status; }
};

// the state network's LAST activation is a softmax (legal: reference MLP.py:12-78 takes any Keras activation): only the
// wave-specialised kernel's row-major epilogue has whole rows in one lane group, so that kernel runs whatever is pinned
bool state_softmax(const gnn_loop_args_t &a, const Plan &p) {
    for (int t = 0; t < p.T; ++t)
        if (a.net_state[t].n_layers >= 1 && a.net_state[t].activation[a.net_state[t].n_layers - 1] == GNN_ACT_SOFTMAX) return true;
    return false;
}

// 0: un-fused kernels; 1: any fused kernel; 2: two-layer state networks - only the wave-specialised kernel and the
// persistent whole-loop kernel carry the second Dense; 3: state width 65 .. 128 - the wide kernel, whatever generation is pinned.
int fuse_class(const gnn_loop_args_t &a, const Plan &p) {
    if ((a.flags & GNN_FLAG_UNFUSED) || p.SP > 128) return 0;      // W1 = [2SP x SP] floats must fit the CU's LDS: 128 KB at SP = 128 (kernel_state_wide.hpp)
    // the fused kernel addresses state rows and C with 32-bit byte offsets off a scalar base
    if ((size_t)(std::max(a.adjacency.n_src, p.N) + p.n_heavy) * p.SP * 4 >= ((size_t)1 << 32) || (size_t)p.N * p.ldC * 4 >= ((size_t)1 << 32)) return 0;
    // ... and the CSR arrays through 4 GiB buffer windows
    if ((size_t)iter_adjacency(a, p).nnz * 4 >= ((size_t)1 << 32) || ((size_t)p.N + 1) * 4 >= ((size_t)1 << 32)) return 0;
    // One Dense layer everywhere, or two with at most SP hidden units (the matrix waves have the time, and LDS holds a
    // second weight matrix in place of two ring slots).
    bool two = false;
    for (int t = 0; t < p.T; ++t) {
        const gnn_mlp_t &m = a.net_state[t];
        if (m.n_layers < 1 || m.n_layers > 2) return 0;
        if (m.activation[m.n_layers - 1] == GNN_ACT_SOFTMAX && p.SP > 64) return 0;   // a softmax state: the wave-specialised kernel only (widths up to 64)
        if (m.n_layers == 2 && (m.activation[0] == GNN_ACT_SOFTMAX || m.units[0] > p.SP)) return 0;
        if (t > 0 && (m.n_layers == 2) != two) return 0;                // every node type the same depth
        two = m.n_layers == 2;
    }
    if (p.SP == 128) return two ? 0 : 3;     // state widths 65 .. 128: one-layer state networks on the wide kernel
    return two ? 2 : 1;
}

// Which generation of the fused iteration kernel the SIZE asks for (GNN_FLAG_FUSED_GEN2 / 4, else GNN_FUSED_KERNEL = 2 / 4, else automatic):
//   4  wave-specialised (12 gather waves + 4 matrix waves per workgroup, 32 waves per CU)      <- d > 16 and >= 32768 nodes
//   2  phase-alternating (every wave gathers, then every wave multiplies; 16 waves per CU)      <- d <= 16 or small graphs
//      (measured crossover on ER graphs with 10 arcs / node, d = 64: 17.2 vs 16.4 us at 2e3 nodes, 28.3 vs 28.5 at 3e4,
//       60 vs 74 at 1e5, 480 vs 542 at 1e6)
// (a software-pipelined generation 3 lost to both at every size - profiles/r01_gather_sweep.txt - and was removed)
// A tuning knob, never a correctness switch: both are held to the same parity tests.  (A flag that pins a whole-loop generation,
// 5 .. 7, leaves this choice to the environment's 2 / 4.)  Also says whether the set-up packs the XC inputs.
int size_generation(const Plan &p, int flags) {      // (no per-call knob: cheap enough for every iteration)
    for (int pin : {(flags & GNN_FLAG_FUSED_GEN_MASK) >> 4, process_knobs().env_pin})      // the flag's pin, then the environment's
        if (pin == 2 || pin == 4) return pin;
    return (p.SP > 16 && p.N >= 32768) ? 4 : 2;
}

// State networks with two or more hidden layers (reference MLP.py:83-139 `hidden_units=[h1, h2, ..]`): the first TWO Dense layers run
// fused with the aggregate in the wave-specialised kernel's two-layer form, which then writes the second hidden layer's activations
// (not a state) - the remaining layers are plain dense launches over that matrix, the last one carrying the predicate.  Homogeneous models on
// one GPU, hidden widths within the padded state width; GNN_PREFIX_FUSION=0 or a pin by FLAG to a generation other than 4: the un-fused path.
bool prefix_covers(const gnn_loop_args_t &a, const Plan &p, const Knobs &k) {
    if ((a.flags & GNN_FLAG_UNFUSED) || !k.prefix_fusion || p.composite || p.T != 1 || p.tp[0].rows || a.nodes_src || p.n_groups > 0) return false;
    const gnn_mlp_t &m = a.net_state[0];
    if (m.n_layers < 3 || (p.SP != 32 && p.SP != 64)) return false;
    if (m.units[0] > p.SP || m.units[1] > p.SP || m.activation[0] == GNN_ACT_SOFTMAX || m.activation[1] == GNN_ACT_SOFTMAX) return false;
    if (k.flag_pin != 0 && k.flag_pin != 4) return false;
    if ((size_t)(p.N + p.n_heavy) * p.SP * 4 >= ((size_t)1 << 32) || (size_t)p.N * p.ldC * 4 >= ((size_t)1 << 32)) return false;
    return (size_t)iter_adjacency(a, p).nnz * 4 < ((size_t)1 << 32);
}

// State widths 129 .. 256 (kernel_state_xwide.hpp): homogeneous graphs, one Dense layer, no hub split (make_plan keeps hub rows
// off these widths), every array within the 32-bit byte offsets of a buffer window.  GNN_XWIDE=0 keeps the un-fused path.
bool xwide_covers(const gnn_loop_args_t &a, const Plan &p, const Knobs &k) {
    if (!k.xwide || (a.flags & GNN_FLAG_UNFUSED)) return false;
    if (p.SP <= 128 || p.S > 256 || p.composite || p.T != 1 || p.tp[0].rows || p.n_heavy != 0 || p.N < 1) return false;
    if (a.n_heavy_segments > 0) return false;      // hub rows (the caller's split says so): one gather wave would walk a hub two rows at a time
    const gnn_mlp_t &m = a.net_state[0];
    if (m.n_layers != 1 || m.activation[0] == GNN_ACT_SOFTMAX || (int)m.units[0] != p.S) return false;
    if ((size_t)std::max(a.adjacency.n_src, p.N) * p.SP * 4 >= ((size_t)1 << 32) || (size_t)p.N * p.ldC * 4 >= ((size_t)1 << 32)) return false;
    return (size_t)a.adjacency.nnz * 4 < ((size_t)1 << 32) && ((size_t)p.N + 1) * 4 < ((size_t)1 << 32);
}

// The kernel that runs ONE iteration: the size-based / pinned generation, except that a softmax state and two-layer state networks
// go to the wave-specialised kernel (the only per-iteration kernel that carries a second Dense) unless pinned below 4; padded
// width 128 is the wide kernel's whatever is pinned; what no fused kernel covers: three-layer prefix, widths 129 .. 256, un-fused.
IterRoute route_iteration(const gnn_loop_args_t &a, const Plan &p, const Knobs &k) {
    IterRoute r;
    r.fuse = fuse_class(a, p);
    int gen = size_generation(p, a.flags);
    if (state_softmax(a, p)) gen = 4;
    else if (r.fuse == 2 && p.SP > 16 && (k.pin == 0 || k.pin >= 4)) gen = 4;
    if (r.fuse == 3) r.kernel = IterKernel::wide;
    else if (r.fuse == 1 || (r.fuse == 2 && gen == 4)) r.kernel = gen == 4 ? IterKernel::fused4 : IterKernel::fused2;
    else if (prefix_covers(a, p, k)) r.kernel = IterKernel::prefix;
    else if (xwide_covers(a, p, k)) r.kernel = IterKernel::xwide;
    else r.kernel = IterKernel::unfused;
    // the wide kernel, or one-layer state networks on the wave-specialised kernel (not pinned elsewhere by flag); no hub rows
    r.split_ok = p.n_heavy == 0 && (r.fuse == 3 || (r.fuse == 1 && p.SP > 16 && (k.flag_pin == 0 || k.flag_pin == 4)));
    return r;
}

// The whole loop in ONE launch (kernel_state_small.hpp) for graphs of at most 64 nodes per CU: no hub rows, d <= 64, every tile resident.
bool small_covers(const gnn_loop_args_t &a, const Plan &p, const Knobs &k) {
    if ((k.pin != 0 && k.pin != 5) || p.n_heavy != 0 || a.max_iteration < 1 || (p.SP != 16 && p.SP != 32 && p.SP != 64)) return false;
    int tiles = 0;
    for (int t = 0; t < p.T; ++t) tiles += (p.tp[t].count + 63) / 64;
    if (p.n_groups > 0) tiles = p.group_tiles;
    return tiles > 0 && tiles <= std::min(device_cus(), GNN_SMALL_MAX_TILES);
}

// Small homogeneous graphs about to run the whole-loop kernel: BN folds, both constant aggregates, C, the predicate of
// state_0 and the zeroing of the loop words in ONE launch (kernels_setup.hpp) instead of five.
bool setup_small_covers(const gnn_loop_args_t &a, const Plan &p) {
    if (p.composite || p.N == 0) return false;
    const int L = a.state_dim > 0 ? p.L : 0, H = a.net_state[0].units[0];
    if (H > 128) return false;
    return gnn::setup_small_lds(H, 2 * L + p.A, std::max(a.net_state[0].in_dim, a.net_output.in_dim)) <= 64 * 1024;
}

// Mid-size graphs: the whole loop in one launch with several tiles per workgroup (kernel_state_mid.hpp).  Between the
// small whole-loop kernel's range (one tile per CU) and GNN_MID_MAX_NODES.  The default is where one launch per iteration
// of the wave-specialised kernel catches up (profiles/r02_mid_sweep.txt, 10 arcs per node: d = 64 25.4 vs 28.5 us at
// 30 000 nodes, 40.1 vs 35.7 at 45 000; d = 32 16.4 vs 17.6 at 30 000, 26.3 vs 26.1 at 60 000); pinned to generation 6: at any size.
bool mid_covers(const gnn_loop_args_t &a, const Plan &p, const Knobs &k) {
    if ((k.pin != 0 && k.pin != 6) || p.n_heavy != 0 || a.max_iteration < 1 || (p.SP != 32 && p.SP != 64) || p.N == 0) return false;
    return k.pin == 6 || p.N <= k.mid_max_nodes;
}

// Groups whose whole state fits the LDS of one CU: one workgroup per group, no grid barrier (generation 7).  What both kernels ask for:
bool lds_common(const gnn_loop_args_t &a, const Plan &p, const Knobs &k) {
    if ((k.pin != 0 && k.pin != 7) || p.n_groups < 1 || p.n_heavy != 0 || a.max_iteration < 1 || (p.SP != 16 && p.SP != 32)) return false;
    return !(a.flags & GNN_FLAG_UNFUSED) && !(p.has_sets && p.n_groups > device_cus());      // groups that wait for each other must all be resident
}
// The hidden-layer form of both kernels, opt-in (GNN_FLAG_LDS_HIDDEN): every type's state network Dense(H) - Dense(S).  `fuse` == 2 has
// checked H <= SP, no softmax on the hidden layer and the same depth for every type; the last activation must not be a softmax either.
bool lds_hidden_asked(const gnn_loop_args_t &a, const Plan &p, int fuse) {
    if (!(a.flags & GNN_FLAG_LDS_HIDDEN) || fuse != 2) return false;
    for (int t = 0; t < p.T; ++t) {
        const gnn_mlp_t &m = a.net_state[t];
        if (m.n_layers != 2 || m.units[0] < 1 || (int)m.units[1] != p.S || m.activation[1] == GNN_ACT_SOFTMAX) return false;
    }
    return true;
}
// ... a homogeneous model (kernel_state_lds.hpp): one Dense layer, or two in the hidden-layer form
bool lds_covers(const gnn_loop_args_t &a, const Plan &p, const Knobs &k, int fuse) {
    if (!lds_common(a, p, k) || p.composite) return false;
    if (fuse == 2 ? !lds_hidden_asked(a, p, fuse) : (a.net_state[0].n_layers != 1 || a.net_state[0].activation[0] == GNN_ACT_SOFTMAX)) return false;
    return gnn::lds_group_fits(p.group_max_nodes, p.SP, fuse == 2);          // (the hidden form's W2 / b2 come out of the group's LDS)
}
// ... a heterogeneous model (kernel_state_lds_types.hpp): every type's state network one Dense layer; the largest group must fit with
// every (group, type) range padded to 16 rows - decided from the shapes alone (type_nodes is a device array): rows <= n_g + 15 n_types.
bool lds_types_covers(const gnn_loop_args_t &a, const Plan &p, const Knobs &k, int fuse) {
    if (!lds_common(a, p, k) || !p.composite || p.T < 1 || p.T > GNN_MAX_TYPES || a.n_heavy_segments > 0 || a.nodes_src) return false;
    if (fuse == 2 && !lds_hidden_asked(a, p, fuse)) return false;      // (two layers per type: H and the activations may differ per type)
    for (int t = 0; fuse != 2 && t < p.T; ++t)
        if (a.net_state[t].n_layers != 1 || a.net_state[t].activation[0] == GNN_ACT_SOFTMAX || (int)a.net_state[t].units[0] != p.S) return false;
    if ((size_t)(p.N + (size_t)15 * p.T * p.n_groups) * p.SP * 4 >= ((size_t)1 << 32)) return false;      // the staging rows: 32-bit byte offsets
    return gnn::lds_types_group_fits(p.group_max_nodes, p.T, p.SP, fuse == 2);
}

#define GNN_ROUTE_STR_(x) #x
#define GNN_ROUTE_STR(x) GNN_ROUTE_STR_(x)
// The order of trial: groups that fit one CU each (typed for a composite model: nothing else runs composite groups); else the small
// whole-loop kernel, then the mid-size one, then one launch per iteration.  A softmax state: one launch per iteration.
LoopRoute route_loop(const gnn_loop_args_t &a, const Plan &p) {
    const Knobs k = knobs(a.flags);
    LoopRoute r = {};
    r.iter = route_iteration(a, p, k);
    const int fz = r.iter.fuse;
    const bool fz12 = fz == 1 || fz == 2;       // (2: two-layer state networks - the hidden-layer form, where the caller asked for it)
    if (p.n_groups > 0 && fz12 && lds_covers(a, p, k, fz) && setup_small_covers(a, p)) { r.whole = WholeLoop::lds; r.lds_hidden = fz == 2; return r; }
    if (p.n_groups > 0 && p.composite) {
        if (fz12 && lds_types_covers(a, p, k, fz)) { r.whole = WholeLoop::lds_types; r.lds_hidden = fz == 2; }
        else r.refuse(GNN_STATUS_NOT_COVERED, "convergence groups of a composite graph need the one-CU-per-group kernel (gnn_loop_groups_supported() != 2 for these args)");
        return r;
    }
    const bool soft = state_softmax(a, p);
    const bool small = fz != 0 && !soft && small_covers(a, p, k);
    r.small_setup = small && setup_small_covers(a, p);
    r.try_mid = !r.small_setup && fz == 1 && !soft && mid_covers(a, p, k);
    r.whole = small ? WholeLoop::small : r.try_mid ? WholeLoop::mid : WholeLoop::none;
    // (sets: an error, not NOT_COVERED - the callers that rerun a refused merge batch by batch have never done so for this one)
    if (p.has_sets) r.refuse(GNN_STATUS_ERROR, "convergence group sets need the one-CU-per-group form (gnn_loop_groups_supported() != 2 for these args)");
    else if (p.n_groups > GNN_MAX_GROUPS)
        r.refuse(GNN_STATUS_NOT_COVERED, "more than " GNN_ROUTE_STR(GNN_MAX_GROUPS) " convergence groups need every group to fit one CU's LDS (gnn_loop_groups_supported() != 2)");
    else if (p.n_groups > 0 && !r.small_setup) r.refuse(GNN_STATUS_NOT_COVERED, "convergence groups need the whole-loop kernel (gnn_loop_groups_supported() == 0 for these args)");
    if (r.refused) return r;
    // the XC form: decided from the static part of the small kernel's answer, and only where the mid-size kernel is not tried
    r.xc_loop = p.xc_ok && !small && fz == 1 && !r.try_mid && p.SP != 128 && !iter_adjacency(a, p).w &&
                r.iter.kernel == IterKernel::fused4 && size_generation(p, a.flags) == 4;
    r.xc_line = r.xc_loop && !p.composite && p.N > 0;
    return r;
}

// gnn_loop_route_name(): the kernel stems are what the launchers report through gnn_last_kernel_name()
void route_name(const LoopRoute &r, char *name, size_t n) {
    static const char *const stem[] = {"k_aggregate_vec", "k_state_fused2", "k_state_fused4", "k_state_wide", "k_state_fused4<.., L2>", "k_state_xwide_b3"};      // (IterKernel)
    if (r.refused) snprintf(name, n, "refused: %s", r.refused);
    else if (r.whole == WholeLoop::lds) snprintf(name, n, r.lds_hidden ? "k_state_lds<.., hidden>" : "k_state_lds");
    else if (r.whole == WholeLoop::lds_types) snprintf(name, n, r.lds_hidden ? "k_state_lds_types<.., hidden>" : "k_state_lds_types");
    else if (r.small_setup) snprintf(name, n, "k_state_small(setup_small)");
    else snprintf(name, n, "%s%s%s%s", r.whole == WholeLoop::small ? "k_state_small > " : "", r.try_mid ? "k_state_mid > " : "",
                  stem[(int)r.iter.kernel], r.xc_loop ? "+xc" : "");
}

}  // namespace
