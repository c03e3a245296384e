/* The host side of the phased training step (gnn_train_step_ex, include/gnnloop.h) driven from plain C without a GPU: the argument
 * checks of the second argument block, the coverage query, the plan / workspace layout that phase 1 and phase 2 share (one tape,
 * one phase_state), up to the first refused call or the first HIP error.  Meant for a sanitizer build of the HOST code: no device is
 * needed, no kernel runs.
 *
 * Build and run (AddressSanitizer + UBSan on the host code of the library and of this file; `make -C gnnkeras_amd/csrc asan` builds
 * libgnnloop_asan.so with `-fsanitize=address,undefined -fno-gpu-sanitize`; the same compiler links this file, so that both share one
 * sanitizer runtime):
 *   make -C gnnkeras_amd/csrc asan
 *   /opt/rocm/llvm/bin/clang -std=c99 -g -fsanitize=address,undefined -fno-omit-frame-pointer -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include \
 *       -Iinclude examples/joint_phases_host.c -Lgnnkeras_amd/csrc -l:libgnnloop_asan.so -L/opt/rocm/lib -lamdhip64 \
 *       -Wl,-rpath,$PWD/gnnkeras_amd/csrc -Wl,-rpath,/opt/rocm/lib -o joint_phases_host
 *   ./joint_phases_host
 * Exit code 0 and a line "joint_phases_host: OK ..." when every call answered as expected. */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "gnnloop.h"

static int failures = 0;
#define EXPECT(cond, what) do { if (!(cond)) { fprintf(stderr, "FAILED line %d: %s (last error: %s, status %d)\n", __LINE__, what, gnn_last_error(), gnn_last_status()); ++failures; } } while (0)

/* addresses that are never dereferenced on the host: the library hands them to the device */
#define FAKE(n) ((void *)(uintptr_t)(0x10000000u + 4096u * (n)))

static void fill(gnn_train_args_t *ta, int n_nodes, int d, int L, int A, int T, int focus, int state_layers) {
    memset(ta, 0, sizeof(*ta));
    gnn_loop_args_t *a = &ta->loop;
    const int S = d > 0 ? d : L, n_arcs = 2 * n_nodes;
    a->abi_version = GNN_ABI_VERSION; a->n_types = 1;
    a->n_nodes = n_nodes; a->n_arcs = n_arcs; a->dim_node_label = L; a->dim_arc_label = A;
    a->nodes = (const float *)FAKE(1); a->ld_nodes = L; a->arc_labels = (const float *)FAKE(2); a->ld_arcs = A + 2;
    a->state_dim = d; a->max_iteration = 4; a->state_threshold = 0.01f; a->state0 = (const float *)FAKE(3);
    gnn_mlp_t *m = &a->net_state[0];
    m->in_dim = d > 0 ? 2 * S + 2 * L + A : 2 * S + A; m->n_layers = state_layers;
    for (int i = 0; i < state_layers; ++i) {
        m->units[i] = i == state_layers - 1 ? S : 12; m->activation[i] = GNN_ACT_TANH;
        m->kernel[i] = (const float *)FAKE(10 + i); m->bias[i] = (const float *)FAKE(20 + i);
    }
    gnn_mlp_t *o = &a->net_output;
    const int node_part = d > 0 ? S + L : S;
    o->in_dim = focus == GNN_FOCUS_ARC ? 2 * node_part + A : node_part; o->n_layers = 1;
    o->units[0] = T; o->activation[0] = GNN_ACT_SOFTMAX; o->kernel[0] = (const float *)FAKE(30); o->bias[0] = (const float *)FAKE(31);
    a->focus = focus; a->n_out = focus == GNN_FOCUS_ARC ? n_arcs : n_nodes; a->out_index = (const int32_t *)FAKE(4);
    a->arc_src = (const int32_t *)FAKE(5); a->arc_dst = (const int32_t *)FAKE(6);
    gnn_csr_t csr;
    memset(&csr, 0, sizeof(csr));
    csr.rowptr = (const int32_t *)FAKE(40); csr.src = (const int32_t *)FAKE(41);
    csr.n_dst = n_nodes; csr.n_src = n_nodes; csr.nnz = n_arcs; a->adjacency = csr; ta->adjacency_by_source = csr;
    csr.n_src = n_arcs; a->arcnode = csr;
    if (focus == GNN_FOCUS_GRAPH) {
        csr.n_dst = 12; csr.n_src = n_nodes; csr.nnz = n_nodes; a->nodegraph = csr;
        csr.n_dst = n_nodes; csr.n_src = 12; ta->nodegraph_by_source = csr;
    }
    ta->targets = (const float *)FAKE(50); ta->loss_kind = 0; ta->bn_momentum = 0.99f;
    ta->grad_state.dkernel[0] = (float *)FAKE(60); ta->grad_state.dbias[0] = (float *)FAKE(61);
    ta->grad_state.dkernel[1] = (float *)FAKE(62); ta->grad_state.dbias[1] = (float *)FAKE(63);
    ta->grad_output.dkernel[0] = (float *)FAKE(64); ta->grad_output.dbias[0] = (float *)FAKE(65);
    ta->y_pred = (float *)FAKE(70); ta->state = (float *)FAKE(71); ta->loss = (float *)FAKE(72);
}

int main(void) {
    static gnn_train_args_t ta;
    gnn_train_phase_args_t px;
    gnn_train_phase_state_t ps;
    int32_t k_host = -7;
    if (gnn_abi_version() != GNN_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 2; }
    /* the addresses below are not memory: where a device IS present nothing of this may get near a launch */
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) == hipSuccess && n_dev > 0) { printf("joint_phases_host: a HIP device is present - this program is for hosts without one, nothing done\n"); return 0; }
    EXPECT(gnn_struct_size(4) == sizeof(gnn_train_args_t) && gnn_struct_size(8) == sizeof(px) && gnn_struct_size(9) == sizeof(ps), "struct sizes");

    /* ---- coverage: dims and network descriptions only -------------------------------------------------------------------------- */
    const int foci[3] = {GNN_FOCUS_NODE, GNN_FOCUS_ARC, GNN_FOCUS_GRAPH};
    const int shapes[6][3] = {{8, 14, 3}, {8, 24, 3}, {0, 14, 3}, {0, 46, 3}, {40, 14, 3}, {6, 14, 7}};      /* d, L, A */
    size_t bytes_seen = 0;
    for (int f = 0; f < 3; ++f)
        for (int s = 0; s < 6; ++s)
            for (int layers = 1; layers <= 2; ++layers) {
                fill(&ta, 203, shapes[s][0], shapes[s][1], shapes[s][2], 2, foci[f], layers);
                EXPECT(gnn_train_phases_supported(&ta) == 0, "a MUTAG-sized shape is covered");
                const size_t need = gnn_train_workspace_bytes(&ta);      /* the plan both phases carve from the same tape */
                EXPECT(need > 0 && need % 256 == 0, "workspace bytes");
                bytes_seen += need;
            }
    fill(&ta, 32768, 16, 14, 3, 2, GNN_FOCUS_NODE, 1);
    EXPECT(gnn_train_phases_supported(&ta) == -1, "the row-streaming path is not covered");
    fill(&ta, 203, 8, 14, 3, 2, GNN_FOCUS_NODE, 1); ta.loop.composite = 1;
    EXPECT(gnn_train_phases_supported(&ta) == -1, "composite models are not covered");
    EXPECT(gnn_train_phases_supported(NULL) == -1, "NULL arguments");

    /* ---- refused calls: each fails with a message before the first launch -------------------------------------------------------- */
    fill(&ta, 203, 8, 14, 3, 2, GNN_FOCUS_ARC, 1);
    ta.k_host = &k_host; ta.tape = FAKE(100); ta.tape_bytes = gnn_train_workspace_bytes(&ta);
    memset(&px, 0, sizeof(px)); memset(&ps, 0, sizeof(ps));
    px.phase = GNN_TRAIN_PHASE_BACKWARD;
    EXPECT(gnn_train_step_ex(&ta, &px) != 0 && strstr(gnn_last_error(), "needs phase_state"), "phase 2 without phase_state");
    px.phase_state = &ps;
    EXPECT(gnn_train_step_ex(&ta, &px) != 0 && strstr(gnn_last_error(), "not filled by a phase-1 call"), "phase 2 on a phase_state no phase 1 filled");
    memset(&px, 0, sizeof(px));
    ta.loss_kind = GNN_LOSS_NONE;
    EXPECT(gnn_train_step_ex(&ta, &px) != 0 && strstr(gnn_last_error(), "GNN_LOSS_NONE"), "GNN_LOSS_NONE in a whole step");
    ta.loss_kind = 0;
    px.d_arc_labels = (float *)FAKE(80);
    EXPECT(gnn_train_step_ex(&ta, &px) != 0 && strstr(gnn_last_error(), "arcnode_by_source"), "d_arc_labels without arcnode_by_source");
    memset(&px, 0, sizeof(px));
    px.d_nodes = (float *)FAKE(81); px.ld_d_nodes = 13;
    EXPECT(gnn_train_step_ex(&ta, &px) != 0 && strstr(gnn_last_error(), "ld_d_nodes"), "a leading dimension below the label width");
    memset(&px, 0, sizeof(px));
    px.phase = 3;
    EXPECT(gnn_train_step_ex(&ta, &px) != 0 && strstr(gnn_last_error(), "unknown phase"), "an unknown phase");
    ta.tape_bytes -= 256;
    memset(&px, 0, sizeof(px)); px.phase = GNN_TRAIN_PHASE_FORWARD; px.phase_state = &ps;
    EXPECT(gnn_train_step_ex(&ta, &px) != 0 && strstr(gnn_last_error(), "tape too small"), "a tape one block short");
    ta.tape_bytes += 256;
    EXPECT(k_host == -7 && ps.magic == 0 && ps.k == 0, "refused calls write nothing");

    /* ---- phase 1 with complete arguments: every host check passes; without a device the first HIP call ends it ------------------------ */
    px.node_out = (float *)FAKE(82);
    const int rc = gnn_train_step_ex(&ta, &px);
    printf("phase 1 on complete arguments: rc = %d (%s, status %d)\n", rc, rc ? gnn_last_error() : "ran", rc ? gnn_last_status() : GNN_STATUS_OK);
    EXPECT(rc != 0 && ps.magic == 0, "a phase 1 that did not reach its synchronisation leaves phase_state alone");
    px.phase = GNN_TRAIN_PHASE_BACKWARD;      /* ... so the phase 2 that follows it is refused, not run on a stale tape */
    EXPECT(gnn_train_step_ex(&ta, &px) != 0 && strstr(gnn_last_error(), "not filled by a phase-1 call"), "phase 2 behind a failed phase 1");
    if (failures) { fprintf(stderr, "joint_phases_host: %d check(s) failed\n", failures); return 1; }
    printf("joint_phases_host: OK (36 plans, %zu workspace bytes in all)\n", bytes_seen);
    return 0;
}
