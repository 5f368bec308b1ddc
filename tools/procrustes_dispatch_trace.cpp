// Records what basd_procrustes_forward_fused (csrc/fused.hip) launches, without a GPU and without the HIP runtime, in
// the manner of jacobi_dispatch_trace.cpp: procrustes.o, fused.o, jacobi.o and gemm.o are linked against the stand-ins
// of hip_trace_standins.h.  Two builds -- one against the objects of a parent commit, one against the working tree --
// must print the same bytes over the sweep: launch names, grids, blocks, LDS bytes, function attributes, fills and
// return codes.  (Scalar kernel arguments are not seen: those are compared by eye in the diff.)
//
//   make -C vit-inductive-bias-distillation_amd/csrc          (objects: O = vit-inductive-bias-distillation_amd/csrc)
//   g++ -O1 -std=c++17 tools/procrustes_dispatch_trace.cpp $O/procrustes.o $O/fused.o $O/jacobi.o $O/gemm.o -o ptrace
//   ./ptrace options | layouts | shapes > trace.txt          (a summary line goes to stderr)
//   ./ptrace plans                                           (the planner's answer per call; needs the query)
//
// Pointers handed in are never dereferenced by the launcher except student_host_ptrs, which is a real host array.
#include "hip_trace_standins.h"

extern "C" int basd_procrustes_plan_query(const BasdProcrustesArgs*, long*) __attribute__((weak));

static const int kOrders[] = {4, 16, 20, 49, 64, 65, 100, 144, 196, 197, 252, 253, 576, 664, 665};
static const int kE[] = {1, 2, 4, 5, 12}, kL[] = {1, 3, 4, 24};

struct Case {
    int E, L, B, n_s, n_t, d_s, d_t;
    int s_bf16, s_layout;        // 0 aligned, 1 row stride not a multiple of 16 bytes, 2 base pointers not aligned
    int t_bf16, t_layout;        // 0 row-major aligned, 1 row stride odd, 2 features strided (sd != 1)
    unsigned opts;               // bit 0 k_prime, 1 dx (+ h, grad_layers), 2 raw, 3 w_stack (+ sigma_u), 4 jac_ws,
                                 // 5 split teacher Gram, 6 uw_ce (+ uw_out), 7 sweeps
    int hook, finish;
};
static bool g_plans = false;

static uintptr_t fake(int i) { return 0x100000 + 0x1000 * (uintptr_t)i; }      // 16-byte aligned, never dereferenced
template <typename T> static T* at(int i) { return (T*)fake(i); }

static void run(const Case& c) {
    static const void* host_ptrs[16];
    BasdProcrustesArgs a = {};
    const int n = c.n_s < c.n_t ? c.n_s : c.n_t, G = c.L == 1 ? 1 : c.E;
    for (int e = 0; e < c.E; ++e) host_ptrs[e] = (const void*)(fake(100 + e) + (c.s_layout == 2 ? 4 : 0));
    a.student_ptrs = at<const void*>(1);
    a.student_host_ptrs = host_ptrs;
    a.s_dtype = c.s_bf16;
    a.s_sn = c.d_s + (c.s_layout == 1 ? 1 : 0);
    a.s_sb = a.s_sn * c.n_s;
    a.s_aligned = c.s_layout != 2;
    a.tok_ptrs = at<const void*>(2);
    a.t_dtype = c.t_bf16;
    if (c.t_layout == 2) { a.t_sd = c.n_t; a.t_sn = 1; a.t_sb = (long)c.n_t * c.d_t; }
    else { a.t_sd = 1; a.t_sn = c.d_t + (c.t_layout == 1 ? 1 : 0); a.t_sb = a.t_sn * c.n_t; }
    a.attn_ptrs = at<const void*>(3);
    a.a_dtype = 0; a.a_sk = 1; a.a_sq = c.n_t; a.a_sh = (long)c.n_t * c.n_t; a.a_sb = 4 * a.a_sh;
    a.mix = at<float>(4);
    a.E = c.E; a.L = c.L; a.G = G; a.B = c.B; a.n_s = c.n_s; a.n_t = c.n_t; a.d_s = c.d_s; a.d_t = c.d_t;
    a.H = 4; a.A = c.n_t; a.has_cls = 0; a.n_a = c.n_t; a.n = n; a.max_sweeps = 2;
    if (c.n_t != c.n_s) { a.atap0 = at<int>(5); a.atap1 = at<int>(6); a.alam = at<float>(7); }
    if (c.n_t < c.n_s) { a.tap0 = at<int>(8); a.tap1 = at<int>(9); a.lam = at<float>(10); a.range0 = at<int>(11); a.range1 = at<int>(12); }
    if (c.n_t > c.n_s) { a.g0 = at<int>(13); a.g1 = at<int>(14); a.glam = at<float>(15); }
    a.omega = at<float>(16); a.omega_t = at<float>(17); a.mu_t = at<float>(18); a.tc = at<float>(19);
    a.mu_s = at<float>(20); a.tr_part = at<float>(21); a.tr_s = at<float>(22); a.a_prime = at<float>(23);
    a.g_all = at<double>(24); a.l_all = at<double>(25); a.W = at<float>(26); a.sigma = at<float>(27);
    a.jflags = at<int>(28); a.tr_t = at<float>(29); a.nuc = at<float>(30); a.loss_b = at<float>(31);
    if (c.opts & 1) a.k_prime = at<float>(32);
    if (c.opts & 2) { a.dx = at<float>(33); a.h = at<float>(34); a.grad_layers = at<float>(35); }
    if (c.opts & 4) a.raw = at<float>(36);
    if (c.opts & 8) { a.w_stack = at<float>(37); a.sigma_u = at<float>(38); }
    if (c.opts & 16) a.jac_ws = at<void>(39);
    a.g_splits = 1;
    if (c.opts & 32) { a.g_slabs = at<double>(40); a.g_splits = 4; }
    if (c.opts & 64) { a.uw_ce = at<float>(41); a.uw_out = at<float>(42); }
    if (c.opts & 128) a.sweeps = at<int>(43);
    basd_procrustes_tuning(c.hook);
    basd_procrustes_finish_tuning(c.finish);
    char what[256];
    snprintf(what, sizeof what, "E=%d L=%d B=%d n_s=%d n_t=%d d_s=%d d_t=%d s=%s/%d t=%s/%d opts=%02x hook=%d finish=%d", c.E,
             c.L, c.B, c.n_s, c.n_t, c.d_s, c.d_t, c.s_bf16 ? "bf16" : "f32", c.s_layout, c.t_bf16 ? "bf16" : "f32",
             c.t_layout, c.opts, c.hook, c.finish);
    if (g_plans) {
        long p[20] = {};
        const int rc = basd_procrustes_plan_query(&a, p);
        printf("%s rc=%d plan", what, rc);
        for (long v : p) printf(" %ld", v);
        printf("\n");
        ++g_calls;
        return;
    }
    finish_call(what, basd_procrustes_forward_fused(&a, nullptr));
}

// E * B on both sides of 128 and of 65535, and a batch of a few samples
static int batches(int E, int* out) {
    int k = 0;
    out[k++] = 2;
    out[k++] = (127 / E) > 0 ? 127 / E : 1;
    out[k++] = (128 + E - 1) / E;
    out[k++] = 65535 / E;
    out[k++] = 65535 / E + 1;
    return k;
}

template <typename F> static void for_hooks(Case c, F&& f) {
    for (c.hook = 0; c.hook <= 2; ++c.hook)
        for (c.finish = 0; c.finish <= 1; ++c.finish) f(c);
}

// every combination of the optional pointers x hooks, over the orders and batches at which the core routes change
static void sweep_options() {
    static const int pairs[][2] = {{196, 49}, {49, 196}, {197, 64}, {65, 665}};
    int bs[8];
    for (int E : kE) {
        const int nb = batches(E, bs);
        for (int ib = 0; ib < nb; ++ib)
            for (unsigned opts = 0; opts < 256; ++opts) {
                Case c = {E, E == 5 ? 1 : 4, bs[ib], 0, 0, 64, 64, 0, 0, 0, 0, opts, 0, 0};
                for (int n : kOrders) { c.n_s = c.n_t = n; for_hooks(c, run); }
                for (auto& p : pairs) { c.n_s = p[0]; c.n_t = p[1]; for_hooks(c, run); }
            }
    }
}

// dtypes, strides, alignment flags and feature counts (D % 8 in {0, 4}; a long teacher axis for the scratch bound of
// the stream centring) x L x E, without and with the gradients
static void sweep_layouts() {
    static const unsigned opt_set[] = {0x00, 0x03, 0x0f, 0x47};
    static const int d_t_set[] = {64, 68, 2048};
    for (int E : {1, 2, 5})
        for (int L : kL)
            for (int B : {2, 64})
                for (int n_s : kOrders)
                    for (int rel = 0; rel < 3; ++rel) {
                        const int n_t = rel == 0 ? n_s : rel == 1 ? 49 : 196;
                        if (rel && n_t == n_s) continue;
                        for (int d_s : {64, 68})
                            for (int d_t : d_t_set)
                                for (int sl = 0; sl < 6; ++sl)
                                    for (int tl = 0; tl < 6; ++tl)
                                        for (unsigned opts : opt_set) {
                                            Case c = {E, L, B, n_s, n_t, d_s, d_t, sl / 3, sl % 3, tl / 3, tl % 3, opts, 1, 1};
                                            run(c);
                                            if (opts == 0x03 && B == 2) { c.hook = 2; run(c); }
                                        }
                    }
}

// every pair of token counts x E x L x the batches around the thresholds x hooks
static void sweep_shapes() {
    int bs[8];
    for (int E : kE)
        for (int L : kL) {
            const int nb = batches(E, bs);
            for (int ib = 0; ib < nb; ++ib)
                for (int n_s : kOrders)
                    for (int n_t : kOrders)
                        for (unsigned opts : {0x00u, 0x13u, 0x2fu}) {
                            Case c = {E, L, bs[ib], n_s, n_t, 64, 512, 0, 0, 0, 0, opts, 0, 0};
                            for_hooks(c, run);
                        }
        }
}

int main(int argc, char** argv) {
    std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "plans") {
        if (!basd_procrustes_plan_query) { fprintf(stderr, "these objects have no basd_procrustes_plan_query\n"); return 2; }
        g_plans = true;
        mode = argc > 2 ? argv[2] : "options";
    }
    if (mode == "options") sweep_options();
    else if (mode == "layouts") sweep_layouts();
    else if (mode == "shapes") sweep_shapes();
    else if (mode == "one" && argc == 17) {
        // one call: E L B n_s n_t d_s d_t s_bf16 s_layout t_bf16 t_layout opts(hex) hook finish plans
        int v[15];
        for (int i = 0; i < 15; ++i) v[i] = (int)strtol(argv[2 + i], nullptr, i == 11 ? 16 : 10);
        g_plans = v[14] != 0 && basd_procrustes_plan_query;
        run(Case{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], (unsigned)v[11], v[12], v[13]});
    } else {
        fprintf(stderr, "usage: %s [plans] options | layouts | shapes | one E L B N_S N_T D_S D_T S_BF16 S_LAYOUT T_BF16 "
                        "T_LAYOUT OPTS HOOK FINISH PLANS\n", argv[0]);
        return 2;
    }
    basd_procrustes_tuning(1);
    basd_procrustes_finish_tuning(1);
    fprintf(stderr, "%s: %ld calls, %zu distinct launch sequences, %zu kernels registered\n", mode.c_str(), g_calls,
            g_distinct.size(), g_kernels.size());
    return 0;
}
