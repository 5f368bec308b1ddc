// Records what the host side of csrc/tridiag.hip launches, without a GPU and without the HIP runtime, in the manner of
// jacobi_dispatch_trace.cpp: tridiag.o is linked against the stand-ins of hip_trace_standins.h, which print the kernel
// name, grid, block and dynamic LDS bytes of every launch, every function attribute that is set, every fill and every
// event that is recorded.  Two builds -- one against the tridiag.hip of a parent commit, one against the working tree --
// run over the same sweeps must print the same bytes: that is the proof that a change to the dispatcher left the launch
// sequences alone.  (Scalar kernel arguments are not seen: those are compared by eye in the diff.)
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -c csrc/tridiag.hip -o tridiag.o
//   g++ -O1 -std=c++17 tools/tridiag_dispatch_trace.cpp tridiag.o -o tridiag_dispatch_trace
//   ./tridiag_dispatch_trace factor | vectors | queries > trace.txt           (a summary line goes to stderr)
//
// The resident budget of the shared stage is found once per order (the stand-ins answer 256 CUs with one workgroup each:
// the cap of 128) and BASD_TRIDIAG_BUDGET overrides it: smaller budgets are separate runs with that variable set.
// -DTRIDIAG_TRACE_NO_QUERY leaves out `queries`, for an object from before basd_tridiag_plan_query.
#include "hip_trace_standins.h"

// never dereferenced: the stand-ins launch nothing
static float* const kA = (float*)0x1000000;
static float* const kD = (float*)0x2000000;
static float* const kE = (float*)0x3000000;
static float* const kTau = (float*)0x4000000;
static float* const kVh = (float*)0x5000000;
static float* const kX = (float*)0x6000000;
static float* const kOut = (float*)0x7000000;
static void* const kWork = (void*)0x8000000;
static int* const kRanks = (int*)0x9000000;
static int* const kMirror = (int*)0xA000000;
static unsigned* const kGo = (unsigned*)0xB000000;
static void* const kEvent = (void*)0xC000000;

static const int kBatches[] = {1, 2, 6, 8, 9, 28, 64, 129}, kTails[] = {0, 1, 3}, kMembers[] = {0, 1, 5, 16}, kPads[] = {-1, 3};

template <class F>
static void for_each_order(F f) {
    for (int n = 2; n <= 1100; ++n) f(n);
    for (int n : {2048, 4096, 4097}) f(n);
}

// every tuning of the sweep; the reset first restores pad = -1, which no call can set
template <class F>
static void for_each_tuning(F f) {
    for (int tail : kTails)
        for (int members : kMembers)
            for (int pad : kPads) {
                if (basd_tridiag_tuning(members, pad, -1, -1, tail, 1) != 0) abort();
                f(tail, members, pad);
            }
    basd_tridiag_tuning(-1, -1, -1, -1, -1, 1);
}

// layouts of the batch: 0 = quads (aligned base, stride a multiple of 4), 1 = base off by 4 bytes, 2 = odd stride
static float* base_of(int layout) { return layout == 1 ? kA + 1 : kA; }
static long stride_of(int layout, int n) { return layout == 2 ? ((long)n * n) | 1 : ((long)n * n + 3) & ~3L; }

static void sweep_factor() {
    for_each_tuning([](int tail, int members, int pad) {
        for (int batch : kBatches)
            for_each_order([&](int n) {
                for (int layout = 0; layout < 3; ++layout) {
                    float* a = base_of(layout);
                    const long stride = stride_of(layout, n);
                    char what[160];
                    const int head = snprintf(what, sizeof what, "tail=%d members=%d pad=%d batch=%d n=%d layout=%d ", tail,
                                              members, pad, batch, n, layout);
                    auto call = [&](const char* name, int rc) {
                        snprintf(what + head, sizeof what - head, "%s", name);
                        finish_call(what, rc);
                    };
                    const int count = batch > 1 ? batch - 1 : 1;
                    call("tridiag", basd_tridiag(a, stride, n, batch, kD, kE, kTau, kVh, kWork, nullptr));
                    call("ranked", basd_tridiag_ranked(a, stride, n, batch, kD, kE, kTau, kVh, kWork, count, 2.0, n - 1,
                                                       kRanks, kMirror, nullptr, nullptr));
                    call("ranked+event", basd_tridiag_ranked(a, stride, n, batch, kD, kE, kTau, kVh, kWork, count, 2.0,
                                                             n - 1, kRanks, nullptr, kEvent, nullptr));
                    call("gated", basd_tridiag_ranked_gated(a, stride, n, batch, kD, kE, kTau, kVh, kWork, count, 2.0,
                                                            n - 1, kRanks, kMirror, kGo, 1u, 1000, nullptr));
                }
            });
    });
}

static void sweep_vectors() {
    auto orders = [](auto f) {
        for (int n = 1; n <= 1100; ++n) f(n);
        for (int n : {8192, 8193}) f(n);
    };
    for (int batch : {1, 3})
        orders([&](int n) {
            char what[96];
            auto call = [&](const char* name, int k, int rc) {
                snprintf(what, sizeof what, "batch=%d n=%d k=%d %s", batch, n, k, name);
                finish_call(what, rc);
            };
            call("eigenvalues", 0, basd_tridiag_eigenvalues(kD, kE, n, batch, kOut, nullptr));
            call("mp_rank", 0, basd_tridiag_mp_rank(kD, kE, n, batch, 2.0, n - 1, kRanks, nullptr, nullptr, kMirror, nullptr));
            call("mp_rank_rank1", 0, basd_tridiag_mp_rank_rank1(kD, kE, kX, n, batch, 64.0, 2.0, n - 1, kRanks, nullptr,
                                                                kMirror, nullptr));
            for (int k : {1, 4, 64, 65, n}) {
                call("eigenvalues_leading", k, basd_tridiag_eigenvalues_leading(kD, kE, n, k, batch, kOut, nullptr));
                call("apply_q", k, basd_tridiag_apply_q(kTau, kVh, n, k, batch, kX, kOut, k, 0, nullptr));
                call("apply_qt", k, basd_tridiag_apply_q(kTau, kVh, n, k, batch, kX, kOut, k, 1, nullptr));
                call("shifted_solve", k, basd_tridiag_shifted_solve(kD, kE, kTau, k, n, k, batch, kX, kOut, nullptr));
                call("eigenvectors", k, basd_tridiag_eigenvectors(kD, kE, kTau, kVh, kOut, n, k, batch, kX, kOut, k, nullptr));
            }
        });
}

#ifndef TRIDIAG_TRACE_NO_QUERY
static void print_queries() {
    for_each_tuning([](int tail, int members, int pad) {
        for (int batch : kBatches)
            for_each_order([&](int n) {
                printf("tail=%d members=%d pad=%d batch=%d n=%d workspace_bytes=%ld\n", tail, members, pad, batch, n,
                       basd_tridiag_workspace_bytes(n, batch));
                for (int flags = 0; flags < 8; ++flags)
                    for (int budget : {0, 16, 1}) {
                        int out[12] = {};
                        const int rc = basd_tridiag_plan_query(n, batch, flags, budget, out);
                        printf("  flags=%d budget=%d rc=%d plan", flags, budget, rc);
                        for (int v : out) printf(" %d", v);
                        printf("\n");
                        ++g_calls;
                    }
            });
    });
}
#endif

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "factor") sweep_factor();
    else if (mode == "vectors") sweep_vectors();
#ifndef TRIDIAG_TRACE_NO_QUERY
    else if (mode == "queries") print_queries();
#endif
    else {
        fprintf(stderr, "usage: %s factor | vectors | queries\n", argv[0]);
        return 2;
    }
    fprintf(stderr, "%s: %ld calls, %zu distinct launch sequences, %zu kernels registered\n", mode.c_str(), g_calls,
            g_distinct.size(), g_kernels.size());
    return 0;
}
