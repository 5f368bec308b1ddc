// Records what the host side of csrc/jacobi.hip launches, without a GPU and without the HIP runtime.
//
// jacobi.o needs eleven runtime symbols; hip_trace_standins.h supplies stand-ins for the ten that are HIP's (atexit is
// libc's), so the object links into a plain program.  The stand-ins launch nothing: they print the kernel name, grid,
// block and dynamic LDS bytes of every launch, every function attribute that is set and the byte count of every fill
// / copy.  Two builds of this program -- one against the jacobi.hip of a parent commit, one against the working tree --
// run over the same sweep of shapes must print the same bytes: that is the proof that a change to the dispatcher left
// the launch sequences alone.  (Scalar kernel arguments are not seen: those are compared by eye in the diff.)
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -c csrc/jacobi.hip -o jacobi.o
//   g++ -O1 -std=c++17 tools/jacobi_dispatch_trace.cpp jacobi.o -o jacobi_dispatch_trace
//   ./jacobi_dispatch_trace onesided | tall | twopass | queries > trace.txt      (a summary line goes to stderr)
//
// Runs of identical consecutive launches (the rounds of the block solver) are folded into one line with a count.
#include "hip_trace_standins.h"

// never dereferenced: the stand-ins launch nothing
static float* const kW = (float*)0x10000;
static float* const kColnorm = (float*)0x20000;
static int* const kFlags = (int*)0x30000;
static int* const kSweeps = (int*)0x40000;
static int* const kOrders = (int*)0x50000;
static void* const kWorkspace = (void*)0x60000;
static const int kMaxSweeps = 2;

static void onesided(int rows_dot, int rows_tot, int n, int batch, bool orders, bool with_flags, int lanes, int ordering) {
    char what[160];
    snprintf(what, sizeof what, "onesided dot=%d tot=%d n=%d batch=%d orders=%d flags=%d lanes=%d ordering=%d", rows_dot,
             rows_tot, n, batch, (int)orders, (int)with_flags, lanes, ordering);
    const int rc = basd_jacobi_onesided(kW, (long)rows_tot * n, rows_dot, rows_tot, n, batch, orders ? kOrders : nullptr,
                                        kColnorm, n, kMaxSweeps, 0.f, with_flags ? kFlags : nullptr, kSweeps, nullptr);
    finish_call(what, rc);
}

static void sweep_onesided() {
    static const int lanes_set[] = {0, 4, 8, 16}, batches[] = {1, 2, 127, 128, 255, 256, 320, 321, 1024};
    for (int lanes : lanes_set)
        for (int ordering = 0; ordering <= 1; ++ordering) {
            if (basd_jacobi_tuning(lanes) != 0 || basd_jacobi_ordering(ordering) != 0) abort();
            for (int batch : batches) {
                // plain square, past the largest order, with and without per-matrix orders
                for (int n = 1; n <= 1100; ++n)
                    for (int orders = 0; orders <= 1; ++orders) onesided(n, n, n, batch, orders, true, lanes, ordering);
                // plain rectangular
                for (int n = 1; n <= 260; ++n) {
                    const int rows[] = {n - 1, n + 7, 96, 97, 160, 161, 200, 201, 2 * n};
                    for (int r : rows)
                        if (r >= 1) onesided(r, r, n, batch, false, true, lanes, ordering);
                }
                // stacked
                for (int n = 1; n <= 640; ++n) onesided(n, 2 * n, n, batch, false, true, lanes, ordering);
                for (int n = 1; n <= 260; ++n) {
                    onesided(n + 6, 2 * n + 13, n, batch, false, true, lanes, ordering);
                    onesided(n, n + 1, n, batch, false, true, lanes, ordering);
                }
                // errors: per-matrix orders with riding rows; no flags on shapes of the block path and past it
                onesided(49, 98, 49, batch, true, true, lanes, ordering);
                onesided(300, 600, 300, batch, true, true, lanes, ordering);
                onesided(300, 300, 300, batch, false, false, lanes, ordering);
                onesided(300, 300, 300, batch, true, false, lanes, ordering);
                onesided(392, 784, 392, batch, false, false, lanes, ordering);
                onesided(1100, 1100, 1100, batch, false, false, lanes, ordering);
                onesided(49, 49, 49, batch, false, false, lanes, ordering);      // LDS routes take no flags
            }
        }
    basd_jacobi_tuning(0);
    basd_jacobi_ordering(1);
}

// long columns with few of them, short columns with many, halves of unequal length: the panel and LDS shapes that
// square-ish matrices never pick
static void sweep_tall() {
    static const int lanes_set[] = {0, 4, 8, 16}, batches[] = {1, 128, 256}, orders[] = {2, 7, 8, 40, 64, 200, 400, 1000};
    for (int lanes : lanes_set)
        for (int ordering = 0; ordering <= 1; ++ordering) {
            if (basd_jacobi_tuning(lanes) != 0 || basd_jacobi_ordering(ordering) != 0) abort();
            for (int batch : batches)
                for (int n : orders)
                    for (int dot = 1; dot <= 1030; ++dot) {
                        const int ride[] = {0, 1, dot / 3, dot, 2 * dot, 1024 - dot, 1030};
                        for (int r : ride)
                            if (r >= 0) onesided(dot, dot + r, n, batch, false, true, lanes, ordering);
                    }
        }
    basd_jacobi_tuning(0);
    basd_jacobi_ordering(1);
}

static void sweep_twopass() {
    static const int batches[] = {1, 16, 256};
    for (int batch : batches)
        for (int n = 2; n <= 260; ++n) {
            char what[96];
            snprintf(what, sizeof what, "twopass n=%d batch=%d", n, batch);
            const int rc = basd_jacobi_stacked_twopass(kW, 2L * n * n, n, batch, kColnorm, n, kMaxSweeps, 0.f, kWorkspace,
                                                       kSweeps, nullptr);
            finish_call(what, rc);
        }
}

static void print_queries() {
    for (int n = -1; n <= 1100; ++n)
        printf("n=%d plain4_fits=%d lds_square_fits=%d\n", n, basd_jacobi_plain4_fits(n), basd_jacobi_lds_square_fits(n));
    static const int batches[] = {1, 16, 256}, sweeps[] = {1, 30};
    for (int n = 0; n <= 260; ++n)
        for (int batch : batches)
            for (int s : sweeps)
                printf("n=%d batch=%d sweeps=%d twopass_workspace_bytes=%ld\n", n, batch, s,
                       basd_jacobi_twopass_workspace_bytes(n, batch, s));
    for (int batch : batches)
        for (int s : sweeps) printf("batch=%d sweeps=%d workspace_ints=%d\n", batch, s, basd_jacobi_workspace_ints(batch, s));
    printf("max_rows=%d\n", basd_jacobi_max_rows());
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "onesided") sweep_onesided();
    else if (mode == "tall") sweep_tall();
    else if (mode == "twopass") sweep_twopass();
    else if (mode == "queries") print_queries();
    else if (mode == "one" && argc == 10) {
        // one call: rows_dot rows_tot n batch orders flags lanes ordering
        int v[8];
        for (int i = 0; i < 8; ++i) v[i] = atoi(argv[2 + i]);
        if (basd_jacobi_tuning(v[6]) != 0 || basd_jacobi_ordering(v[7]) != 0) return 2;
        onesided(v[0], v[1], v[2], v[3], v[4] != 0, v[5] != 0, v[6], v[7]);
    } else {
        fprintf(stderr, "usage: %s onesided | tall | twopass | queries | one DOT TOT N BATCH ORDERS FLAGS LANES ORDERING\n", argv[0]);
        return 2;
    }
    if (g_calls) fprintf(stderr, "%s: %ld calls, %zu distinct launch sequences, %zu kernels registered\n", mode.c_str(), g_calls,
                         g_distinct.size(), g_kernels.size());
    return 0;
}
