// The teacher side of a single-layer teacher, kept per dataset image: rows of three cache arrays (the fp64 Gram of the
// centred, weighted teacher tokens on the core grid, omega, omega_t) scattered from / gathered into the places one
// Procrustes call writes / reads them.  Plain copies, one launch each way; every offset is formed in 64 bits (a cache
// of ImageNet-1k at 49 tokens is 24.6 GB of Grams: row * n * n * 8 passes 2^32 after 223,000 rows).
#include "basd_common.h"
#include "../../include/basd_hip.h"

namespace basd {

constexpr int TCC_THREADS = 256;
constexpr int TCC_PER_THREAD = 4;      // 16-byte (or 8-byte) elements of the Gram per thread and grid-stride pass
constexpr int TCC_MAX_GROUPS = 32;     // workgroups per row at most

// grid (groups per row, B).  GATHER: cache row index[b] -> call row b (a repeated index only reads a row twice);
// otherwise call row b -> cache row index[b] (equal indices in one launch race; the caller hands over equal rows for
// them, so every interleaving leaves the same bytes).  An index outside [0, capacity) copies nothing.
template <bool GATHER, typename V>
__global__ void __launch_bounds__(TCC_THREADS) teacher_cache_copy_kernel(
    const V* __restrict__ src_g, const float* __restrict__ src_omega, const float* __restrict__ src_omega_t,
    const long* __restrict__ index, long capacity, long g_row /* elements of V per Gram */, int n_s, int n,
    V* __restrict__ dst_g, float* __restrict__ dst_omega, float* __restrict__ dst_omega_t) {
    const long b = blockIdx.y;
    const long row = index[b];
    if (row < 0 || row >= capacity) return;
    const long rs = GATHER ? row : b, rd = GATHER ? b : row;
    const V* sg = src_g + rs * g_row;
    V* dg = dst_g + rd * g_row;
    const long step = (long)gridDim.x * TCC_THREADS;
    for (long i = (long)blockIdx.x * TCC_THREADS + threadIdx.x; i < g_row; i += step) dg[i] = sg[i];
    if (blockIdx.x == gridDim.x - 1) {          // the group with the shortest share of the Gram
        const float* so = src_omega + rs * n_s;
        float* dout = dst_omega + rd * n_s;
        for (int i = threadIdx.x; i < n_s; i += TCC_THREADS) dout[i] = so[i];
        const float* st = src_omega_t + rs * n;
        float* dt = dst_omega_t + rd * n;
        for (int i = threadIdx.x; i < n; i += TCC_THREADS) dt[i] = st[i];
    }
}

template <bool GATHER>
static int teacher_cache_copy(const double* src_g, const float* src_omega, const float* src_omega_t, const long* index,
                              int B, int n, int n_s, long capacity, double* dst_g, float* dst_omega, float* dst_omega_t,
                              hipStream_t stream) {
    BASD_CHECK_ARG(src_g && src_omega && src_omega_t && index && dst_g && dst_omega && dst_omega_t);
    BASD_CHECK_ARG(B > 0 && B <= 65535 && n > 0 && n_s > 0 && n <= 32768 && capacity > 0);
    const long nn = (long)n * n;
    // rows of an even number of doubles behind 16-byte aligned bases start on 16 bytes: copied as 16-byte pairs
    const bool pairs = nn % 2 == 0 && (((uintptr_t)src_g | (uintptr_t)dst_g) & 15) == 0;
    const long g_row = pairs ? nn / 2 : nn;
    const long per_group = (long)TCC_THREADS * TCC_PER_THREAD;
    long groups = (g_row + per_group - 1) / per_group;
    groups = groups < 1 ? 1 : groups > TCC_MAX_GROUPS ? TCC_MAX_GROUPS : groups;
    const dim3 grid((unsigned)groups, (unsigned)B);
    if (pairs)
        teacher_cache_copy_kernel<GATHER, double2><<<grid, TCC_THREADS, 0, stream>>>(
            (const double2*)src_g, src_omega, src_omega_t, index, capacity, g_row, n_s, n, (double2*)dst_g, dst_omega,
            dst_omega_t);
    else
        teacher_cache_copy_kernel<GATHER, double><<<grid, TCC_THREADS, 0, stream>>>(
            src_g, src_omega, src_omega_t, index, capacity, g_row, n_s, n, dst_g, dst_omega, dst_omega_t);
    BASD_RETURN_LAST();
}

}  // namespace basd

extern "C" {

int basd_teacher_cache_store(const double* g, const float* omega, const float* omega_t, const long* index, int B, int n,
                             int n_s, long capacity, double* cache_g, float* cache_omega, float* cache_omega_t,
                             hipStream_t stream) {
    return basd::teacher_cache_copy<false>(g, omega, omega_t, index, B, n, n_s, capacity, cache_g, cache_omega,
                                           cache_omega_t, stream);
}

int basd_teacher_cache_load(const double* cache_g, const float* cache_omega, const float* cache_omega_t,
                            const long* index, int B, int n, int n_s, long capacity, double* g, float* omega,
                            float* omega_t, hipStream_t stream) {
    return basd::teacher_cache_copy<true>(cache_g, cache_omega, cache_omega_t, index, B, n, n_s, capacity, g, omega,
                                          omega_t, stream);
}

}  // extern "C"
