// Opt-in residual check of the tridiagonal factorisations (specification: include/basd_hip.h; arithmetic:
// tridiag_check_core.h).  Two launches around basd_tridiag* -- no kernel of tridiag.hip is touched:
//   tridiag_probe_kernel  one pass over A before it is destroyed: x, y = A x, tr A and |A|_F^2 per block of rows;
//   tridiag_check_kernel  one workgroup per matrix: fp64 sums over d, e and T (Q^T x), the three ratios, the verdict.
// Between them the caller runs basd_tridiag_apply_q on the probe's two rows.
#include "basd_common.h"
#include "tridiag_check_core.h"
#include "../../include/basd_hip.h"

namespace basd {

constexpr int kProbeRows = BASD_TRIDIAG_PROBE_ROWS;      // per workgroup: 4 waves x 4 rows
constexpr int kProbeCols = 16;                           // columns per lane: 64 x 16 = BASD_TRIDIAG_CHECK_MAX_N
static_assert(kProbeRows % 4 == 0, "a wave takes every fourth row of its block");
static_assert(64 * kProbeCols == BASD_TRIDIAG_CHECK_MAX_N, "a lane holds the signs of all its columns");

// grid = (ceil(n / kProbeRows), batch), block = 256.  A wave takes one row at a time; a lane reads its columns of the
// row (VEC: four 16-byte groups 256 columns apart, else sixteen single columns 64 apart), accumulates y_i and the row's
// share of |A|_F^2 in fp64 in ascending column order, and the wave folds the lanes by a fixed butterfly.  Wave w of
// the block then holds rows w, w + 4, ...; thread 0 adds the kProbeRows row sums in row order.  Nothing depends on
// which workgroup runs first, so two calls leave the same bits.  The signs of a lane's columns are the same for every
// row: they are hashed once.
template <bool VEC>
__global__ void __launch_bounds__(256) tridiag_probe_kernel(const float* __restrict__ a, long a_batch_stride, int n,
                                                            float* __restrict__ xy, double* __restrict__ parts,
                                                            unsigned* __restrict__ ctl) {
    const int z = blockIdx.y, blk = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __shared__ double s_tr[kProbeRows], s_f[kProbeRows];
    if (blk == 0 && z == 0 && threadIdx.x < kTridiagCtlWords) ctl[threadIdx.x] = tridiag_ctl_initial(threadIdx.x);
    const float* az = a + (long)z * a_batch_stride;
    float sx[kProbeCols];
#pragma unroll
    for (int c = 0; c < kProbeCols; ++c) {
        const int col = VEC ? 4 * lane + 256 * (c >> 2) + (c & 3) : lane + 64 * c;
        sx[c] = col < n ? basd_tridiag_probe_sign((uint32_t)z, (uint32_t)col) : 0.f;
    }
#pragma unroll
    for (int k = 0; k < kProbeRows / 4; ++k) {
        const int r = wave + 4 * k, row = blk * kProbeRows + r;
        if (row >= n) {                                   // wave-uniform
            if (lane == 0) s_tr[r] = 0.0, s_f[r] = 0.0;
            continue;
        }
        const float* ar = az + (long)row * n;
        double y = 0.0, f = 0.0, dg = 0.0;
        if (VEC) {
#pragma unroll
            for (int g = 0; g < kProbeCols / 4; ++g) {
                const int col = 4 * lane + 256 * g;
                if (col < n) {                            // n % 4 == 0: the whole group is inside the row
                    const float4 v = *reinterpret_cast<const float4*>(ar + col);
                    const float q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        tridiag_probe_term(q[t], sx[4 * g + t], y, f);
                        if (col + t == row) dg = (double)q[t];
                    }
                }
            }
        } else {
#pragma unroll
            for (int c = 0; c < kProbeCols; ++c) {
                const int col = lane + 64 * c;
                if (col < n) {
                    const float v = ar[col];
                    tridiag_probe_term(v, sx[c], y, f);
                    if (col == row) dg = (double)v;
                }
            }
        }
        y = wave_sum(y);
        f = wave_sum(f);
        dg = wave_sum(dg);                                // one lane holds A(i, i), the others 0
        if (lane == 0) {
            xy[((long)z * 2 + 0) * n + row] = basd_tridiag_probe_sign((uint32_t)z, (uint32_t)row);
            xy[((long)z * 2 + 1) * n + row] = (float)y;
            s_tr[r] = dg;
            s_f[r] = f;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double tr = 0.0, f = 0.0;
        for (int r = 0; r < kProbeRows; ++r) tr += s_tr[r], f += s_f[r];
        double* p = parts + ((long)z * gridDim.x + blk) * 2;
        p[0] = tr;
        p[1] = f;
    }
}

struct TridiagCheckArgs {
    const float* d;
    const float* e;
    const float* uv;          // (batch, 2, n): Q^T x, Q^T y
    const double* parts;      // (batch, n_parts, 2)
    double* sums;             // (batch, 2)
    unsigned* ctl;
    float* ratios_out;
    int* verdict_out;
    int* host_mirror;         // nullable
    float thr[3];
    int n, batch, n_parts;
};

// grid = batch, block = 256.  The ratios of one matrix; thread 0 then adds the matrix to the batch's verdict through
// integer atomics on the control words (sums, minima and maxima of integers: the same result in any order), and the
// workgroup that arrives last writes the verdict out and puts the control words back for the next check.
__global__ void __launch_bounds__(256) tridiag_check_kernel(const TridiagCheckArgs p) {
    const int z = blockIdx.x, tid = threadIdx.x, n = p.n;
    __shared__ double scratch[32];
    const float* d = p.d + (long)z * n;
    const float* e = p.e + (long)z * n;
    const float* u = p.uv + (long)z * 2 * n;
    double sd = 0.0, sd2 = 0.0, se2 = 0.0, r2 = 0.0;
    for (int i = tid; i < n; i += 256) {
        const double di = (double)d[i];
        sd += di;
        sd2 += di * di;
        if (i + 1 < n) se2 += (double)e[i] * (double)e[i];
        const double r = tridiag_residual_term(d, e, u, u + n, n, i);
        r2 += r * r;
    }
    sd = block_sum(sd, scratch);
    sd2 = block_sum(sd2, scratch);
    se2 = block_sum(se2, scratch);
    r2 = block_sum(r2, scratch);
    if (tid != 0) return;
    double tr = 0.0, fro2 = 0.0;
    for (int b = 0; b < p.n_parts; ++b) {
        tr += p.parts[((long)z * p.n_parts + b) * 2];
        fro2 += p.parts[((long)z * p.n_parts + b) * 2 + 1];
    }
    p.sums[2 * z] = tr;
    p.sums[2 * z + 1] = fro2;
    double rho[3];
    tridiag_check_ratios(sd, sd2, se2, r2, tr, fro2, n, rho);
    const int mask = tridiag_check_mask(rho, p.thr);
    for (int k = 0; k < 3; ++k) {
        const float rk = (float)rho[k];
        p.ratios_out[3 * z + k] = rk;
        atomicMax(&p.ctl[4 + k], __float_as_uint(rk));          // ratios are >= 0 or NaN: NaN patterns sort above +inf
    }
    if (mask) {
        atomicAdd(&p.ctl[1], 1u);
        atomicMin(&p.ctl[2], (unsigned)z);
        atomicOr(&p.ctl[3], (unsigned)mask);
    }
    const unsigned arrived = __hip_atomic_fetch_add(&p.ctl[0], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (arrived != (unsigned)p.batch - 1u) return;
    unsigned w[kTridiagCtlWords];
    for (int k = 0; k < kTridiagCtlWords; ++k) w[k] = __hip_atomic_load(&p.ctl[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int verdict[BASD_TRIDIAG_VERDICT_INTS] = {(int)w[1], w[2] == kTridiagNoFirst ? -1 : (int)w[2], (int)w[3], p.batch,
                                              (int)w[4], (int)w[5], (int)w[6], 0};
    for (int k = 0; k < BASD_TRIDIAG_VERDICT_INTS; ++k) {
        p.verdict_out[k] = verdict[k];
        if (p.host_mirror) p.host_mirror[k] = verdict[k];
    }
    for (int k = 0; k < kTridiagCtlWords; ++k)
        __hip_atomic_store(&p.ctl[k], tridiag_ctl_initial(k), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace basd

using namespace basd;

extern "C" {

long basd_tridiag_probe_bytes(int n, int batch) {
    if (n < 1 || n > BASD_TRIDIAG_CHECK_MAX_N || batch < 1) return 0;
    return tridiag_probe_layout(n, batch).bytes;
}

int basd_tridiag_probe(const float* a, long a_batch_stride, int n, int batch, void* probe, hipStream_t stream) {
    BASD_CHECK_ARG(a && probe && n >= 1 && batch >= 1 && batch <= 65535 && a_batch_stride >= (long)n * n);
    BASD_CHECK_ARG((((uintptr_t)probe) & 15) == 0 && (((uintptr_t)a) & 3) == 0);
    if (n > BASD_TRIDIAG_CHECK_MAX_N) return BASD_EUNSUPPORTED;
    const TridiagProbeLayout l = tridiag_probe_layout(n, batch);
    char* base = (char*)probe;
    float* xy = (float*)base;
    double* parts = (double*)(base + l.parts);
    unsigned* ctl = (unsigned*)(base + l.ctl);
    const dim3 grid(l.n_parts, batch);
    const bool vec = n % 4 == 0 && a_batch_stride % 4 == 0 && (((uintptr_t)a) & 15) == 0;
    if (vec) tridiag_probe_kernel<true><<<grid, 256, 0, stream>>>(a, a_batch_stride, n, xy, parts, ctl);
    else tridiag_probe_kernel<false><<<grid, 256, 0, stream>>>(a, a_batch_stride, n, xy, parts, ctl);
    BASD_RETURN_LAST();
}

int basd_tridiag_check(const float* d, const float* e, const float* tau, const float* vh, int n, int batch,
                       void* probe, const float* work, const float* thresholds, float* ratios_out, int* verdict_out,
                       int* host_mirror, hipStream_t stream) {
    BASD_CHECK_ARG(d && e && tau && vh && probe && ratios_out && verdict_out && n >= 1 && batch >= 1 && batch <= 65535);
    BASD_CHECK_ARG((((uintptr_t)probe) & 15) == 0 && (work || n == 1));
    if (n > BASD_TRIDIAG_CHECK_MAX_N) return BASD_EUNSUPPORTED;
    const TridiagProbeLayout l = tridiag_probe_layout(n, batch);
    char* base = (char*)probe;
    TridiagCheckArgs p;
    p.d = d;
    p.e = e;
    p.uv = work ? work : (const float*)base;
    p.parts = (const double*)(base + l.parts);
    p.sums = (double*)(base + l.sums);
    p.ctl = (unsigned*)(base + l.ctl);
    p.ratios_out = ratios_out;
    p.verdict_out = verdict_out;
    p.host_mirror = host_mirror;
    if (thresholds) {
        for (int k = 0; k < 3; ++k) {
            BASD_CHECK_ARG(thresholds[k] >= 0.f);         // false for a NaN too
            p.thr[k] = thresholds[k];
        }
    } else {
        tridiag_check_default_thresholds(n, p.thr);
    }
    p.n = n;
    p.batch = batch;
    p.n_parts = l.n_parts;
    tridiag_check_kernel<<<batch, 256, 0, stream>>>(p);
    BASD_RETURN_LAST();
}

}  // extern "C"
