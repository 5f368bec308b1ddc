// Schedule-free AdamW (Defazio et al., "The Road Less Scheduled"; the form the schedulefree package ships as
// AdamWScheduleFree) over ALL tensors of ALL parameter groups in one launch, and the train <-> eval interpolation.
//
// A streaming pass: per element 4 fp32 reads (y, z, v, grad) and 3 writes (y, z, v), 4 writes when the gradient is
// zeroed in the same pass -- 28 / 32 bytes, no reuse.  Work is cut into chunks of kChunk elements of ONE tensor
// (chunk list on the device: tensor index, chunk index inside the tensor); a capped grid walks the list with a
// grid stride.  Per-group coefficients travel in the kernel arguments, so a step needs no host-to-device copy.
// Opt-in: global-norm clipping and a non-finite guard, as a norm pass plus the same update behind a prologue.
#include <atomic>

#include "basd_common.h"
#include "../../include/basd_hip.h"

namespace basd {

constexpr int kSfChunk = 4096;          // elements per chunk: 256 lanes x 4 x float4
constexpr int kSfBlock = 256;
constexpr int kSfMaxGrid = 2048;        // 256 CUs x 8 workgroups; the chunk list is walked with a grid stride
constexpr int kSfMaxGroups = BASD_SFADAMW_MAX_GROUPS;

typedef float v4f __attribute__((ext_vector_type(4)));
typedef BASD_GLOBAL_AS float gf32;
typedef BASD_GLOBAL_AS v4f gv4f;

// what the update needs of one parameter group, derived on the host in fp64 and rounded once
struct SfCoef {
    float lr, ckp1, bc2, beta2, omb2, eps, wd, ycoef;     // omb2 = 1 - beta2, ycoef = lr * (beta1 * (1 - ckp1) - 1)
};
struct SfCoefs {
    SfCoef g[kSfMaxGroups];
};

// One element.  Contraction is off and every path (16-byte, scalar gradient, scalar) goes through this function:
// which path a tensor takes depends on its addresses only, never on its values.
__device__ __forceinline__ void sf_update(float& y, float& z, float& v, float graw, float gscale, const SfCoef& c) {
#pragma clang fp contract(off)
    const float g = graw * gscale;
    v = c.beta2 * v + (c.omb2 * g) * g;
    const float gn = g / (sqrtf(v / c.bc2) + c.eps) + c.wd * y;      // decay taken at y, before y moves
    y = y + c.ckp1 * (z - y);
    y = y + c.ycoef * gn;
    z = z - c.lr * gn;
}

__device__ __forceinline__ void sf_update4(v4f& y, v4f& z, v4f& v, const v4f& g, float gscale, const SfCoef& c) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float yy = y[j], zz = z[j], vv = v[j];
        sf_update(yy, zz, vv, g[j], gscale, c);
        y[j] = yy; z[j] = zz; v[j] = vv;
    }
}

__device__ __forceinline__ v4f sf_load_grad4(const gf32* g, int i, bool gvec) {
    if (gvec) return ((const gv4f*)g)[i];
    v4f r;                                   // a FlatGradBucket view at an element offset that is no multiple of 4
    r[0] = g[4 * i]; r[1] = g[4 * i + 1]; r[2] = g[4 * i + 2]; r[3] = g[4 * i + 3];
    return r;
}

__device__ __forceinline__ void sf_zero_grad4(gf32* g, int i, bool gvec) {
    if (gvec) {
        ((gv4f*)g)[i] = v4f{0.f, 0.f, 0.f, 0.f};
    } else {
        g[4 * i] = 0.f; g[4 * i + 1] = 0.f; g[4 * i + 2] = 0.f; g[4 * i + 3] = 0.f;
    }
}

__global__ void __launch_bounds__(kSfBlock) sfadamw_step_kernel(const BasdSfAdamwTensor* __restrict__ table,
                                                                const int* __restrict__ chunks, int n_chunks,
                                                                SfCoefs coefs, float gscale, int zero_grad) {
    const int tid = threadIdx.x;
    for (int ci = blockIdx.x; ci < n_chunks; ci += gridDim.x) {
        const int ti = chunks[2 * ci];
        const long base = (long)chunks[2 * ci + 1] * kSfChunk;
        const BasdSfAdamwTensor t = table[ti];
        if (t.grad == nullptr) continue;                     // no gradient this step: the tensor is left alone
        const long rest = t.numel - base;
        const int len = rest < kSfChunk ? (int)rest : kSfChunk;
        gf32* y = (gf32*)t.y + base;
        gf32* z = (gf32*)t.z + base;
        gf32* v = (gf32*)t.v + base;
        gf32* g = (gf32*)t.grad + base;
        const SfCoef c = coefs.g[t.group];
        // chunk starts are multiples of 16 KB inside a tensor: a chunk is aligned as its tensor is
        const bool vec = ((((uintptr_t)y) | ((uintptr_t)z) | ((uintptr_t)v)) & 15) == 0;
        const bool gvec = (((uintptr_t)g) & 15) == 0;
        int done = 0;
        if (vec) {
            const int n4 = len >> 2;
            int i = tid;
            // two float4 per lane and tensor in flight before the first dependent instruction
            for (; i + kSfBlock < n4; i += 2 * kSfBlock) {
                const int i1 = i + kSfBlock;
                v4f y0 = ((gv4f*)y)[i], y1 = ((gv4f*)y)[i1];
                v4f z0 = ((gv4f*)z)[i], z1 = ((gv4f*)z)[i1];
                v4f v0 = ((gv4f*)v)[i], v1 = ((gv4f*)v)[i1];
                const v4f g0 = sf_load_grad4(g, i, gvec), g1 = sf_load_grad4(g, i1, gvec);
                sf_update4(y0, z0, v0, g0, gscale, c);
                sf_update4(y1, z1, v1, g1, gscale, c);
                ((gv4f*)y)[i] = y0; ((gv4f*)y)[i1] = y1;
                ((gv4f*)z)[i] = z0; ((gv4f*)z)[i1] = z1;
                ((gv4f*)v)[i] = v0; ((gv4f*)v)[i1] = v1;
                if (zero_grad) { sf_zero_grad4(g, i, gvec); sf_zero_grad4(g, i1, gvec); }
            }
            if (i < n4) {
                v4f y0 = ((gv4f*)y)[i], z0 = ((gv4f*)z)[i], v0 = ((gv4f*)v)[i];
                const v4f g0 = sf_load_grad4(g, i, gvec);
                sf_update4(y0, z0, v0, g0, gscale, c);
                ((gv4f*)y)[i] = y0; ((gv4f*)z)[i] = z0; ((gv4f*)v)[i] = v0;
                if (zero_grad) sf_zero_grad4(g, i, gvec);
            }
            done = n4 << 2;
        }
        // the last numel % 4 elements of a tensor, or all of a chunk whose y / z / v are not 16-byte aligned
        for (int i = done + tid; i < len; i += kSfBlock) {
            float yy = y[i], zz = z[i], vv = v[i];
            sf_update(yy, zz, vv, g[i], gscale, c);
            y[i] = yy; z[i] = zz; v[i] = vv;
            if (zero_grad) g[i] = 0.f;
        }
    }
}

struct SfWeights {
    float w[kSfMaxGroups];
};

// p <- p + w (z - p) for every tensor of the table, w per group (y -> x: w = 1 - 1 / beta1, x -> y: w = 1 - beta1)
__global__ void __launch_bounds__(kSfBlock) sfadamw_swap_kernel(const BasdSfAdamwTensor* __restrict__ table,
                                                                const int* __restrict__ chunks, int n_chunks,
                                                                SfWeights weights) {
    const int tid = threadIdx.x;
    for (int ci = blockIdx.x; ci < n_chunks; ci += gridDim.x) {
        const int ti = chunks[2 * ci];
        const long base = (long)chunks[2 * ci + 1] * kSfChunk;
        const BasdSfAdamwTensor t = table[ti];
        const long rest = t.numel - base;
        const int len = rest < kSfChunk ? (int)rest : kSfChunk;
        gf32* y = (gf32*)t.y + base;
        const gf32* z = (const gf32*)t.z + base;
        const float w = weights.w[t.group];
        int done = 0;
        if (((((uintptr_t)y) | ((uintptr_t)z)) & 15) == 0) {
            const int n4 = len >> 2;
            for (int i = tid; i < n4; i += kSfBlock) {
#pragma clang fp contract(off)
                const v4f p = ((gv4f*)y)[i], q = ((const gv4f*)z)[i];
                ((gv4f*)y)[i] = p + w * (q - p);
            }
            done = n4 << 2;
        }
        for (int i = done + tid; i < len; i += kSfBlock) {
#pragma clang fp contract(off)
            const float p = y[i];
            y[i] = p + w * (z[i] - p);
        }
    }
}

// ---- global-norm clipping and the non-finite guard ---------------------------------------------------------------
// Two launches: the norm pass leaves one fp64 partial per workgroup, the clipped step sums them in its prologue (the
// launch boundary is the only synchronisation: no ticket, no flag, no spin).

constexpr int kSfMaxParts = 1024;       // 8 KB of partials, read by every workgroup of the clipped step

// Sum of squares of the gradients.  The square of an fp32 value is exact in fp64; all terms are >= 0, so n additions
// in any order stay within n 2^-53 relative.  block_sum is a fixed order: same gradients, same bits.
__global__ void __launch_bounds__(kSfBlock) grad_sqnorm_kernel(const BasdSfAdamwTensor* __restrict__ table,
                                                               const int* __restrict__ chunks, int n_chunks,
                                                               double* __restrict__ partials) {
    __shared__ double red[32];
    const int tid = threadIdx.x;
    double acc = 0.;
    for (int ci = blockIdx.x; ci < n_chunks; ci += gridDim.x) {
        const int ti = chunks[2 * ci];
        const long base = (long)chunks[2 * ci + 1] * kSfChunk;
        const BasdSfAdamwTensor t = table[ti];
        if (t.grad == nullptr) continue;
        const long rest = t.numel - base;
        const int len = rest < kSfChunk ? (int)rest : kSfChunk;
        const gf32* g = (const gf32*)t.grad + base;
        int done = 0;
        if ((((uintptr_t)g) & 15) == 0) {
            const int n4 = len >> 2;
#pragma unroll 4
            for (int i = tid; i < n4; i += kSfBlock) {
                const v4f q = ((const gv4f*)g)[i];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc += (double)q[j] * (double)q[j];
            }
            done = n4 << 2;
        }
        // the last numel % 4 elements of a tensor, or all of a chunk whose gradient is not 16-byte aligned
#pragma unroll 4
        for (int i = done + tid; i < len; i += kSfBlock) {
            const double q = (double)g[i];
            acc += q * q;
        }
    }
    const double s = block_sum(acc, red);
    if (tid == 0) partials[blockIdx.x] = s;
}

// sfadamw_step_kernel's walk behind a prologue that turns the partials into (gradient scale, skip).  The per-element
// code is sf_update: with the same effective scale the bytes are those of sfadamw_step_kernel.
__global__ void __launch_bounds__(kSfBlock) sfadamw_step_clipped_kernel(
    const BasdSfAdamwTensor* __restrict__ table, const int* __restrict__ chunks, int n_chunks, SfCoefs coefs,
    float grad_scale, int zero_grad, const double* __restrict__ partials, int n_partials, double max_norm,
    int skip_nonfinite, BasdGradVerdict* __restrict__ verdict) {
    __shared__ double red[32];
    const int tid = threadIdx.x;
    // every workgroup: lane t takes partials t, t + 256, ..., then block_sum -- one order, the same bits everywhere
    double part = 0.;
    for (int i = tid; i < n_partials; i += kSfBlock) part += partials[i];
    const double norm_sq = block_sum(part, red);
    const double norm = fabs((double)grad_scale) * sqrt(norm_sq);
    double c = 1.;
    if (max_norm > 0.) {
        const double q = max_norm / (norm + 1e-6);
        if (q < 1.) c = q;
    }
    const float coef = (float)c;
    const bool skip = skip_nonfinite && !__builtin_isfinite(norm_sq);
    if (blockIdx.x == 0 && tid == 0) {
        verdict->norm_sq = norm_sq;
        verdict->norm = (float)norm;
        verdict->coef = coef;
        verdict->skipped = skip ? 1 : 0;
        verdict->skipped_total += skip ? 1 : 0;
    }
    if (skip && !zero_grad) return;
    const float gscale = grad_scale * coef;                 // one fp32 rounding of the exact product

    for (int ci = blockIdx.x; ci < n_chunks; ci += gridDim.x) {
        const int ti = chunks[2 * ci];
        const long base = (long)chunks[2 * ci + 1] * kSfChunk;
        const BasdSfAdamwTensor t = table[ti];
        if (t.grad == nullptr) continue;
        const long rest = t.numel - base;
        const int len = rest < kSfChunk ? (int)rest : kSfChunk;
        gf32* g = (gf32*)t.grad + base;
        const bool gvec = (((uintptr_t)g) & 15) == 0;
        if (skip) {                                          // y, z, v stay as they are; a NaN must not stay in a bucket
            const int n4 = gvec ? len >> 2 : 0;
            for (int i = tid; i < n4; i += kSfBlock) sf_zero_grad4(g, i, true);
            for (int i = (n4 << 2) + tid; i < len; i += kSfBlock) g[i] = 0.f;
            continue;
        }
        gf32* y = (gf32*)t.y + base;
        gf32* z = (gf32*)t.z + base;
        gf32* v = (gf32*)t.v + base;
        const SfCoef c = coefs.g[t.group];
        const bool vec = ((((uintptr_t)y) | ((uintptr_t)z) | ((uintptr_t)v)) & 15) == 0;
        int done = 0;
        if (vec) {
            const int n4 = len >> 2;
            int i = tid;
            for (; i + kSfBlock < n4; i += 2 * kSfBlock) {
                const int i1 = i + kSfBlock;
                v4f y0 = ((gv4f*)y)[i], y1 = ((gv4f*)y)[i1];
                v4f z0 = ((gv4f*)z)[i], z1 = ((gv4f*)z)[i1];
                v4f v0 = ((gv4f*)v)[i], v1 = ((gv4f*)v)[i1];
                const v4f g0 = sf_load_grad4(g, i, gvec), g1 = sf_load_grad4(g, i1, gvec);
                sf_update4(y0, z0, v0, g0, gscale, c);
                sf_update4(y1, z1, v1, g1, gscale, c);
                ((gv4f*)y)[i] = y0; ((gv4f*)y)[i1] = y1;
                ((gv4f*)z)[i] = z0; ((gv4f*)z)[i1] = z1;
                ((gv4f*)v)[i] = v0; ((gv4f*)v)[i1] = v1;
                if (zero_grad) { sf_zero_grad4(g, i, gvec); sf_zero_grad4(g, i1, gvec); }
            }
            if (i < n4) {
                v4f y0 = ((gv4f*)y)[i], z0 = ((gv4f*)z)[i], v0 = ((gv4f*)v)[i];
                const v4f g0 = sf_load_grad4(g, i, gvec);
                sf_update4(y0, z0, v0, g0, gscale, c);
                ((gv4f*)y)[i] = y0; ((gv4f*)z)[i] = z0; ((gv4f*)v)[i] = v0;
                if (zero_grad) sf_zero_grad4(g, i, gvec);
            }
            done = n4 << 2;
        }
        for (int i = done + tid; i < len; i += kSfBlock) {
            float yy = y[i], zz = z[i], vv = v[i];
            sf_update(yy, zz, vv, g[i], gscale, c);
            y[i] = yy; z[i] = zz; v[i] = vv;
            if (zero_grad) g[i] = 0.f;
        }
    }
}

// BasdSfAdamwGroup (host, fp64) -> what the kernels take; false = a group the update cannot run with
static bool sf_make_coefs(const BasdSfAdamwGroup* groups, int n_groups, SfCoefs& coefs) {
    for (int i = 0; i < n_groups; ++i) {
        const BasdSfAdamwGroup& s = groups[i];
        if (!(s.bias_correction2 > 0. && s.eps >= 0.)) return false;
        SfCoef& c = coefs.g[i];
        c.lr = (float)s.lr;
        c.ckp1 = (float)s.ckp1;
        c.bc2 = (float)s.bias_correction2;
        c.beta2 = (float)s.beta2;
        c.omb2 = (float)(1. - s.beta2);
        c.eps = (float)s.eps;
        c.wd = (float)s.weight_decay;
        c.ycoef = (float)(s.lr * (s.beta1 * (1. - s.ckp1) - 1.));
    }
    return true;
}

static std::atomic<long> g_sf_launches{0};

}  // namespace basd

extern "C" {

int basd_sfadamw_chunk(void) { return basd::kSfChunk; }

long basd_sfadamw_launches(void) { return basd::g_sf_launches.load(); }

int basd_sfadamw_step(const BasdSfAdamwTensor* table, const int* chunks, int n_chunks, const BasdSfAdamwGroup* groups,
                      int n_groups, float grad_scale, int zero_grad, hipStream_t stream) {
    BASD_CHECK_ARG(n_chunks >= 0 && groups && n_groups >= 1 && n_groups <= basd::kSfMaxGroups);
    if (n_chunks == 0) return BASD_OK;
    BASD_CHECK_ARG(table && chunks);
    basd::SfCoefs coefs = {};
    for (int i = 0; i < n_groups; ++i) {
        const BasdSfAdamwGroup& s = groups[i];
        BASD_CHECK_ARG(s.bias_correction2 > 0. && s.eps >= 0.);
        basd::SfCoef& c = coefs.g[i];
        c.lr = (float)s.lr;
        c.ckp1 = (float)s.ckp1;
        c.bc2 = (float)s.bias_correction2;
        c.beta2 = (float)s.beta2;
        c.omb2 = (float)(1. - s.beta2);
        c.eps = (float)s.eps;
        c.wd = (float)s.weight_decay;
        c.ycoef = (float)(s.lr * (s.beta1 * (1. - s.ckp1) - 1.));
    }
    const int grid = n_chunks < basd::kSfMaxGrid ? n_chunks : basd::kSfMaxGrid;
    basd::sfadamw_step_kernel<<<grid, basd::kSfBlock, 0, stream>>>(table, chunks, n_chunks, coefs, grad_scale,
                                                                  zero_grad != 0);
    basd::g_sf_launches.fetch_add(1);
    BASD_RETURN_LAST();
}

int basd_sfadamw_swap(const BasdSfAdamwTensor* table, const int* chunks, int n_chunks, const float* weights,
                      int n_groups, hipStream_t stream) {
    BASD_CHECK_ARG(n_chunks >= 0 && weights && n_groups >= 1 && n_groups <= basd::kSfMaxGroups);
    if (n_chunks == 0) return BASD_OK;
    BASD_CHECK_ARG(table && chunks);
    basd::SfWeights w = {};
    for (int i = 0; i < n_groups; ++i) w.w[i] = weights[i];
    const int grid = n_chunks < basd::kSfMaxGrid ? n_chunks : basd::kSfMaxGrid;
    basd::sfadamw_swap_kernel<<<grid, basd::kSfBlock, 0, stream>>>(table, chunks, n_chunks, w);
    basd::g_sf_launches.fetch_add(1);
    BASD_RETURN_LAST();
}

int basd_grad_sqnorm_parts(int n_chunks) {
    return n_chunks < 1 ? 1 : n_chunks < basd::kSfMaxParts ? n_chunks : basd::kSfMaxParts;
}

int basd_grad_sqnorm(const BasdSfAdamwTensor* table, const int* chunks, int n_chunks, double* partials, int n_partials,
                     hipStream_t stream) {
    BASD_CHECK_ARG(n_chunks >= 0 && n_partials == basd_grad_sqnorm_parts(n_chunks));
    BASD_CHECK_ARG(partials && (((uintptr_t)partials) & 7) == 0);
    if (n_chunks == 0) return BASD_OK;
    BASD_CHECK_ARG(table && chunks);
    basd::grad_sqnorm_kernel<<<n_partials, basd::kSfBlock, 0, stream>>>(table, chunks, n_chunks, partials);
    basd::g_sf_launches.fetch_add(1);
    BASD_RETURN_LAST();
}

int basd_sfadamw_step_clipped(const BasdSfAdamwTensor* table, const int* chunks, int n_chunks,
                              const BasdSfAdamwGroup* groups, int n_groups, float grad_scale, int zero_grad,
                              const double* partials, int n_partials, double max_norm, int skip_nonfinite,
                              BasdGradVerdict* verdict, hipStream_t stream) {
    BASD_CHECK_ARG(n_chunks >= 0 && groups && n_groups >= 1 && n_groups <= basd::kSfMaxGroups);
    BASD_CHECK_ARG(n_partials == basd_grad_sqnorm_parts(n_chunks) && !(max_norm != max_norm));
    BASD_CHECK_ARG(partials && (((uintptr_t)partials) & 7) == 0 && verdict && (((uintptr_t)verdict) & 7) == 0);
    if (n_chunks == 0) return BASD_OK;
    BASD_CHECK_ARG(table && chunks);
    basd::SfCoefs coefs = {};
    BASD_CHECK_ARG(basd::sf_make_coefs(groups, n_groups, coefs));
    const int grid = n_chunks < basd::kSfMaxGrid ? n_chunks : basd::kSfMaxGrid;
    basd::sfadamw_step_clipped_kernel<<<grid, basd::kSfBlock, 0, stream>>>(table, chunks, n_chunks, coefs, grad_scale,
                                                                          zero_grad != 0, partials, n_partials,
                                                                          max_norm, skip_nonfinite != 0, verdict);
    basd::g_sf_launches.fetch_add(1);
    BASD_RETURN_LAST();
}

}  // extern "C"
