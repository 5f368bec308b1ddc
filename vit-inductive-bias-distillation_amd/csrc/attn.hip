// Teacher attention importance straight from the output of a block's own fused qkv projection, in ONE launch (the
// contract is in include/basd_hip.h): out[b, h, :] is the CLS query's softmax row, or the mean over all queries of the
// softmax rows, of softmax(scale * Q K^T).  Nothing of size N^2 is written anywhere.
//
// One workgroup of 4 waves owns one (b, h).  A softmax row needs its maximum and its sum before its probabilities can
// be added to the column sums, so the 32 x 32 score tiles are computed twice:
//   pass 1  every wave owns 32 queries (their fragments stay in registers) and streams the keys through LDS; the tile
//           comes out of the matrix core as C[key][query] with the QUERY on the lane and 16 keys in the registers, so
//           the running (max, sum) of a query is lane-private; the two lane halves are merged once at the end and
//           (max, 1 / sum) of every query goes to LDS;
//   pass 2  every wave owns 32 keys and streams the queries; the same tile, the same k order, hence the same bits;
//           p = exp(s - max) / sum is added to 16 lane-private column sums, which are reduced over the 32 query lanes
//           once per key tile and stored.
// The key / query axis that is streamed is cut into chunks that fit the staging buffer (N = 1025 at fp32 does not fit
// LDS whole).  All reductions run in a fixed order and there are no atomics: the bits depend on the arguments only.
// Rows reach LDS through 16-byte loads where the view's address and strides allow, element by element otherwise; the
// contraction is padded with zeros to the MFMA's k (bf16: 16).  A NaN in a score reaches the sum of its softmax row
// (fmaxf drops it from the maximum, exp keeps it), and with it every column of out[b, h, :] -- and nothing else.
#include "basd_common.h"
#include "../../include/basd_hip.h"

namespace basd {

typedef float attn_f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 attn_bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int attn_v4u __attribute__((ext_vector_type(4)));

constexpr int kAttnBlock = 256;
constexpr int kAttnWaves = kAttnBlock / kWave;
constexpr int kAttnTile = 32;                         // the MFMA tile: 32 keys x 32 queries
constexpr int kAttnMaxN = 1025;
constexpr int kAttnMaxHd = 128;
constexpr int kAttnRowPad = 16;                       // bytes between rows of the staging buffer
constexpr int kAttnStageBytes = 72 * 1024;            // >= 128 rows at hd = 128, fp32
constexpr float kAttnLowest = -3.402823466e+38f;      // start of a running maximum: finite, so exp(m - m') is defined

struct AttnArgs {
    const void* qkv;
    long sb, sn;
    int N, H, hd, nq;        // nq: queries that count (1: the CLS row, N: the mean over queries)
    float scale;
    float* out;
    int chunk_rows;          // rows of the staging buffer (a multiple of 32)
    int ldb;                 // bytes per row of the staging buffer
    int vec;                 // 16-byte global loads are aligned
};

// s = acc * scale as ONE rounded product in both passes (never fused into the subtraction that follows)
__device__ __forceinline__ float attn_score(float acc, float scale) {
#pragma clang fp contract(off)
    return acc * scale;
}

// Every lane of each half of 32 lanes ends with its half's total; all 64 lanes must be active.
__device__ __forceinline__ float attn_half32_allsum(float x) {
    x = row16_allsum(x);
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// rows [row0, row0 + rows) of one operand (n valid rows of hd elements, row stride sn) -> the staging buffer; rows
// past n are zeros
template <typename T>
__device__ __forceinline__ void attn_stage(char* buf, const AttnArgs& a, const T* base, int row0, int rows, int n) {
    constexpr int EPU = 16 / (int)sizeof(T);          // elements of a 16-byte unit
    const int upr = a.hd / EPU;
    const int total = rows * upr;
    for (int u = threadIdx.x; u < total; u += kAttnBlock) {
        const int row = u / upr, c = u - row * upr;
        const int grow = row0 + row;
        attn_v4u v = {0u, 0u, 0u, 0u};
        if (grow < n) {
            const T* p = base + (long)grow * a.sn + c * EPU;
            if (a.vec) {
                v = *(const attn_v4u*)p;
            } else if constexpr (sizeof(T) == 4) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = ((const unsigned*)p)[e];
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const unsigned lo = ((const unsigned short*)p)[2 * e], hi = ((const unsigned short*)p)[2 * e + 1];
                    v[e] = lo | (hi << 16);
                }
            }
        }
        *(attn_v4u*)(buf + (long)row * a.ldb + c * 16) = v;
    }
}

// The lane's 16-byte unit of k-step s of its row: unit 2 s + h, zeros where the contraction is padded.
template <typename T>
__device__ __forceinline__ attn_v4u attn_unit(const char* row, int s, int h, int hd) {
    constexpr int EPU = 16 / (int)sizeof(T);
    const int u = 2 * s + h;
    attn_v4u v = {0u, 0u, 0u, 0u};
    if (u * EPU < hd) v = *(const attn_v4u*)(row + u * 16);
    return v;
}

template <typename T>
__device__ __forceinline__ attn_f32x16 attn_mma(attn_v4u a, attn_v4u b, attn_f32x16 c) {
    if constexpr (sizeof(T) == 2) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(attn_bf16x8, a),
                                                       __builtin_bit_cast(attn_bf16x8, b), c, 0, 0, 0);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a[e]), __uint_as_float(b[e]), c, 0, 0, 0);
        return c;
    }
}

// PASS 1: owned = queries, streamed = keys, writes (max, 1 / sum) per query to LDS.
// PASS 2: owned = keys, streamed = queries, writes out[b, h, key].
template <typename T, int NS, int PASS>
__device__ __forceinline__ void attn_pass(const AttnArgs& a, const T* own_base, int n_own, const T* str_base,
                                          int n_str, char* buf, float* m_s, float* il_s, float* out_row) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int tiles_own = (n_own + kAttnTile - 1) / kAttnTile;
    const float neg_inf = -__builtin_inff();
    for (int g0 = 0; g0 < tiles_own; g0 += kAttnWaves) {
        const int grp_tiles = tiles_own - g0 < kAttnWaves ? tiles_own - g0 : kAttnWaves;
        __syncthreads();
        attn_stage<T>(buf, a, own_base, g0 * kAttnTile, grp_tiles * kAttnTile, n_own);
        __syncthreads();
        const bool active = wave < grp_tiles;            // wave-uniform
        attn_v4u own[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            own[s] = attn_v4u{0u, 0u, 0u, 0u};
            if (active) own[s] = attn_unit<T>(buf + (long)(wave * kAttnTile + r) * a.ldb, s, h, a.hd);
        }
        float m = kAttnLowest, l = 0.f;                  // PASS 1: the lane's query over the lane half's keys
        float col[16];                                   // PASS 2: column sums of the 16 keys of the lane half
#pragma unroll
        for (int i = 0; i < 16; ++i) col[i] = 0.f;
        for (int c0 = 0; c0 < n_str; c0 += a.chunk_rows) {
            const int left = (n_str - c0 + kAttnTile - 1) & ~(kAttnTile - 1);
            const int rows = left < a.chunk_rows ? left : a.chunk_rows;
            __syncthreads();
            attn_stage<T>(buf, a, str_base, c0, rows, n_str);
            __syncthreads();
            if (!active) continue;
            for (int t0 = 0; t0 < rows; t0 += kAttnTile) {
                const char* srow = buf + (long)(t0 + r) * a.ldb;
                attn_f32x16 acc;
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    if (s * 32 < a.hd * (int)sizeof(T)) {
                        const attn_v4u st = attn_unit<T>(srow, s, h, a.hd);
                        // C[row = key][col = query]: the keys are the A operand in both passes
                        acc = PASS == 1 ? attn_mma<T>(st, own[s], acc) : attn_mma<T>(own[s], st, acc);
                    }
                }
                if constexpr (PASS == 1) {
                    float sv[16], tmax = neg_inf;
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int key = c0 + t0 + (i & 3) + 8 * (i >> 2) + 4 * h;
                        sv[i] = key < n_str ? attn_score(acc[i], a.scale) : neg_inf;
                        tmax = fmaxf(tmax, sv[i]);
                    }
                    const float m_new = fmaxf(m, tmax);
                    l *= __expf(m - m_new);
#pragma unroll
                    for (int i = 0; i < 16; ++i) l += __expf(sv[i] - m_new);
                    m = m_new;
                } else {
                    const int qi = c0 + t0 + r;
                    const float mq = m_s[qi], ilq = il_s[qi];
                    const bool counts = qi < n_str;
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const float p = __expf(attn_score(acc[i], a.scale) - mq) * ilq;
                        col[i] += counts ? p : 0.f;
                    }
                }
            }
        }
        if (!active) continue;
        if constexpr (PASS == 1) {
            // merge the two lane halves (they hold the same query over disjoint keys), in a fixed order
            const float m_o = __shfl_xor(m, 32, kWave), l_o = __shfl_xor(l, 32, kWave);
            const float m_lo = h == 0 ? m : m_o, m_hi = h == 0 ? m_o : m;
            const float l_lo = h == 0 ? l : l_o, l_hi = h == 0 ? l_o : l;
            const float mm = fmaxf(m_lo, m_hi);
            const float ll = l_lo * __expf(m_lo - mm) + l_hi * __expf(m_hi - mm);
            if (h == 0) {
                const int qi = (g0 + wave) * kAttnTile + r;
                m_s[qi] = mm;
                il_s[qi] = 1.0f / ll;
            }
        } else {
            const float nq = (float)n_str;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float tot = attn_half32_allsum(col[i]);
                const int key = (g0 + wave) * kAttnTile + (i & 3) + 8 * (i >> 2) + 4 * h;
                if (r == 0 && key < n_own) out_row[key] = tot / nq;
            }
        }
    }
}

template <typename T, int HDB>
__global__ void __launch_bounds__(kAttnBlock) attn_importance_kernel(AttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) char attn_smem[];
    constexpr int NS = HDB * (int)sizeof(T) / 32;        // k-steps of 32 bytes per row: 16 bf16 or 8 fp32
    const int nqp = (a.nq + kAttnTile - 1) & ~(kAttnTile - 1);
    float* m_s = (float*)attn_smem;
    float* il_s = m_s + nqp;
    char* buf = (char*)(il_s + nqp);
    const int b = blockIdx.x / a.H, hh = blockIdx.x - b * a.H;
    const T* q = (const T*)a.qkv + (long)b * a.sb + (long)hh * a.hd;      // last axis: [3][H][hd]
    const T* k = q + (long)a.H * a.hd;
    float* out_row = a.out + (long)blockIdx.x * a.N;
    attn_pass<T, NS, 1>(a, q, a.nq, k, a.N, buf, m_s, il_s, out_row);
    attn_pass<T, NS, 2>(a, k, a.N, q, a.nq, buf, m_s, il_s, out_row);    // opens with a barrier: the statistics are in
}

template <typename T, int HDB>
static int attn_launch(const AttnArgs& a, int B, size_t lds, hipStream_t stream) {
    if (lds > 48 * 1024)
        (void)hipFuncSetAttribute((const void*)attn_importance_kernel<T, HDB>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
    attn_importance_kernel<T, HDB><<<B * a.H, kAttnBlock, lds, stream>>>(a);
    BASD_RETURN_LAST();
}

template <typename T>
static int attn_launch_hd(const AttnArgs& a, int B, size_t lds, hipStream_t stream) {
    if (a.hd <= 32) return attn_launch<T, 32>(a, B, lds, stream);
    if (a.hd <= 64) return attn_launch<T, 64>(a, B, lds, stream);
    if (a.hd <= 96) return attn_launch<T, 96>(a, B, lds, stream);
    return attn_launch<T, 128>(a, B, lds, stream);
}

}  // namespace basd

extern "C" {

int basd_attn_importance(const void* qkv, int dtype, long sb, long sn, int B, int N, int H, int hd, int mode,
                         float scale, float* out, hipStream_t stream) {
    BASD_CHECK_ARG(qkv && out && B >= 1 && H >= 1 && N >= 1 && hd >= 1);
    BASD_CHECK_ARG(dtype == BASD_DTYPE_F32 || dtype == BASD_DTYPE_BF16);
    BASD_CHECK_ARG(mode == BASD_ATTN_CLS_ROW || mode == BASD_ATTN_QUERY_MEAN);
    BASD_CHECK_ARG((long)B * H < (1L << 31));
    if (N > basd::kAttnMaxN || hd > basd::kAttnMaxHd || hd % 8 != 0) return BASD_EUNSUPPORTED;
    const int es = dtype == BASD_DTYPE_F32 ? 4 : 2;
    basd::AttnArgs a = {};
    a.qkv = qkv; a.sb = sb; a.sn = sn;
    a.N = N; a.H = H; a.hd = hd;
    a.nq = mode == BASD_ATTN_CLS_ROW ? 1 : N;
    a.scale = scale; a.out = out;
    a.ldb = hd * es + basd::kAttnRowPad;
    const int cap = (basd::kAttnStageBytes / a.ldb) & ~(basd::kAttnTile - 1);
    const int n32 = (N + basd::kAttnTile - 1) & ~(basd::kAttnTile - 1);
    a.chunk_rows = n32 < cap ? n32 : cap;
    a.vec = ((uintptr_t)qkv % 16 == 0) && (sb * es % 16 == 0) && (sn * es % 16 == 0);
    const int nqp = (a.nq + basd::kAttnTile - 1) & ~(basd::kAttnTile - 1);
    const size_t lds = (size_t)2 * nqp * sizeof(float) + (size_t)a.chunk_rows * a.ldb;
    if (dtype == BASD_DTYPE_F32) return basd::attn_launch_hd<float>(a, B, lds, stream);
    return basd::attn_launch_hd<__hip_bfloat16>(a, B, lds, stream);
}

}  // extern "C"
