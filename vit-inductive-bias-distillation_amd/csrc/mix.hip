// Batch preparation in ONE launch: MixUp / CutMix of a dense NCHW batch with the batch rolled by one, the conversion of
// the source (fp32, bf16, or uint8 scaled and normalised per channel) and the dense (B, K) soft-target matrix (the
// contract is in include/basd_hip.h).
//
// A streaming pass: every source byte is needed twice (as row i and as the partner of row i + 1), every destination
// byte is written once.  Work is cut into chunks of ONE image (kMixVecs vectors per lane) and walked in storage order
// by a capped grid with a grid stride, so the chunks in flight at any moment cover a few dozen consecutive images: the
// partner read of a chunk follows its first read by one image's worth of chunks and is served by the caches.  The chunks
// of the target matrix follow the image chunks in the same list.  Every scalar of the draw travels in the kernel
// arguments.  Each product and sum is rounded on its own (contraction is off): the bits are those of the same formula
// evaluated op by op in fp32.
#include "basd_common.h"
#include "../../include/basd_hip.h"

namespace basd {

constexpr int kMixBlock = 256;
constexpr int kMixMaxGrid = 2048;       // 256 CUs x 8 workgroups; the chunk list is walked with a grid stride
constexpr int kMixVecs = 2;             // vectors per lane and chunk, all loaded before the first dependent instruction
constexpr int kMixTargetChunk = kMixBlock * 4;
constexpr int kMixMaxStatChannels = BASD_MIX_MAX_STAT_CHANNELS;

enum { kMixNone = 0, kMixMixUp = 1, kMixCutMix = 2 };

typedef unsigned int v2u __attribute__((ext_vector_type(2)));
typedef unsigned int v4u __attribute__((ext_vector_type(4)));

struct MixArgs {
    const void* src;
    void* dst;
    const long* labels;     // nullptr: no targets
    float* targets;
    int B, C, H, W, K;
    int hw, chw;            // elements of a plane / of an image
    int chunks_per_image, image_items, items;
    int y1, y2, x1, x2;     // CutMix box
    float c_s, c_p;         // weights of the row itself / of its partner (MixUp)
    float t_s, t_p;         // the same for the targets
    int n_stat;             // channels with their own mean / std (uint8 source); 1 = one table for all channels
    float mean[kMixMaxStatChannels], std[kMixMaxStatChannels];
};

// elements per vector: the wider of the two element types moves 16 bytes per lane
template <typename S, typename D>
struct MixWidth {
    static constexpr int kMax = sizeof(S) > sizeof(D) ? sizeof(S) : sizeof(D);
    static constexpr int V = 16 / kMax;
};

template <int NW>
__device__ __forceinline__ void mix_load_words(const void* p, unsigned (&w)[NW]) {
    if constexpr (NW == 4) {
        const v4u r = *(const v4u*)p;
        w[0] = r[0]; w[1] = r[1]; w[2] = r[2]; w[3] = r[3];
    } else if constexpr (NW == 2) {
        const v2u r = *(const v2u*)p;
        w[0] = r[0]; w[1] = r[1];
    } else {
        w[0] = *(const unsigned*)p;
    }
}

template <int NW>
__device__ __forceinline__ void mix_store_words(void* p, const unsigned (&w)[NW]) {
    if constexpr (NW == 4) {
        *(v4u*)p = v4u{w[0], w[1], w[2], w[3]};
    } else if constexpr (NW == 2) {
        *(v2u*)p = v2u{w[0], w[1]};
    } else {
        *(unsigned*)p = w[0];
    }
}

// element e of a group of words; `lut` is the channel's 256-entry table (uint8 only)
template <typename S, int NW>
__device__ __forceinline__ float mix_get(const unsigned (&w)[NW], int e, const float* lut) {
    if constexpr (sizeof(S) == 4) {
        return __uint_as_float(w[e]);
    } else if constexpr (sizeof(S) == 2) {
        const unsigned x = w[e >> 1];
        return __uint_as_float((e & 1) ? (x & 0xffff0000u) : (x << 16));
    } else {
        return lut[(w[e >> 2] >> (8 * (e & 3))) & 255u];
    }
}

template <typename S>
__device__ __forceinline__ float mix_get_one(const S* p, const float* lut) {
    if constexpr (sizeof(S) == 4) {
        return *(const float*)p;
    } else if constexpr (sizeof(S) == 2) {
        return __uint_as_float((unsigned)*(const unsigned short*)p << 16);
    } else {
        return lut[*(const unsigned char*)p];
    }
}

// fp32 -> bf16, round to nearest even; a NaN stays a (quiet) NaN
__device__ __forceinline__ unsigned mix_bf16_bits(float f) {
    const unsigned u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

template <typename D, int V>
__device__ __forceinline__ void mix_put(D* p, const float (&o)[V]) {
    if constexpr (sizeof(D) == 4) {
        static_assert(V == 4, "an fp32 destination moves 4 elements per lane");
        const unsigned w[4] = {__float_as_uint(o[0]), __float_as_uint(o[1]), __float_as_uint(o[2]),
                               __float_as_uint(o[3])};
        mix_store_words<4>(p, w);
    } else {
        unsigned w[V / 2];
#pragma unroll
        for (int k = 0; k < V / 2; ++k) w[k] = mix_bf16_bits(o[2 * k]) | (mix_bf16_bits(o[2 * k + 1]) << 16);
        mix_store_words<V / 2>(p, w);
    }
}

template <typename D>
__device__ __forceinline__ void mix_put_one(D* p, float o) {
    if constexpr (sizeof(D) == 4) {
        *(float*)p = o;
    } else {
        *(unsigned short*)p = (unsigned short)mix_bf16_bits(o);
    }
}

// where element r of an image sits: channel, row, column
struct MixPos {
    int ch, y, x;
};

__device__ __forceinline__ MixPos mix_pos(unsigned r, const MixArgs& a) {
    MixPos p;
    p.ch = (int)(r / (unsigned)a.hw);
    const unsigned pos = r - (unsigned)p.ch * (unsigned)a.hw;
    p.y = (int)(pos / (unsigned)a.W);
    p.x = (int)(pos - (unsigned)p.y * (unsigned)a.W);
    return p;
}

__device__ __forceinline__ void mix_pos_next(MixPos& p, const MixArgs& a) {
    if (++p.x == a.W) {
        p.x = 0;
        if (++p.y == a.H) {
            p.y = 0;
            ++p.ch;
        }
    }
}

__device__ __forceinline__ bool mix_in_box(const MixPos& p, const MixArgs& a) {
    return p.y >= a.y1 && p.y < a.y2 && p.x >= a.x1 && p.x < a.x2;
}

// One fp32 operation each, rounded to nearest and never contracted with its neighbour.  (The toolchain's __fmul_rn /
// __fadd_rn are plain operators compiled under the default contraction mode: a product and a sum of theirs fuse.)
__device__ __forceinline__ float mix_mul(float x, float y) {
#pragma clang fp contract(off)
    return x * y;
}
__device__ __forceinline__ float mix_add(float x, float y) {
#pragma clang fp contract(off)
    return x + y;
}
__device__ __forceinline__ float mix_sub(float x, float y) {
#pragma clang fp contract(off)
    return x - y;
}
__device__ __forceinline__ float mix_div(float x, float y) {
#pragma clang fp contract(off)
    return x / y;
}

// One element: s = v(x_i), p = v(x_{i-1}) (read only where the kind needs it).
template <int KIND>
__device__ __forceinline__ float mix_one(float s, float p, bool in_box, const MixArgs& a) {
    if constexpr (KIND == kMixMixUp) {
        return mix_add(mix_mul(p, a.c_p), mix_mul(s, a.c_s));
    } else if constexpr (KIND == kMixCutMix) {
        return in_box ? p : s;
    } else {
        return s;
    }
}

template <typename S, typename D, int KIND>
__global__ void __launch_bounds__(kMixBlock) mix_batch_kernel(MixArgs a) {
    constexpr int V = MixWidth<S, D>::V;
    constexpr int NW = V * (int)sizeof(S) / 4;           // 32-bit words of one source vector
    constexpr int kChunk = kMixBlock * kMixVecs * V;     // elements of one image chunk
    constexpr bool kU8 = sizeof(S) == 1;
    constexpr bool kNeedPos = kU8 || KIND == kMixCutMix;
    __shared__ float lut[kU8 ? kMixMaxStatChannels * 256 : 1];
    const int tid = threadIdx.x;
    if constexpr (kU8) {
        // v(u) = ((float(u) / 255) - mean_c) / std_c with two true divisions, once per workgroup and byte value
#pragma clang fp contract(off)
        for (int c = 0; c < a.n_stat; ++c) {
            const float scaled = mix_div((float)tid, 255.0f);
            lut[c * 256 + tid] = mix_div(mix_sub(scaled, a.mean[c]), a.std[c]);
        }
        __syncthreads();
    }
    const S* src = (const S*)a.src;
    D* dst = (D*)a.dst;
    for (int it = blockIdx.x; it < a.items; it += gridDim.x) {
        if (it < a.image_items) {
            const int i = it / a.chunks_per_image;
            const int r0 = (it - i * a.chunks_per_image) * kChunk;
            const int ip = i == 0 ? a.B - 1 : i - 1;     // roll(1, 0): the partner of row i is row i - 1
            const int len = a.chw - r0 < kChunk ? a.chw - r0 : kChunk;
            const S* xs = src + (long)i * a.chw + r0;
            const S* xp = src + (long)ip * a.chw + r0;
            D* o = dst + (long)i * a.chw + r0;
            // chunk starts are multiples of the vector width: a chunk is aligned as its image is
            bool vec = (((uintptr_t)xs) % (V * sizeof(S))) == 0 && (((uintptr_t)o) % (V * sizeof(D))) == 0;
            if (KIND != kMixNone) vec = vec && (((uintptr_t)xp) % (V * sizeof(S))) == 0;
            int done = 0;
            if (vec) {
                const int nv = len / V;
                unsigned ws[kMixVecs][NW], wp[kMixVecs][NW];
                MixPos pos[kMixVecs];
                bool need[kMixVecs];
#pragma unroll
                for (int u = 0; u < kMixVecs; ++u) {
                    const int j = tid + u * kMixBlock;
                    need[u] = false;
                    if (j < nv) {
                        mix_load_words<NW>(xs + j * V, ws[u]);
                        if constexpr (kNeedPos) pos[u] = mix_pos((unsigned)(r0 + j * V), a);
                        if constexpr (KIND == kMixMixUp) need[u] = true;
                        if constexpr (KIND == kMixCutMix) {
                            MixPos q = pos[u];
#pragma unroll
                            for (int e = 0; e < V; ++e) {
                                need[u] |= mix_in_box(q, a);
                                mix_pos_next(q, a);
                            }
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < kMixVecs; ++u) {
#pragma unroll
                    for (int w = 0; w < NW; ++w) wp[u][w] = 0u;
                    if (need[u]) mix_load_words<NW>(xp + (tid + u * kMixBlock) * V, wp[u]);
                }
#pragma unroll
                for (int u = 0; u < kMixVecs; ++u) {
                    const int j = tid + u * kMixBlock;
                    if (j < nv) {
                        float out[V];
                        MixPos q = {0, 0, 0};
                        if constexpr (kNeedPos) q = pos[u];
#pragma unroll
                        for (int e = 0; e < V; ++e) {
                            const float* row = lut;
                            if constexpr (kU8) row = lut + (a.n_stat > 1 ? q.ch * 256 : 0);
                            const bool in_box = KIND == kMixCutMix && mix_in_box(q, a);
                            const float s = mix_get<S, NW>(ws[u], e, row);
                            // outside the box (or with no partner read at all) the partner's value is not used
                            const float p = KIND == kMixNone ? 0.f : mix_get<S, NW>(wp[u], e, row);
                            out[e] = mix_one<KIND>(s, p, in_box, a);
                            if constexpr (kNeedPos) mix_pos_next(q, a);
                        }
                        mix_put<D, V>(o + j * V, out);
                    }
                }
                done = nv * V;
            }
            // the last chw % V elements of an image, or all of a chunk whose rows are not aligned for the vectors
            for (int r = done + tid; r < len; r += kMixBlock) {
                MixPos q = {0, 0, 0};
                if constexpr (kNeedPos) q = mix_pos((unsigned)(r0 + r), a);
                const float* row = lut;
                if constexpr (kU8) row = lut + (a.n_stat > 1 ? q.ch * 256 : 0);
                const bool in_box = KIND == kMixCutMix && mix_in_box(q, a);
                const float s = mix_get_one<S>(xs + r, row);
                float p = 0.f;
                if (KIND == kMixMixUp || in_box) p = mix_get_one<S>(xp + r, row);
                mix_put_one<D>(o + r, mix_one<KIND>(s, p, in_box, a));
            }
        } else {
            // T[i][k] = [y_{i-1} == k] t_p + [y_i == k] t_s; a label outside [0, K) in the pair: the row is NaN
#pragma clang fp contract(off)
            const int n = a.B * a.K;
            const int e0 = (it - a.image_items) * kMixTargetChunk + tid * 4;
            float out[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                out[e] = 0.f;
                if (e0 + e < n) {
                    const int i = (e0 + e) / a.K, k = (e0 + e) - i * a.K;
                    const long yi = a.labels[i], yp = a.labels[i == 0 ? a.B - 1 : i - 1];
                    const bool ok = yi >= 0 && yi < a.K && yp >= 0 && yp < a.K;
                    const float v = mix_add(mix_mul(yp == k ? 1.f : 0.f, a.t_p), mix_mul(yi == k ? 1.f : 0.f, a.t_s));
                    out[e] = ok ? v : __builtin_nanf("");
                }
            }
            float* t = a.targets + e0;
            if (e0 + 4 <= n && (((uintptr_t)t) & 15) == 0) {
                mix_put<float, 4>(t, out);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (e0 + e < n) t[e] = out[e];
            }
        }
    }
}

template <typename S, typename D>
static int mix_launch(MixArgs a, int kind, hipStream_t stream) {
    constexpr int kChunk = kMixBlock * kMixVecs * MixWidth<S, D>::V;
    a.chunks_per_image = (a.chw + kChunk - 1) / kChunk;
    const long image_items = (long)a.B * a.chunks_per_image;
    const long target_items = a.labels ? ((long)a.B * a.K + kMixTargetChunk - 1) / kMixTargetChunk : 0;
    BASD_CHECK_ARG(image_items + target_items < (1L << 31));
    a.image_items = (int)image_items;
    a.items = (int)(image_items + target_items);
    const int grid = a.items < kMixMaxGrid ? a.items : kMixMaxGrid;
    if (kind == kMixNone) {
        mix_batch_kernel<S, D, kMixNone><<<grid, kMixBlock, 0, stream>>>(a);
    } else if (kind == kMixMixUp) {
        mix_batch_kernel<S, D, kMixMixUp><<<grid, kMixBlock, 0, stream>>>(a);
    } else {
        mix_batch_kernel<S, D, kMixCutMix><<<grid, kMixBlock, 0, stream>>>(a);
    }
    BASD_RETURN_LAST();
}

template <typename S>
static int mix_launch_dst(const MixArgs& a, int dst_dtype, int kind, hipStream_t stream) {
    if (dst_dtype == BASD_DTYPE_F32) return mix_launch<S, float>(a, kind, stream);
    return mix_launch<S, __hip_bfloat16>(a, kind, stream);
}

}  // namespace basd

extern "C" {

int basd_mix_batch(const void* src, int src_dtype, void* dst, int dst_dtype, int B, int C, int H, int W, int kind,
                   double lam, int y1, int y2, int x1, int x2, const float* mean, const float* std,
                   const long* labels, int K, double lam_targets, float* targets, hipStream_t stream) {
    BASD_CHECK_ARG(B >= 0 && C > 0 && H > 0 && W > 0);
    BASD_CHECK_ARG(kind == basd::kMixNone || kind == basd::kMixMixUp || kind == basd::kMixCutMix);
    BASD_CHECK_ARG(src_dtype == BASD_DTYPE_F32 || src_dtype == BASD_DTYPE_BF16 || src_dtype == BASD_DTYPE_U8);
    BASD_CHECK_ARG(dst_dtype == BASD_DTYPE_F32 || dst_dtype == BASD_DTYPE_BF16);
    BASD_CHECK_ARG((mean == nullptr) == (std == nullptr));
    BASD_CHECK_ARG(mean == nullptr || (src_dtype == BASD_DTYPE_U8 && C <= basd::kMixMaxStatChannels));
    BASD_CHECK_ARG(labels == nullptr || (targets != nullptr && K > 0));
    const long chw = (long)C * H * W;
    // 32-bit element indices inside an image and inside the target matrix, with a chunk of headroom
    BASD_CHECK_ARG(chw < (1L << 30) && (long)B * (labels ? K : 1) < (1L << 30));
    if (kind == basd::kMixCutMix) BASD_CHECK_ARG(0 <= y1 && y1 <= y2 && y2 <= H && 0 <= x1 && x1 <= x2 && x2 <= W);
    if (B == 0) return BASD_OK;
    BASD_CHECK_ARG(src && dst);
    const long ss = src_dtype == BASD_DTYPE_F32 ? 4 : src_dtype == BASD_DTYPE_BF16 ? 2 : 1;
    const long ds = dst_dtype == BASD_DTYPE_F32 ? 4 : 2;
    const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (uintptr_t)(B * chw * ss);
    const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + (uintptr_t)(B * chw * ds);
    BASD_CHECK_ARG(s1 <= d0 || d1 <= s0);                  // row i reads the ORIGINAL row i - 1
    basd::MixArgs a = {};
    a.src = src; a.dst = dst; a.labels = labels; a.targets = targets;
    a.B = B; a.C = C; a.H = H; a.W = W; a.K = labels ? K : 0;
    a.hw = H * W; a.chw = (int)chw;
    a.y1 = y1; a.y2 = y2; a.x1 = x1; a.x2 = x2;
    a.c_s = (float)lam; a.c_p = (float)(1.0 - lam);
    a.t_s = (float)lam_targets; a.t_p = (float)(1.0 - lam_targets);
    a.n_stat = mean ? C : 1;
    for (int c = 0; c < basd::kMixMaxStatChannels; ++c) {
        a.mean[c] = mean && c < C ? mean[c] : 0.f;
        a.std[c] = std && c < C ? std[c] : 1.f;
    }
    if (src_dtype == BASD_DTYPE_F32) return basd::mix_launch_dst<float>(a, dst_dtype, kind, stream);
    if (src_dtype == BASD_DTYPE_BF16) return basd::mix_launch_dst<__hip_bfloat16>(a, dst_dtype, kind, stream);
    return basd::mix_launch_dst<unsigned char>(a, dst_dtype, kind, stream);
}

}  // extern "C"
