// TrivialAugmentWide and the horizontal flip for dense uint8 NCHW batches in ONE launch (the contract and the
// specification of every operation are in include/basd_hip.h).
//
// One workgroup of 16 waves per image; the op of an image is uniform over its workgroup, so the dispatch on it costs no
// divergence.  Three phases, each skipped where the op does not need it:
//   load    the image is read once with 16-byte loads behind a byte-wise head (as stats.hip cuts a segment) and staged
//           in LDS when it fits (C H W <= BASD_TAUG_STAGE_BYTES: 3 x 224 x 224 is the largest); AutoContrast and
//           Equalize take the per-channel histogram on the way, by LDS integer atomics into one of four copies (by wave)
//           with runs of equal neighbours inside a lane's 16 bytes added at once: a constant image makes one add per
//           lane.  The flip changes none of the statistics, so this phase does not look at it.
//   tables  minimum / maximum from the histogram, the grey sum (Contrast) as an exact integer reduction, then one
//           256-entry table per channel for Brightness, Contrast, Posterize, Solarize, AutoContrast and Equalize.
//   write   every output byte is computed from source pixels read through ONE accessor -- from LDS, or from global
//           memory (L2-hot: the second read) for an image above the budget -- which applies the flip to the column; 16
//           bytes per lane and store where the destination is aligned, single bytes for its head and tail.
// Every fp32 / fp64 product and sum is rounded on its own (contraction is off).
#include "basd_common.h"
#include "../../include/basd_hip.h"

namespace basd {

constexpr int kTaugBlock = 1024;
constexpr int kTaugHistCopies = 4;                                    // wave w adds into copy w mod 4
constexpr int kTaugHistWords = 3 * 256;
constexpr int kTaugLutOff = kTaugHistCopies * kTaugHistWords * 4;     // 12288
constexpr int kTaugMiscOff = kTaugLutOff + 3 * 256;                   // 13056: the grey sum (8 B), lo[3], hi[3]
constexpr int kTaugImageOff = kTaugMiscOff + 64;                      // 13120, a multiple of 16
constexpr int kTaugStageBytes = BASD_TAUG_STAGE_BYTES;
// the staged image keeps its address mod 16 (up to 15 bytes in front of it): 13120 + 16 + 150528 = 163664 <= 163840
constexpr int kTaugMaxLds = kTaugImageOff + 16 + kTaugStageBytes;
static_assert(kTaugMaxLds <= 160 * 1024, "one workgroup may declare at most 160 KiB of LDS");
static_assert(sizeof(BasdTaugRecord) == 64, "the record table has 64-byte rows");

typedef unsigned int v4u __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

struct TaugArgs {
    const unsigned char* src;
    unsigned char* dst;
    const BasdTaugRecord* table;
    int* status;
    int C, H, W, hw, chw;
    int staged;
};

// the source image of a workgroup: LDS (staged) or global memory; px applies the flip
struct TaugSrc {
    const unsigned char* g;
    const unsigned char* l;
    int staged, W, hw, flip;
    __device__ __forceinline__ unsigned raw(int i) const { return staged ? l[i] : g[i]; }
    __device__ __forceinline__ unsigned px(int c, int y, int x) const {
        return raw(c * hw + y * W + (flip ? W - 1 - x : x));
    }
};

__device__ __forceinline__ unsigned taug_grey(unsigned r, unsigned g, unsigned b) {
    return (19595u * r + 38470u * g + 7471u * b + 32768u) >> 16;
}

// blend(a = degenerate, b = image, f): t = float(a) + f * float(b - a), one product and one sum
__device__ __forceinline__ unsigned taug_blend(unsigned a, unsigned b, float f, bool unit) {
#pragma clang fp contract(off)
    const float prod = f * (float)((int)b - (int)a);
    const float t = (float)(int)a + prod;
    if (unit) return (unsigned)(int)t & 255u;                          // 0 <= f <= 1: t stays inside [0, 255]
    return t <= 0.f ? 0u : t >= 255.f ? 255u : (unsigned)(int)t;
}

__device__ __forceinline__ double taug_coord(double a0, double a1, double a2, double xc, double yc) {
#pragma clang fp contract(off)
    const double p0 = a0 * xc;
    const double p1 = a1 * yc;
    const double s = p0 + p1;
    return s + a2;
}

// ops 0-5: the nearest source pixel under the inverse affine map, 0 outside the image
struct TaugGeo {
    TaugSrc s;
    double a[6];
    int H;
    __device__ __forceinline__ unsigned operator()(int c, int y, int x) const {
        const double xc = (double)x + 0.5, yc = (double)y + 0.5;
        const double fx = taug_coord(a[0], a[1], a[2], xc, yc);
        const double fy = taug_coord(a[3], a[4], a[5], xc, yc);
        // floor(f) in [0, n)  <=>  0 <= f < n; there the conversion truncates as floor does
        if (!(fx >= 0.0 && fx < (double)s.W && fy >= 0.0 && fy < (double)H)) return 0u;
        return s.px(c, (int)fy, (int)fx);
    }
};

struct TaugLut {
    TaugSrc s;
    const unsigned char* lut;
    __device__ __forceinline__ unsigned operator()(int c, int y, int x) const { return lut[c * 256 + s.px(c, y, x)]; }
};

struct TaugColor {
    TaugSrc s;
    float f;
    bool unit, rgb;
    __device__ __forceinline__ unsigned operator()(int c, int y, int x) {
        if (!rgb) return s.px(c, y, x);
        const unsigned r = s.px(0, y, x), g = s.px(1, y, x), b = s.px(2, y, x);
        return taug_blend(taug_grey(r, g, b), c == 0 ? r : c == 1 ? g : b, f, unit);
    }
};

// The write pass walks a row from left to right, so the 3 x 3 window slides: the functor keeps the window's last two
// columns (as the fp32 values the sum takes) and reads one new column per byte, three LDS reads instead of ten.
struct TaugSharp {
    TaugSrc s;
    float f;
    bool unit;
    int H;
    int lc, ly, lx;                                                    // where the kept columns belong; lx < 0: nowhere
    float left[3], mid[3], right[3];
    __device__ __forceinline__ void column(int c, int y, int x, float (&q)[3]) const {
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) q[dy] = (float)(int)s.px(c, y + dy - 1, x);
    }
    __device__ __forceinline__ unsigned operator()(int c, int y, int x) {
#pragma clang fp contract(off)
        if (y < 1 || y >= H - 1 || s.W < 3) {                          // the one-pixel border is copied: blend(p, p) = p
            lx = -2;
            return s.px(c, y, x);
        }
        if (lx >= 0 && c == lc && y == ly && x == lx + 1) {
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) left[dy] = mid[dy], mid[dy] = right[dy];
        } else {
            if (x >= 1) column(c, y, x - 1, left);
            column(c, y, x, mid);
        }
        if (x + 1 < s.W) column(c, y, x + 1, right);
        lc = c, ly = y, lx = x;
        const unsigned p = (unsigned)(int)mid[1];
        unsigned smooth = p;
        if (x >= 1 && x < s.W - 1) {
            const float k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f;
            float acc = 0.5f;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
                float prod = left[dy] * k1;
                acc = acc + prod;
                prod = mid[dy] * (dy == 1 ? k5 : k1);
                acc = acc + prod;
                prod = right[dy] * k1;
                acc = acc + prod;
            }
            smooth = acc >= 255.f ? 255u : (unsigned)(int)acc;          // acc >= 0.5
        }
        return taug_blend(smooth, p, f, unit);
    }
};

// every output byte once: a byte-wise head up to the destination's first 16-byte boundary, 16-byte stores, a tail
template <typename F>
__device__ __forceinline__ void taug_write(unsigned char* d, const TaugArgs& a, F f) {
    const int tid = threadIdx.x;
    const int to_boundary = (int)((0 - (uintptr_t)d) & 15);
    const int hd = to_boundary < a.chw ? to_boundary : a.chw;
    const int nvec = (a.chw - hd) >> 4;
    for (int v = tid; v < nvec; v += kTaugBlock) {
        const int i0 = hd + 16 * v;
        int c = i0 / a.hw;
        const int r = i0 - c * a.hw;
        int y = r / a.W;
        int x = r - y * a.W;
        unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            w[k >> 2] |= (f(c, y, x) & 255u) << (8 * (k & 3));
            if (++x == a.W) {
                x = 0;
                if (++y == a.H) {
                    y = 0;
                    ++c;
                }
            }
        }
        *(v4u*)(d + i0) = v4u{w[0], w[1], w[2], w[3]};
    }
    const int tail0 = hd + 16 * nvec;
    const int loose = hd + (a.chw - tail0);                            // fewer than 32 bytes
    if (tid < loose) {
        const int i = tid < hd ? tid : tail0 + (tid - hd);
        const int c = i / a.hw;
        const int r = i - c * a.hw;
        const int y = r / a.W;
        d[i] = (unsigned char)f(c, y, r - y * a.W);
    }
}

__global__ void __launch_bounds__(kTaugBlock) trivial_augment_kernel(TaugArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned* hist = (unsigned*)smem;
    unsigned char* lut = smem + kTaugLutOff;
    u64* grey_sum = (u64*)(smem + kTaugMiscOff);
    int* lohi = (int*)(smem + kTaugMiscOff + 8);                       // lo[3], hi[3]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int img = blockIdx.x;
    const BasdTaugRecord* rec = a.table + img;
    int op = __builtin_amdgcn_readfirstlane(rec->op);
    const bool known = op >= BASD_TAUG_IDENTITY && op <= BASD_TAUG_EQUALIZE;
    if (!known) {
        // an op code outside the table: the (flipped) image is copied and the status word says so
        if (tid == 0) atomicOr(a.status, 1);
        op = BASD_TAUG_IDENTITY;
    }
    const unsigned char* s = a.src + (long)img * a.chw;
    unsigned char* d = a.dst + (long)img * a.chw;
    const int pad = (int)((uintptr_t)s & 15);
    unsigned char* limg = smem + kTaugImageOff + pad;                  // limg + i is aligned as s + i is
    const bool need_hist = op == BASD_TAUG_AUTOCONTRAST || op == BASD_TAUG_EQUALIZE;
    const bool need_grey = op == BASD_TAUG_CONTRAST;

    if (need_hist) {
        for (int i = tid; i < kTaugHistCopies * kTaugHistWords; i += kTaugBlock) hist[i] = 0u;
    }
    if (need_grey && tid == 0) *grey_sum = 0;
    if (need_hist || need_grey) __syncthreads();

    // ---- load: stage and / or count
    if (a.staged || need_hist) {
        const int to_boundary = (16 - pad) & 15;
        const int h = to_boundary < a.chw ? to_boundary : a.chw;
        const int nvec = (a.chw - h) >> 4;
        unsigned* mine = hist + (wid & (kTaugHistCopies - 1)) * kTaugHistWords;
        for (int v = tid; v < nvec; v += kTaugBlock) {
            const int i0 = h + 16 * v;
            const v4u w = *(const v4u*)(s + i0);
            if (a.staged) *(v4u*)(limg + i0) = w;
            if (need_hist) {
                int c = i0 / a.hw;
                int next = (c + 1) * a.hw;                             // first byte of the next plane
                unsigned key = 0u, count = 0u;
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    if (i0 + k == next) {
                        ++c;
                        next += a.hw;
                    }
                    const unsigned here = (unsigned)c * 256u + ((w[k >> 2] >> (8 * (k & 3))) & 255u);
                    if (k == 0 || here == key) {
                        key = here;
                        ++count;
                    } else {
                        atomicAdd(mine + key, count);
                        key = here;
                        count = 1u;
                    }
                }
                atomicAdd(mine + key, count);
            }
        }
        const int tail0 = h + 16 * nvec;
        const int loose = h + (a.chw - tail0);                         // fewer than 32 bytes
        if (tid < loose) {
            const int i = tid < h ? tid : tail0 + (tid - h);
            const unsigned b = s[i];
            if (a.staged) limg[i] = (unsigned char)b;
            if (need_hist) atomicAdd(mine + (unsigned)(i / a.hw) * 256u + b, 1u);
        }
        __syncthreads();
    }

    TaugSrc src;
    src.g = s;
    src.l = limg;
    src.staged = a.staged;
    src.W = a.W;
    src.hw = a.hw;
    src.flip = __builtin_amdgcn_readfirstlane(rec->flip != 0);

    // ---- tables
    if (need_hist) {
        if (tid < kTaugHistWords)
            hist[tid] = hist[tid] + hist[kTaugHistWords + tid] + hist[2 * kTaugHistWords + tid] +
                        hist[3 * kTaugHistWords + tid];
        __syncthreads();
        if (wid < a.C) {
            int lo = 256, hi = -1;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int bin = 4 * lane + k;
                if (hist[wid * 256 + bin] != 0u) {
                    lo = lo < bin ? lo : bin;
                    hi = hi > bin ? hi : bin;
                }
            }
            for (int m = 32; m > 0; m >>= 1) {
                const int olo = __shfl_xor(lo, m, kWave), ohi = __shfl_xor(hi, m, kWave);
                lo = lo < olo ? lo : olo;
                hi = hi > ohi ? hi : ohi;
            }
            if (lane == 0) {
                lohi[wid] = lo;
                lohi[3 + wid] = hi;
            }
        }
        __syncthreads();
    }
    if (need_grey) {
        unsigned part = 0u;                                            // at most 2^20 pixels of 255 per thread
        for (int p = tid; p < a.hw; p += kTaugBlock)
            part += a.C == 3 ? taug_grey(src.raw(p), src.raw(a.hw + p), src.raw(2 * a.hw + p)) : src.raw(p);
        const u64 total = group_sum((u64)part, kWave);
        if (lane == 0) __hip_atomic_fetch_add(grey_sum, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __syncthreads();
    }
    const float farg = rec->farg;
    const bool unit = farg >= 0.f && farg <= 1.f;
    const bool table_op = op == BASD_TAUG_BRIGHTNESS || op == BASD_TAUG_CONTRAST || op == BASD_TAUG_POSTERIZE ||
                          op == BASD_TAUG_SOLARIZE || need_hist;
    if (table_op) {
        if (tid < 256 * a.C) {
            const int c = tid >> 8;
            const unsigned v = (unsigned)tid & 255u;
            unsigned o = v;
            if (op == BASD_TAUG_BRIGHTNESS) {
                o = taug_blend(0u, v, farg, unit);
            } else if (op == BASD_TAUG_CONTRAST) {
                // floor(sum / n + 0.5) = (2 sum + n) div 2 n: the quotient is at least 1 / 2n away from the next integer,
                // far more than an fp64 rounding
                const u64 n = (u64)a.hw;
                const unsigned mean = (unsigned)((2 * *grey_sum + n) / (2 * n));
                o = taug_blend(mean, v, farg, unit);
            } else if (op == BASD_TAUG_POSTERIZE) {
                const int bits = rec->iarg < 0 ? 0 : rec->iarg > 8 ? 8 : rec->iarg;
                o = v & (0xFFu << (8 - bits)) & 255u;
            } else if (op == BASD_TAUG_SOLARIZE) {
                o = (float)(int)v < farg ? v : 255u - v;
            } else {
                const int lo = lohi[c], hi = lohi[3 + c];
                if (op == BASD_TAUG_AUTOCONTRAST) {
                    if (hi > lo) {
#pragma clang fp contract(off)
                        const double scale = 255.0 / (double)(hi - lo);
                        const double offset = (double)(-lo) * scale;
                        const double prod = (double)(int)v * scale;
                        const double t = prod + offset;
                        const int q = (int)t;
                        o = q < 0 ? 0u : q > 255 ? 255u : (unsigned)q;
                    }
                } else if (hi > lo) {
                    const unsigned step = ((unsigned)a.hw - hist[c * 256 + hi]) / 255u;
                    if (step != 0u) {
                        unsigned n = step / 2u;
                        for (unsigned j = 0; j < v; ++j) n += hist[c * 256 + j];
                        const unsigned q = n / step;
                        o = q > 255u ? 255u : q;
                    }
                }
            }
            lut[tid] = (unsigned char)o;
        }
        __syncthreads();
    }

    // ---- write
    if (table_op) {
        TaugLut f = {src, lut};
        taug_write(d, a, f);
    } else if (op == BASD_TAUG_COLOR) {
        TaugColor f = {src, farg, unit, a.C == 3};
        taug_write(d, a, f);
    } else if (op == BASD_TAUG_SHARPNESS) {
        TaugSharp f;
        f.s = src;
        f.f = farg;
        f.unit = unit;
        f.H = a.H;
        f.lc = f.ly = 0;
        f.lx = -2;
        taug_write(d, a, f);
    } else {
        TaugGeo f;
        f.s = src;
        f.H = a.H;
#pragma unroll
        for (int k = 0; k < 6; ++k) f.a[k] = known ? rec->a[k] : (k == 0 || k == 4 ? 1.0 : 0.0);
        taug_write(d, a, f);
    }
}

}  // namespace basd

extern "C" {

int basd_trivial_augment(const unsigned char* src, unsigned char* dst, int B, int C, int H, int W,
                         const BasdTaugRecord* table, int* status, hipStream_t stream) {
    BASD_CHECK_ARG(B >= 0 && (C == 1 || C == 3) && H > 0 && W > 0);
    const long chw = (long)C * H * W;
    BASD_CHECK_ARG(chw < (1L << 30));                                  // 32-bit byte indices inside an image
    if (B == 0) return BASD_OK;
    BASD_CHECK_ARG(src && dst && table && status);
    const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (uintptr_t)(B * chw);
    const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + (uintptr_t)(B * chw);
    BASD_CHECK_ARG(s1 <= d0 || d1 <= s0);                              // an output pixel reads anywhere in its image
    static const bool attribute_set = [] {
        return hipFuncSetAttribute((const void*)basd::trivial_augment_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   basd::kTaugMaxLds) == hipSuccess;
    }();
    if (!attribute_set) return (int)hipErrorInvalidValue;
    basd::TaugArgs a = {};
    a.src = src; a.dst = dst; a.table = table; a.status = status;
    a.C = C; a.H = H; a.W = W; a.hw = H * W; a.chw = (int)chw;
    a.staged = chw <= basd::kTaugStageBytes ? 1 : 0;
    // staged: the image and up to 15 bytes in front of it, rounded up to 16
    const int lds = basd::kTaugImageOff + (a.staged ? (int)((chw + 15 + 15) & ~15L) : 0);
    basd::trivial_augment_kernel<<<B, basd::kTaugBlock, lds, stream>>>(a);
    BASD_RETURN_LAST();
}

}  // extern "C"
