// The per-axis code of the resize (specification: include/basd_hip.h) as host + device functions: the filters' weight
// functions, the taps of one output index, the tap count, the record check and the rounding of an accumulator.
// csrc/resize.hip calls them from its kernel, tools/resize_host_check.cpp compiles the same text for the host under the
// sanitizers.  Nothing here allocates or touches memory other than the k[] it is handed.
#pragma once
#include "../../include/basd_hip.h"

#ifndef BASD_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define BASD_HD __host__ __device__ __forceinline__
#else
#define BASD_HD inline
#endif
#endif

namespace basd {

constexpr int kResizeTapsMax = 2 * BASD_RESIZE_MAX_RATIO + 1;          // 65

struct alignas(8) ResizeSpan {                                         // the taps of one output index
    int first, count;                                                  // source indices first .. first + count
};

BASD_HD bool resize_filter_ok(int filter) {
    return filter == BASD_RESIZE_FILTER_BILINEAR || filter == BASD_RESIZE_FILTER_BICUBIC ||
           filter == BASD_RESIZE_FILTER_BOX;
}

// Twice the filter's support S_f (1.0, 2.0, 0.5), which is an integer.
BASD_HD int resize_support2(int filter) {
    return filter == BASD_RESIZE_FILTER_BICUBIC ? 4 : filter == BASD_RESIZE_FILTER_BOX ? 1 : 2;
}

// The largest reduction in / out of a filter: ceil(S_f * in / out) <= BASD_RESIZE_MAX_RATIO, and never above
// BASD_RESIZE_MAX_RATIO itself (which is what holds box back: its support alone would admit 64).
BASD_HD int resize_max_reduction(int filter) {
    return filter == BASD_RESIZE_FILTER_BICUBIC ? BASD_RESIZE_MAX_RATIO / 2 : BASD_RESIZE_MAX_RATIO;
}

// 2 ceil(support) + 1 with support = S_f * fs, fs = max(fp64(in) / fp64(out), 1), in integers.  S_f * fs is exact in
// fp64 (S_f is a power of two), so only the quotient rounds.  For in > out the real number q = S_f * in / out is a
// multiple of 1 / (2 out): where it is an integer, in / out is a multiple of 1/2 or of 2 and the fp64 quotient is exact;
// where it is not, it is at least 1 / (2 out) >= 2^-21 away from the next integer, the fp64 value less than
// q * 2^-52 <= 2^-45 away from q, so both have the ceiling ceil(S2 * in / (2 out)) with S2 = 2 S_f.
BASD_HD int resize_ksize(int in, int out, int filter) {
    const long s2 = resize_support2(filter);
    const long c = in > out ? (s2 * in + 2L * out - 1) / (2L * out) : (s2 + 1) / 2;
    return 2 * (int)c + 1;
}

template <int F>
BASD_HD double resize_weight(double t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (F == BASD_RESIZE_FILTER_BOX) return (t > -0.5 && t <= 0.5) ? 1.0 : 0.0;   // no |t|: the asymmetry is Pillow's
    t = t < 0.0 ? -t : t;
    if (F == BASD_RESIZE_FILTER_BILINEAR) return t < 1.0 ? 1.0 - t : 0.0;
    const double a = -0.5;
    if (t < 1.0) return ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0;
    if (t < 2.0) return (((t - 5.0) * t + 8.0) * t - 4.0) * a;
    return 0.0;
}

// The taps of output index xx: k[0 .. count) and the first source index (the formulas of the header, in their order).
template <int F>
BASD_HD ResizeSpan resize_taps_of(int in, int out, int xx, int ksize, int* k) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = (F == BASD_RESIZE_FILTER_BICUBIC ? 2.0 : F == BASD_RESIZE_FILTER_BOX ? 0.5 : 1.0) * fs;
    const double inv = 1.0 / fs;
    const double center = ((double)xx + 0.5) * scale;
    int lo = (int)((center - support) + 0.5);
    int hi = (int)((center + support) + 0.5);
    lo = lo < 0 ? 0 : lo;
    hi = hi > in ? in : hi;
    int n = hi - lo;
    n = n < 0 ? 0 : n > ksize ? ksize : n;
    double ww = 0.0;
    for (int x = 0; x < n; ++x) {
        const double w = resize_weight<F>((((double)(x + lo) - center) + 0.5) * inv);
        ww = ww + w;
    }
    for (int x = 0; x < n; ++x) {
        double w = resize_weight<F>((((double)(x + lo) - center) + 0.5) * inv);
        if (ww != 0.0) w = w / ww;
        const double scaled = w * 4194304.0;
        // only bicubic has negative weights
        k[x] = (F == BASD_RESIZE_FILTER_BICUBIC && w < 0.0) ? (int)(-0.5 + scaled) : (int)(0.5 + scaled);
    }
    return ResizeSpan{lo, n};
}

// filter has passed resize_filter_ok (anything else is taken as bilinear here)
BASD_HD ResizeSpan resize_taps(int in, int out, int xx, int ksize, int filter, int* k) {
    if (filter == BASD_RESIZE_FILTER_BICUBIC) return resize_taps_of<BASD_RESIZE_FILTER_BICUBIC>(in, out, xx, ksize, k);
    if (filter == BASD_RESIZE_FILTER_BOX) return resize_taps_of<BASD_RESIZE_FILTER_BOX>(in, out, xx, ksize, k);
    return resize_taps_of<BASD_RESIZE_FILTER_BILINEAR>(in, out, xx, ksize, k);
}

// acc = 2^21 + sum k * p in int32.  The bicubic coefficients have both signs, so acc may be negative or above
// 255 << 22; the shift is arithmetic and the clamp cuts both.  acc stays inside int32: sum |k| is at most about
// 1.3 * 2^22 (the full kernel has 1.25; clamping at the window and the rounding of the k add little), and
// 255 * 1.3 * 2^22 + 2^21 < 2^31.
BASD_HD unsigned resize_clip(int acc) {
    const int v = acc >> 22;
    return v < 0 ? 0u : v > 255 ? 255u : (unsigned)v;
}

// Every field of a record against the source buffer and the output rectangle: 0, or one BASD_RESIZE_BAD_* bit.
BASD_HD int resize_check(const BasdResizeRecord& r, long src_bytes, int C, int OH, int OW) {
    const long lim = BASD_RESIZE_MAX_SIDE;
    bool ok = r.src_h >= 1 && r.src_w >= 1 && r.src_h <= lim && r.src_w <= lim && r.res_h >= 1 && r.res_w >= 1 &&
              r.res_h <= lim && r.res_w <= lim;
    ok = ok && r.src_offset >= 0 && r.src_offset <= src_bytes &&
         (long)r.src_h * r.src_w * C <= src_bytes - r.src_offset;                   // sides <= 2^20: no overflow
    ok = ok && r.win_x >= 0 && r.win_y >= 0 && r.win_w >= 1 && r.win_h >= 1 && (long)r.win_x + r.win_w <= r.src_w &&
         (long)r.win_y + r.win_h <= r.src_h;
    ok = ok && r.out_x >= 0 && r.out_y >= 0 && (long)r.out_x + OW <= r.res_w && (long)r.out_y + OH <= r.res_h;
    if (!ok) return BASD_RESIZE_BAD_GEOMETRY;
    if (!resize_filter_ok(r.filter)) return BASD_RESIZE_BAD_FILTER;
    const long most = resize_max_reduction(r.filter);
    if (r.win_w > most * r.res_w || r.win_h > most * r.res_h) return BASD_RESIZE_BAD_RATIO;
    return 0;
}

}  // namespace basd
