// Pillow-exact crops and resizes (bilinear, bicubic, box; chosen per record) of ragged uint8 HWC images into dense uint8
// NCHW batches in ONE launch (the contract and the specification are in include/basd_hip.h; the per-axis code -- taps,
// tap count, record check -- is resize_core.h, which a host program compiles too).
//
// One workgroup of 8 waves per (band of output rows, record).  The record is uniform over the workgroup, so its
// validation and its filter cost no divergence: a record outside its limits has its band zeroed and nothing of it is
// read.  Phases:
//   coefficients  the horizontal taps of the workgroup's columns and the vertical taps of its rows, one lane per column /
//                 row, fp64 with contraction off, as integers of 22 fractional bits in LDS.  Each is made once.  The
//                 passes below only see integer taps (of either sign) and do not know the filter.
//   horizontal    for the source rows the vertical taps of a run of output rows need: one lane per (row, column), the
//                 C channels of a pixel together, bytes from global memory, the rounded byte into LDS (planar, pitch a
//                 multiple of 4).  The run is as long as BASD_RESIZE_STAGE_BYTES allows (a band is cut where it does
//                 not fit), and a row too wide for the coefficient table or for the stage is cut into column chunks.
//   vertical      out of LDS, four neighbouring bytes of a row per lane through one 32-bit LDS read per tap, and one
//                 32-bit store where the destination is aligned (single bytes otherwise and at a row's end).
#include "basd_common.h"
#include "resize_core.h"

namespace basd {

constexpr int kResizeBlock = 512;
constexpr int kResizeBandMax = 32;                                     // output rows of a workgroup
constexpr int kResizeColsMax = 1024;                                   // columns of a chunk
constexpr int kResizeCoefInts = 4096;                                  // horizontal coefficients of a chunk
constexpr int kResizeStage = BASD_RESIZE_STAGE_BYTES;
constexpr int kResizeHxOff = 0;                                        // ResizeSpan (first tap, taps) per column
constexpr int kResizeKhOff = kResizeHxOff + kResizeColsMax * 8;
constexpr int kResizeVyOff = kResizeKhOff + kResizeCoefInts * 4;       // ResizeSpan per row
constexpr int kResizeKvOff = kResizeVyOff + kResizeBandMax * 8;
constexpr int kResizeStageOff = (kResizeKvOff + kResizeBandMax * kResizeTapsMax * 4 + 15) & ~15;
constexpr int kResizeLds = kResizeStageOff + kResizeStage;
static_assert(kResizeLds <= 80 * 1024, "two workgroups share a CU's 160 KiB of LDS");
static_assert(kResizeStage / (3 * kResizeTapsMax) >= 8, "the taps of one output row always fit the stage");
static_assert(sizeof(BasdResizeRecord) == 64, "the record table has 64-byte rows");
static_assert(offsetof(BasdResizeRecord, filter) == 48, "the filter took the first reserved word");
static_assert(sizeof(ResizeSpan) == 8, "one 64-bit LDS read per span");

struct ResizeArgs {
    const unsigned char* src;
    long src_bytes;
    unsigned char* dst;
    const BasdResizeRecord* table;
    int* status;
    int C, OH, OW, band, bands;
};

__global__ void __launch_bounds__(kResizeBlock) resize_crop_kernel(ResizeArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    ResizeSpan* hx = (ResizeSpan*)(smem + kResizeHxOff);
    int* kh = (int*)(smem + kResizeKhOff);
    ResizeSpan* vy = (ResizeSpan*)(smem + kResizeVyOff);
    int* kv = (int*)(smem + kResizeKvOff);
    unsigned char* stage = smem + kResizeStageOff;
    const int tid = threadIdx.x;
    const int rec = (int)(blockIdx.x / (unsigned)a.bands), band = (int)(blockIdx.x - (unsigned)rec * a.bands);
    const BasdResizeRecord r = a.table[rec];
    const int C = a.C, OH = a.OH, OW = a.OW;
    const int y0 = band * a.band;
    const int nrows = OH - y0 < a.band ? OH - y0 : a.band;
    unsigned char* d = a.dst + (long)rec * C * OH * OW;

    const int bad = resize_check(r, a.src_bytes, a.C, a.OH, a.OW);
    if (bad) {                                                         // uniform over the workgroup
        if (tid == 0 && band == 0) atomicOr(a.status, bad);
        const int per_plane = nrows * OW;
        for (int i = tid; i < C * per_plane; i += kResizeBlock) {
            const int c = i / per_plane;
            d[((long)c * OH + y0) * OW + (i - c * per_plane)] = 0;
        }
        return;
    }

    const int filter = r.filter;                                       // uniform, and one of the three
    const int ksh = resize_ksize(r.win_w, r.res_w, filter), ksv = resize_ksize(r.win_h, r.res_h, filter);
    // columns of a chunk: the coefficient table, the column table and ksv rows of the stage hold them
    int cw = OW;
    cw = cw < kResizeCoefInts / ksh ? cw : kResizeCoefInts / ksh;
    cw = cw < kResizeColsMax ? cw : kResizeColsMax;
    const int stage_cols = (kResizeStage / (C * ksv)) & ~3;
    cw = cw < stage_cols ? cw : stage_cols;
    if (cw < OW) cw &= ~3;                                             // later chunks start at a multiple of 4
    const unsigned char* window = a.src + r.src_offset + ((long)r.win_y * r.src_w + r.win_x) * C;
    const long src_pitch = (long)r.src_w * C;

    for (int x0 = 0; x0 < OW; x0 += cw) {
        const int cols = OW - x0 < cw ? OW - x0 : cw;
        const int cwp = (cols + 3) & ~3;
        const int pitch = C * cwp;
        const int max_rows = kResizeStage / pitch;                     // >= ksv

        // ---- coefficients (the rows' with the first chunk)
        const int items = cols + (x0 == 0 ? nrows : 0);
        for (int i = tid; i < items; i += kResizeBlock) {
            if (i < cols) hx[i] = resize_taps(r.win_w, r.res_w, r.out_x + x0 + i, ksh, filter, kh + i * ksh);
            else vy[i - cols] = resize_taps(r.win_h, r.res_h, r.out_y + y0 + (i - cols), ksv, filter,
                                            kv + (i - cols) * ksv);
        }
        __syncthreads();

        for (int s = 0; s < nrows;) {
            // the longest run of output rows whose source rows fit the stage (first taps and ends do not decrease)
            const int row0 = vy[s].first;
            int e = s + 1;
            while (e < nrows && vy[e].first + vy[e].count - row0 <= max_rows) ++e;
            int nsrc = vy[e - 1].first + vy[e - 1].count - row0;
            nsrc = nsrc > max_rows ? max_rows : nsrc;                  // never: vy[s].count <= ksv <= max_rows

            // Both passes multiply with __mul24 (v_mad_i32_i24, full rate; a 32-bit multiply is not): a coefficient is a
            // signed 24-bit number (|w / ww| < 2, so |k| < 2^23) and a byte is one too, and the product is exact.
            // ---- horizontal: source rows row0 .. row0 + nsrc of the window -> stage
            for (int i = tid; i < nsrc * cols; i += kResizeBlock) {
                const int rr = i / cols, col = i - rr * cols;
                const ResizeSpan t = hx[col];
                const unsigned char* p = window + (long)(row0 + rr) * src_pitch + (long)t.first * C;
                const int* k = kh + col * ksh;
                unsigned char* q = stage + rr * pitch + col;
                if (C == 3) {
                    int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
                    for (int j = 0; j < t.count; ++j) {
                        const int kk = k[j];
                        a0 += __mul24(kk, (int)p[3 * j]);
                        a1 += __mul24(kk, (int)p[3 * j + 1]);
                        a2 += __mul24(kk, (int)p[3 * j + 2]);
                    }
                    q[0] = (unsigned char)resize_clip(a0);
                    q[cwp] = (unsigned char)resize_clip(a1);
                    q[2 * cwp] = (unsigned char)resize_clip(a2);
                } else {
                    int a0 = 1 << 21;
                    for (int j = 0; j < t.count; ++j) a0 += __mul24(k[j], (int)p[j]);
                    q[0] = (unsigned char)resize_clip(a0);
                }
            }
            __syncthreads();

            // ---- vertical: output rows s .. e, four bytes of a row per lane
            const int groups = cwp >> 2;
            const int pitch4 = pitch >> 2;
            for (int i = tid; i < (e - s) * C * groups; i += kResizeBlock) {
                const int g = i % groups, yc = i / groups;
                const int c = yc % C, y = s + yc / C;
                const ResizeSpan t = vy[y];
                const unsigned* q = (const unsigned*)(stage + (t.first - row0) * pitch + c * cwp) + g;
                const int* k = kv + y * ksv;
                int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21, a3 = 1 << 21;
                for (int j = 0; j < t.count; ++j) {
                    const unsigned w = q[j * pitch4];
                    const int kk = k[j];
                    a0 += __mul24(kk, (int)(w & 255u));
                    a1 += __mul24(kk, (int)((w >> 8) & 255u));
                    a2 += __mul24(kk, (int)((w >> 16) & 255u));
                    a3 += __mul24(kk, (int)(w >> 24));
                }
                const unsigned o0 = resize_clip(a0), o1 = resize_clip(a1), o2 = resize_clip(a2), o3 = resize_clip(a3);
                unsigned char* dp = d + ((long)c * OH + y0 + y) * OW + x0 + 4 * g;
                const int left = cols - 4 * g;                          // >= 1
                if (left >= 4 && ((uintptr_t)dp & 3) == 0) {
                    *(unsigned*)dp = o0 | (o1 << 8) | (o2 << 16) | (o3 << 24);
                } else {
                    dp[0] = (unsigned char)o0;
                    if (left > 1) dp[1] = (unsigned char)o1;
                    if (left > 2) dp[2] = (unsigned char)o2;
                    if (left > 3) dp[3] = (unsigned char)o3;
                }
            }
            __syncthreads();                                           // the stage and the tables are free again
            s = e;
        }
    }
}

}  // namespace basd

extern "C" {

int basd_resize_crop(const unsigned char* src, long src_bytes, unsigned char* dst, int n, int C, int OH, int OW,
                     const BasdResizeRecord* table, int* status, int band_rows, hipStream_t stream) {
    BASD_CHECK_ARG(n >= 0 && (C == 1 || C == 3) && OH >= 1 && OW >= 1 && OH <= BASD_RESIZE_MAX_SIDE &&
                   OW <= BASD_RESIZE_MAX_SIDE && src_bytes >= 0);
    const long chw = (long)C * OH * OW;
    BASD_CHECK_ARG(chw < (1L << 30));
    BASD_CHECK_ARG(band_rows >= 0 && band_rows <= basd::kResizeBandMax);
    if (n == 0) return BASD_OK;
    BASD_CHECK_ARG(src && dst && table && status);
    const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (uintptr_t)src_bytes;
    const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + (uintptr_t)(n * chw);
    BASD_CHECK_ARG(s1 <= d0 || d1 <= s0);
    int band = band_rows;
    if (band == 0) {
        band = basd::kResizeBandMax;
        while (band > 4 && (long)n * ((OH + band - 1) / band) < 1024) band >>= 1;
    }
    const long bands = (OH + band - 1) / band;
    BASD_CHECK_ARG(n * bands < (1L << 31));
    static const bool attribute_set = [] {
        return hipFuncSetAttribute((const void*)basd::resize_crop_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   basd::kResizeLds) == hipSuccess;
    }();
    if (!attribute_set) return (int)hipErrorInvalidValue;
    basd::ResizeArgs a = {};
    a.src = src; a.src_bytes = src_bytes; a.dst = dst; a.table = table; a.status = status;
    a.C = C; a.OH = OH; a.OW = OW; a.band = band; a.bands = (int)bands;
    basd::resize_crop_kernel<<<(unsigned)(n * bands), basd::kResizeBlock, basd::kResizeLds, stream>>>(a);
    BASD_RETURN_LAST();
}

}  // extern "C"
