// 8-bit PNG decoding of a batch of files in TWO launches (the contract and the specification are in
// include/basd_hip.h; the per-image code is csrc/png_core.h, which also compiles for the host).
//
//   inflate    one workgroup of ONE wave per image, so nothing ever waits for another workgroup and a barrier is a
//              wait for the wave's own memory operations.  The decode state (bit reader, positions, symbols) is the
//              same in all 64 lanes: no divergence, every branch is uniform.  The lanes share the work that has width:
//              filling the look-up tables, and copying a match or a stored block.  Matches read a 32 KiB window of the
//              output kept in LDS, not the workspace: a match may read what the symbol before it wrote, and behind an
//              LDS write the wave waits for the LDS counter (tens of cycles) where behind a global store it would wait
//              for the store's acknowledgement from L2 (several hundred), once per match.  39 KiB of LDS per
//              workgroup leave four images per CU.  The wave leaves the image's status word and the offset of the
//              Adler-32 bytes in the status area, unconditionally, so the workspace needs no clearing.
//   unfilter   one workgroup of one wave per image: Adler-32 and filter bytes, then the skewed wavefront over bands of
//              64 scanlines with the RGB written in the same step; raw records are copied, failed images zeroed.
#include "basd_common.h"
#include "png_core.h"

namespace basd {

constexpr int kPngLanes = 64;
static_assert(sizeof(BasdPngRecord) == 64, "the record table has 64-byte rows");
static_assert(sizeof(PngInflateShared) <= 40 * 1024, "four images share a CU's LDS");

struct PngArgs {
    const unsigned char* src;
    long src_bytes;
    unsigned char* out;
    long out_bytes;
    const BasdPngRecord* table;
    unsigned char* ws;
    long ws_bytes, ws_reserved;
    int* status;
    int batch;
};

__global__ void __launch_bounds__(kPngLanes) png_inflate_kernel(PngArgs a) {
    __shared__ PngInflateShared sh;
    const int lane = threadIdx.x, img = blockIdx.x;
    const BasdPngRecord r = a.table[img];
    int code = png_check_record(r, a.src_bytes, a.out_bytes, a.ws_bytes, a.ws_reserved);
    int end_pos = 0;
    if (!code && r.kind == BASD_PNG_KIND_STREAM)                       // uniform over the workgroup
        code = png_inflate(a.src + r.src_offset, r.src_len, a.ws + r.ws_offset, (int)png_filtered_bytes(r), sh, lane,
                           kPngLanes, end_pos);
    if (lane == 0) {
        ((int*)a.ws)[img] = code;
        ((int*)a.ws)[a.batch + img] = end_pos;
        if (code) atomicOr(a.status, 1 << (code - 1));
    }
}

__global__ void __launch_bounds__(kPngLanes) png_unfilter_kernel(PngArgs a) {
    __shared__ unsigned long long sums[2 * kPngLanes];
    __shared__ int flags[kPngLanes];
    const int lane = threadIdx.x, img = blockIdx.x;
    const BasdPngRecord r = a.table[img];
    if (!png_out_ok(r, a.out_bytes)) return;                           // nowhere to write (the status says so)
    int code = ((const int*)a.ws)[img];
    unsigned char* out = a.out + r.out_offset;
    const long out_n = 3L * r.width * r.height;
    const int bpp = png_bpp(r.color_type);
    const long stride = (long)r.width * bpp + 1;
    unsigned char* lines = a.ws + r.ws_offset;
    if (code == 0 && r.kind == BASD_PNG_KIND_STREAM) {                 // the record was admitted by the first launch
        const long n = stride * r.height;
        uint64_t sa, sb;
        png_adler_partial(lines, n, lane, kPngLanes, sa, sb);
        sums[lane] = sa;
        sums[kPngLanes + lane] = sb;
        flags[lane] = png_bad_filters(lines, r.height, stride, lane, kPngLanes);
        __syncthreads();
        uint64_t ta = 0, tb = 0;
        int bad_filter = 0;
        for (int l = 0; l < kPngLanes; ++l) {
            ta += sums[l];
            tb += sums[kPngLanes + l];
            bad_filter |= flags[l];
        }
        const int end_pos = ((const int*)a.ws)[a.batch + img];
        if (png_adler_finish(ta, tb, n) != png_be32(a.src + r.src_offset + end_pos))
            code = BASD_PNG_BAD_ADLER;
        else if (bad_filter)
            code = BASD_PNG_BAD_FILTER;
        if (code && lane == 0) {
            ((int*)a.ws)[img] = code;
            atomicOr(a.status, 1 << (code - 1));
        }
    }
    if (code) {                                                        // uniform
        for (long i = lane; i < out_n; i += kPngLanes) out[i] = 0;
        return;
    }
    if (r.kind == BASD_PNG_KIND_RAW) {
        const unsigned char* from = a.src + r.src_offset;
        for (long i = lane; i < out_n; i += kPngLanes) out[i] = from[i];
        return;
    }
    const unsigned char* plte = a.src + (r.color_type == 3 ? r.plte_offset : 0);
    for (int r0 = 0; r0 < r.height; r0 += kPngLanes) {
        const int row = r0 + lane;
        const bool active = row < r.height;
        unsigned char* line = lines + (active ? row : 0) * stride + 1;
        const unsigned char* above = lines + (r0 ? r0 - 1 : 0) * stride + 1;     // lane 0's row above, kept by the band before
        unsigned char* rgb = out + 3L * (active ? row : 0) * r.width;
        PngRow s = {active ? (int)line[-1] : 0, 0u, 0u, 0u};
        const bool keep = lane == kPngLanes - 1 && r0 + kPngLanes < r.height;
        const int rows = r.height - r0 < kPngLanes ? r.height - r0 : kPngLanes;
        for (int t = 0; t < r.width + rows - 1; ++t) {
            const int x = t - lane;
            const bool inside = active && x >= 0 && x < r.width;
            uint32_t up = __shfl_up(s.last, 1);                        // lane l - 1 made pixel x of its row one step ago
            if (lane == 0) up = r0 && inside ? png_load_px(above + (long)x * bpp, bpp) : 0u;
            if (inside) png_unfilter_step(line, x, bpp, r.color_type, up, s, plte, rgb, keep);
        }
        __syncthreads();                                               // the kept row is written before lane 0 reads it
    }
}

}  // namespace basd

extern "C" {

long basd_png_status_bytes(int B) { return B < 0 ? 0 : ((long)B * 8 + 127) & ~127L; }

int basd_png_decode(const unsigned char* src, long src_bytes, unsigned char* out, long out_bytes, int B,
                    const BasdPngRecord* records, unsigned char* ws, long ws_bytes, int* status, long max_filtered,
                    long max_pixels, hipStream_t stream) {
    BASD_CHECK_ARG(B >= 0 && B <= BASD_PNG_MAX_BATCH && src_bytes >= 0 && out_bytes >= 0 && ws_bytes >= 0 &&
                   max_filtered >= 0 && max_pixels >= 0);
    if (B == 0) return BASD_OK;
    BASD_CHECK_ARG(src && out && records && ws && status);
    BASD_CHECK_ARG((src_bytes & 15) == 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)ws & 15) == 0);
    const long reserved = basd_png_status_bytes(B);
    BASD_CHECK_ARG(ws_bytes >= reserved);
    const long side = BASD_PNG_MAX_SIDE;
    BASD_CHECK_ARG(max_pixels <= side * side && max_filtered <= side * (4 * side + 1));
    const uintptr_t lo[3] = {(uintptr_t)src, (uintptr_t)out, (uintptr_t)ws};
    const uintptr_t hi[3] = {lo[0] + (uintptr_t)src_bytes, lo[1] + (uintptr_t)out_bytes, lo[2] + (uintptr_t)ws_bytes};
    for (int i = 0; i < 3; ++i)
        for (int j = i + 1; j < 3; ++j) BASD_CHECK_ARG(hi[i] <= lo[j] || hi[j] <= lo[i]);
    basd::PngArgs a = {};
    a.src = src; a.src_bytes = src_bytes; a.out = out; a.out_bytes = out_bytes; a.table = records;
    a.ws = ws; a.ws_bytes = ws_bytes; a.ws_reserved = reserved; a.status = status; a.batch = B;
    // always two launches, one wave per image each (max_filtered and max_pixels size nothing: they are checked only)
    basd::png_inflate_kernel<<<(unsigned)B, basd::kPngLanes, 0, stream>>>(a);
    basd::png_unfilter_kernel<<<(unsigned)B, basd::kPngLanes, 0, stream>>>(a);
    BASD_RETURN_LAST();
}

}  // extern "C"
