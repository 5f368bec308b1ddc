// Baseline JPEG decoding of a batch of streams in THREE launches (the contract and the specification are in
// include/basd_hip.h; the per-image arithmetic is csrc/jpeg_core.h, which also compiles for the host).
//
//   entropy   one workgroup of one wave per image.  The record is checked first (uniform over the workgroup: a record
//             outside its bounds is never followed).  Lanes 0 .. 2 ncomp - 1 build the look-ahead tables of the
//             components' Huffman tables in LDS; then lane l decodes the entropy-coded segments l, l + 64, ... (one
//             segment: the whole image, or one restart interval), each block assembled in the lane's own 128 bytes of
//             LDS (pitch 33 words: the lanes' blocks start in different banks) and stored as 64 int16 (in the stream's zigzag order: the IDCT's indices are constants).  The stream is
//             read through aligned 8-byte words with one word of read-ahead.  The image's status word is written
//             unconditionally, so the workspace needs no clearing.
//   idct      one lane per block (grid: blocks x images): dequantise, the integer IDCT with the 64 intermediate values
//             in registers, 8 stores of 8 bytes into the component plane.
//   pixels    one lane per pixel (grid: pixels x images): up to four chroma taps per plane, the colour formula, three
//             byte stores; a raw record's pixels are copied from the byte buffer; a failed image is zeroed.
#include "basd_common.h"
#include "jpeg_core.h"

namespace basd {

constexpr int kJpegLanes = 64;
constexpr int kJpegBlockPitch = 33;                                    // 32-bit words between the lanes' blocks
constexpr int kJpegIdctBlock = 256;
constexpr int kJpegPixelBlock = 256;
static_assert(sizeof(BasdJpegRecord) == 128, "the record table has 128-byte rows");
static_assert(6 * sizeof(JpegHuff) + kJpegLanes * kJpegBlockPitch * 4 <= 32 * 1024, "several images share a CU's LDS");

struct JpegArgs {
    const unsigned char* src;
    long src_bytes;
    unsigned char* out;
    long out_bytes;
    const BasdJpegRecord* table;
    unsigned char* ws;
    long ws_bytes, ws_reserved;
    int* status;
};

__global__ void __launch_bounds__(kJpegLanes) jpeg_entropy_kernel(JpegArgs a) {
    __shared__ JpegHuff tables[6];
    __shared__ uint32_t blocks[kJpegLanes * kJpegBlockPitch];
    __shared__ int failed;
    const int lane = threadIdx.x, img = blockIdx.x;
    const BasdJpegRecord r = a.table[img];
    int* image_status = (int*)a.ws + img;
    int bad = jpeg_check_record(r, a.src_bytes, a.out_bytes, a.ws_bytes, a.ws_reserved);
    JpegGeometry g = {};
    if (!bad && r.kind == BASD_JPEG_KIND_STREAM) {
        g = jpeg_geometry(r);
        if (!jpeg_segments_ok(r, g)) bad = BASD_JPEG_BAD_RESTART;
    }
    if (bad || r.kind == BASD_JPEG_KIND_RAW) {                         // uniform over the workgroup
        if (lane == 0) {
            *image_status = bad;
            if (bad) atomicOr(a.status, 1 << (bad - 1));
        }
        return;
    }
    if (lane == 0) failed = 0;
    __syncthreads();
    const unsigned char* stream = a.src + r.src_offset;
    if (lane < 2 * r.ncomp) {
        const int c = lane < r.ncomp ? lane : lane - r.ncomp;
        const bool ok = jpeg_build_huff(stream, r.src_len, lane < r.ncomp ? jpeg_pick(r.dc, c) : jpeg_pick(r.ac, c),
                                        &tables[lane < r.ncomp ? c : 3 + c]);
        if (!ok) atomicMax(&failed, BASD_JPEG_BAD_TABLE);
    }
    __syncthreads();
    if (failed == 0) {                                                 // uniform
        short* coef = (short*)(a.ws + r.coef_offset);
        short* block = (short*)(blocks + lane * kJpegBlockPitch);
        for (int seg = lane; seg < r.n_seg; seg += kJpegLanes) {
            const int code = jpeg_decode_segment(r, g, a.src, seg, tables, block, coef);
            if (code) {
                atomicMax(&failed, code);
                break;
            }
        }
    }
    __syncthreads();
    if (lane == 0) {
        *image_status = failed;
        if (failed) atomicOr(a.status, 1 << (failed - 1));
    }
}

__global__ void __launch_bounds__(kJpegIdctBlock) jpeg_idct_kernel(JpegArgs a) {
    const int img = blockIdx.y;
    if (((const int*)a.ws)[img] != 0) return;                          // the record is only followed where it was admitted
    const BasdJpegRecord r = a.table[img];
    if (r.kind != BASD_JPEG_KIND_STREAM) return;
    const JpegGeometry g = jpeg_geometry(r);
    const long blk = (long)blockIdx.x * kJpegIdctBlock + threadIdx.x;
    if (blk >= g.blocks) return;
    int comp, pitch;
    long offset;
    jpeg_block_place(r, g, blk, comp, offset, pitch);
    jpeg_idct_block((const short*)(a.ws + r.coef_offset) + blk * 64, a.src + r.src_offset + jpeg_pick(r.quant, comp),
                    a.ws + r.plane_offset + offset, pitch);
}

__global__ void __launch_bounds__(kJpegPixelBlock) jpeg_pixel_kernel(JpegArgs a) {
    const int img = blockIdx.y;
    const BasdJpegRecord r = a.table[img];
    if (!jpeg_out_ok(r, a.out_bytes)) return;                          // nowhere to write (the status says so)
    const long pixels = (long)r.width * r.height;
    const long i = (long)blockIdx.x * kJpegPixelBlock + threadIdx.x;
    if (i >= pixels) return;
    unsigned char* o = a.out + r.out_offset + 3 * i;
    unsigned rgb = 0;
    if (((const int*)a.ws)[img] == 0) {
        if (r.kind == BASD_JPEG_KIND_RAW) {
            const unsigned char* p = a.src + r.src_offset + 3 * i;
            rgb = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
        } else {
            const int y = (int)(i / r.width), x = (int)(i - (long)y * r.width);
            rgb = jpeg_pixel(r, jpeg_geometry(r), a.ws + r.plane_offset, x, y);
        }
    }
    o[0] = (unsigned char)rgb;
    o[1] = (unsigned char)(rgb >> 8);
    o[2] = (unsigned char)(rgb >> 16);
}

}  // namespace basd

extern "C" {

long basd_jpeg_status_bytes(int B) { return B < 0 ? 0 : ((long)B * 4 + 127) & ~127L; }

int basd_jpeg_decode(const unsigned char* src, long src_bytes, unsigned char* out, long out_bytes, int B,
                     const BasdJpegRecord* table, unsigned char* ws, long ws_bytes, int* status, long max_blocks,
                     long max_pixels, hipStream_t stream) {
    BASD_CHECK_ARG(B >= 0 && B <= BASD_JPEG_MAX_BATCH && src_bytes >= 0 && out_bytes >= 0 && ws_bytes >= 0 &&
                   max_blocks >= 0 && max_pixels >= 0);
    if (B == 0) return BASD_OK;
    BASD_CHECK_ARG(src && out && table && ws && status);
    BASD_CHECK_ARG((src_bytes & 15) == 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)ws & 15) == 0);
    const long reserved = basd_jpeg_status_bytes(B);
    BASD_CHECK_ARG(ws_bytes >= reserved);
    const long side = BASD_JPEG_MAX_SIDE;
    BASD_CHECK_ARG(max_pixels <= side * side && max_blocks <= 3 * (side / 8 + 1) * (side / 8 + 1));
    const uintptr_t lo[3] = {(uintptr_t)src, (uintptr_t)out, (uintptr_t)ws};
    const uintptr_t hi[3] = {lo[0] + (uintptr_t)src_bytes, lo[1] + (uintptr_t)out_bytes, lo[2] + (uintptr_t)ws_bytes};
    for (int i = 0; i < 3; ++i)
        for (int j = i + 1; j < 3; ++j) BASD_CHECK_ARG(hi[i] <= lo[j] || hi[j] <= lo[i]);
    basd::JpegArgs a = {};
    a.src = src; a.src_bytes = src_bytes; a.out = out; a.out_bytes = out_bytes; a.table = table;
    a.ws = ws; a.ws_bytes = ws_bytes; a.ws_reserved = reserved; a.status = status;
    basd::jpeg_entropy_kernel<<<(unsigned)B, basd::kJpegLanes, 0, stream>>>(a);
    // always three launches (a batch of raw records alone has no blocks: one idle workgroup per image)
    const long idct_groups = (max_blocks + basd::kJpegIdctBlock - 1) / basd::kJpegIdctBlock;
    const long pixel_groups = (max_pixels + basd::kJpegPixelBlock - 1) / basd::kJpegPixelBlock;
    basd::jpeg_idct_kernel<<<dim3((unsigned)(idct_groups > 0 ? idct_groups : 1), (unsigned)B), basd::kJpegIdctBlock, 0,
                             stream>>>(a);
    basd::jpeg_pixel_kernel<<<dim3((unsigned)(pixel_groups > 0 ? pixel_groups : 1), (unsigned)B), basd::kJpegPixelBlock,
                              0, stream>>>(a);
    BASD_RETURN_LAST();
}

}  // extern "C"
