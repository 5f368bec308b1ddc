// The JPEG decoder's per-image code (csrc/jpeg_core.h) compiled for the host, as a stand-alone program: it runs the
// three stages of csrc/jpeg.hip as plain loops over a packed batch, in buffers of exactly the batch's sizes, so a
// sanitizer build (-fsanitize=address,undefined) sees every read and write the kernels would make.
//
//   jpeg_host_check IN OUT
//
// IN:  8 int64 (magic 0x4745504a44534142, B, src_bytes, out_bytes, ws_bytes, 0, 0, 0), B records of 128 bytes, the byte
//      buffer (what basd_amd.jpeg.pack_jpegs makes; tests/test_jpeg_decode.py writes the file).
// OUT: the out_bytes output bytes, B int32 per-image status words, one int32 batch status word.
// Exit status 0 whatever the streams hold (a bad stream is a status word, not a failure); 2 for a bad IN file.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../vit-inductive-bias-distillation_amd/csrc/jpeg_core.h"

using namespace basd;

namespace {

constexpr long long kMagic = 0x4745504a44534142LL;

struct Buffer {                        // malloc'ed to the byte: 16-byte aligned, and the sanitizer guards both ends
    unsigned char* p = nullptr;
    long n = 0;
    explicit Buffer(long bytes) : p((unsigned char*)malloc(bytes > 0 ? (size_t)bytes : 1)), n(bytes) {}
    ~Buffer() { free(p); }
};

long status_bytes(long B) { return (B * 4 + 127) & ~127L; }

// jpeg_entropy_kernel, the lanes one after the other
int entropy(const BasdJpegRecord& r, const unsigned char* src, long src_bytes, long out_bytes, unsigned char* ws,
            long ws_bytes, long reserved) {
    int bad = jpeg_check_record(r, src_bytes, out_bytes, ws_bytes, reserved);
    JpegGeometry g = {};
    if (!bad && r.kind == BASD_JPEG_KIND_STREAM) {
        g = jpeg_geometry(r);
        if (!jpeg_segments_ok(r, g)) bad = BASD_JPEG_BAD_RESTART;
    }
    if (bad || r.kind == BASD_JPEG_KIND_RAW) return bad;
    std::vector<JpegHuff> tables(6);
    const unsigned char* stream = src + r.src_offset;
    for (int c = 0; c < r.ncomp; ++c) {
        if (!jpeg_build_huff(stream, r.src_len, r.dc[c], &tables[c])) return BASD_JPEG_BAD_TABLE;
        if (!jpeg_build_huff(stream, r.src_len, r.ac[c], &tables[3 + c])) return BASD_JPEG_BAD_TABLE;
    }
    int failed = 0;
    alignas(16) short block[64];
    for (int seg = 0; seg < r.n_seg; ++seg) {
        const int code = jpeg_decode_segment(r, g, src, seg, tables.data(), block, (short*)(ws + r.coef_offset));
        if (code > failed) failed = code;
    }
    return failed;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    long long head[8];
    if (fread(head, 8, 8, f) != 8 || head[0] != kMagic) return 2;
    const long B = head[1], src_bytes = head[2], out_bytes = head[3], ws_bytes = head[4];
    if (B < 0 || B > BASD_JPEG_MAX_BATCH || src_bytes < 0 || (src_bytes & 15) || out_bytes < 0 ||
        ws_bytes < status_bytes(B))
        return 2;
    std::vector<BasdJpegRecord> table((size_t)B);
    Buffer src(src_bytes), out(out_bytes), ws(ws_bytes);
    if (!src.p || !out.p || !ws.p) return 2;
    if (B && fread(table.data(), sizeof(BasdJpegRecord), (size_t)B, f) != (size_t)B) return 2;
    if (src_bytes && fread(src.p, 1, (size_t)src_bytes, f) != (size_t)src_bytes) return 2;
    fclose(f);
    memset(out.p, 0xA5, (size_t)out_bytes);            // what the decoder does not write stays recognisable
    memset(ws.p, 0xA5, (size_t)ws_bytes);
    int* image_status = (int*)ws.p;
    int status = 0;
    const long reserved = status_bytes(B);
    for (long b = 0; b < B; ++b) {
        const int code = entropy(table[b], src.p, src_bytes, out_bytes, ws.p, ws_bytes, reserved);
        image_status[b] = code;
        if (code) status |= 1 << (code - 1);
    }
    for (long b = 0; b < B; ++b) {                     // jpeg_idct_kernel
        const BasdJpegRecord& r = table[b];
        if (image_status[b] != 0 || r.kind != BASD_JPEG_KIND_STREAM) continue;
        const JpegGeometry g = jpeg_geometry(r);
        for (long blk = 0; blk < g.blocks; ++blk) {
            int comp, pitch;
            long offset;
            jpeg_block_place(r, g, blk, comp, offset, pitch);
            jpeg_idct_block((const short*)(ws.p + r.coef_offset) + blk * 64, src.p + r.src_offset + jpeg_pick(r.quant, comp),
                            ws.p + r.plane_offset + offset, pitch);
        }
    }
    for (long b = 0; b < B; ++b) {                     // jpeg_pixel_kernel
        const BasdJpegRecord& r = table[b];
        if (!jpeg_out_ok(r, out_bytes)) continue;
        const long pixels = (long)r.width * r.height;
        for (long i = 0; i < pixels; ++i) {
            unsigned rgb = 0;
            if (image_status[b] == 0) {
                if (r.kind == BASD_JPEG_KIND_RAW) {
                    const unsigned char* p = src.p + r.src_offset + 3 * i;
                    rgb = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
                } else {
                    const int y = (int)(i / r.width), x = (int)(i - (long)y * r.width);
                    rgb = jpeg_pixel(r, jpeg_geometry(r), ws.p + r.plane_offset, x, y);
                }
            }
            unsigned char* o = out.p + r.out_offset + 3 * i;
            o[0] = (unsigned char)rgb;
            o[1] = (unsigned char)(rgb >> 8);
            o[2] = (unsigned char)(rgb >> 16);
        }
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(out.p, 1, (size_t)out_bytes, f);
    fwrite(image_status, 4, (size_t)B, f);
    fwrite(&status, 4, 1, f);
    fclose(f);
    return 0;
}
