// basd_jpeg_decode_progressive's per-image code (csrc/jpeg_core.h) compiled for the host, as a stand-alone program: it
// runs the four stages of csrc/jpeg.hip as plain loops over a packed batch, in buffers of exactly the batch's sizes, so
// a sanitizer build (-fsanitize=address,undefined) sees every read and write the kernels would make.  The scans of a
// progressive record run in stream order and stop at the first scan that has a failing segment, which is the status
// rule of include/basd_hip.h; the kernel's schedule by levels has to give the same words and bytes.
//
//   jpeg_progressive_host_check IN OUT
//
// IN:  8 int64 (magic 0x4745504a44534142, B, src_bytes, out_bytes, ws_bytes, max_scans, max_segments, 0), B records of
//      128 bytes, the byte buffer (what basd_amd.jpeg.pack_jpegs(..., progressive=True) makes).
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

// jpeg_progressive_kernel: the scans one after the other, every segment of a scan
int progressive(const BasdJpegRecord& r, const unsigned char* src, long src_bytes, long out_bytes, unsigned char* ws,
                long ws_bytes, long reserved, int max_scans, int max_segments) {
    const int bad = jpeg_check_progressive(r, src_bytes, out_bytes, ws_bytes, reserved, max_scans);
    if (bad) return bad;
    std::vector<BasdJpegScan> scans((size_t)r.n_scans);
    memcpy(scans.data(), src + r.src_offset + r.scan_offset, sizeof(BasdJpegScan) * (size_t)r.n_scans);
    for (const BasdJpegScan& s : scans)
        if (!jpeg_check_scan(r, s, src_bytes, max_segments)) return BASD_JPEG_BAD_RECORD;
    const JpegGeometry g = jpeg_geometry(r);
    short* coef = (short*)(ws + r.coef_offset);
    memset(coef, 0, (size_t)g.blocks * 128);
    std::vector<JpegHuff> tables(3);
    const unsigned char* stream = src + r.src_offset;
    for (const BasdJpegScan& s : scans) {
        if (s.ss == 0 && s.ah == 0) {
            for (int c = 0; c < r.ncomp; ++c)
                if ((s.ncomp > 1 || c == s.comp) && !jpeg_build_huff(stream, r.src_len, s.dc[c], &tables[c]))
                    return BASD_JPEG_BAD_TABLE;
        } else if (s.ss > 0 && !jpeg_build_huff(stream, r.src_len, s.ac, &tables[0])) {
            return BASD_JPEG_BAD_TABLE;
        }
        int row;
        if (!jpeg_scan_segments_ok(s, jpeg_scan_units(r, g, s, row))) return BASD_JPEG_BAD_RESTART;
        int failed = 0;
        for (int seg = 0; seg < s.n_seg; ++seg) {
            const int code = jpeg_scan_segment(r, g, s, src, seg, tables.data(), coef);
            if (code > failed) failed = code;
        }
        if (failed) return failed;
    }
    return 0;
}

// jpeg_entropy_kernel<true>, the lanes one after the other
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
    const long max_scans = head[5], max_segments = head[6];
    if (B < 0 || B > BASD_JPEG_MAX_BATCH || src_bytes < 0 || (src_bytes & 15) || out_bytes < 0 ||
        ws_bytes < status_bytes(B) || max_scans < 0 || max_scans > BASD_JPEG_MAX_SCANS || max_segments < 0 ||
        max_segments > 0x7fffffff)
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
    for (long b = 0; b < B; ++b) {                     // jpeg_progressive_kernel, then the baseline entropy kernel
        const BasdJpegRecord& r = table[b];
        const int code = r.kind == BASD_JPEG_KIND_PROGRESSIVE
                             ? progressive(r, src.p, src_bytes, out_bytes, ws.p, ws_bytes, reserved, (int)max_scans,
                                           (int)max_segments)
                             : entropy(r, src.p, src_bytes, out_bytes, ws.p, ws_bytes, reserved);
        image_status[b] = code;
        if (code) status |= 1 << (code - 1);
    }
    for (long b = 0; b < B; ++b) {                     // jpeg_idct_kernel
        const BasdJpegRecord& r = table[b];
        if (image_status[b] != 0 || (r.kind != BASD_JPEG_KIND_STREAM && r.kind != BASD_JPEG_KIND_PROGRESSIVE)) continue;
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
