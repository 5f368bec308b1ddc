// The PNG decoder's per-image code (csrc/png_core.h) compiled for the host, as a stand-alone program: it runs the two
// stages of csrc/png.hip as plain loops (lanes = 1) over a packed batch, in buffers of exactly the batch's sizes, so a
// sanitizer build (-fsanitize=address,undefined) sees every read and write the kernels would make.
//
//   png_host_check IN OUT
//
// IN:  8 int64 (magic 0x474e504444534142, B, src_bytes, out_bytes, ws_bytes, 0, 0, 0), B records of 64 bytes, the byte
//      buffer (what basd_amd.png.pack_pngs makes; tests/test_png_decode.py writes the file).
// OUT: the out_bytes output bytes, B int32 per-image status words, one int32 batch status word.
// Exit status 0 whatever the streams hold (a bad stream is a status word, not a failure); 2 for a bad IN file.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../vit-inductive-bias-distillation_amd/csrc/png_core.h"

using namespace basd;

namespace {

constexpr long long kMagic = 0x474e504444534142LL;

struct Buffer {                        // malloc'ed to the byte: 16-byte aligned, and the sanitizer guards both ends
    unsigned char* p = nullptr;
    long n = 0;
    explicit Buffer(long bytes) : p((unsigned char*)malloc(bytes > 0 ? (size_t)bytes : 1)), n(bytes) {}
    ~Buffer() { free(p); }
};

long status_bytes(long B) { return (B * 8 + 127) & ~127L; }

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    long long head[8];
    if (fread(head, 8, 8, f) != 8 || head[0] != kMagic) return 2;
    const long B = head[1], src_bytes = head[2], out_bytes = head[3], ws_bytes = head[4];
    if (B < 0 || B > BASD_PNG_MAX_BATCH || src_bytes < 0 || (src_bytes & 15) || out_bytes < 0 || ws_bytes < status_bytes(B))
        return 2;
    std::vector<BasdPngRecord> table((size_t)B);
    Buffer src(src_bytes), out(out_bytes), ws(ws_bytes);
    if (!src.p || !out.p || !ws.p) return 2;
    if (B && fread(table.data(), sizeof(BasdPngRecord), (size_t)B, f) != (size_t)B) return 2;
    if (src_bytes && fread(src.p, 1, (size_t)src_bytes, f) != (size_t)src_bytes) return 2;
    fclose(f);
    memset(out.p, 0xA5, (size_t)out_bytes);            // what the decoder does not write stays recognisable
    memset(ws.p, 0xA5, (size_t)ws_bytes);
    int* image_status = (int*)ws.p;
    int* end_pos = image_status + B;
    int status = 0;
    const long reserved = status_bytes(B);
    std::vector<PngInflateShared> shared(1);
    for (long i = 0; i < B; ++i) {                      // png_inflate_kernel
        const BasdPngRecord& r = table[i];
        int code = png_check_record(r, src_bytes, out_bytes, ws_bytes, reserved);
        int at = 0;
        if (!code && r.kind == BASD_PNG_KIND_STREAM)
            code = png_inflate(src.p + r.src_offset, r.src_len, ws.p + r.ws_offset, (int)png_filtered_bytes(r), shared[0], 0,
                               1, at);
        image_status[i] = code;
        end_pos[i] = at;
        if (code) status |= 1 << (code - 1);
    }
    for (long i = 0; i < B; ++i) {                      // png_unfilter_kernel
        const BasdPngRecord& r = table[i];
        if (!png_out_ok(r, out_bytes)) continue;
        int code = image_status[i];
        unsigned char* o = out.p + r.out_offset;
        const long out_n = 3L * r.width * r.height;
        const int bpp = png_bpp(r.color_type);
        const long stride = (long)r.width * bpp + 1;
        unsigned char* lines = ws.p + r.ws_offset;
        if (code == 0 && r.kind == BASD_PNG_KIND_STREAM) {
            const long n = stride * r.height;
            uint64_t sa, sb;
            png_adler_partial(lines, n, 0, 1, sa, sb);
            const int bad_filter = png_bad_filters(lines, r.height, stride, 0, 1);
            if (png_adler_finish(sa, sb, n) != png_be32(src.p + r.src_offset + end_pos[i]))
                code = BASD_PNG_BAD_ADLER;
            else if (bad_filter)
                code = BASD_PNG_BAD_FILTER;
            if (code) {
                image_status[i] = code;
                status |= 1 << (code - 1);
            }
        }
        if (code) {
            memset(o, 0, (size_t)out_n);
            continue;
        }
        if (r.kind == BASD_PNG_KIND_RAW) {
            memcpy(o, src.p + r.src_offset, (size_t)out_n);
            continue;
        }
        const unsigned char* plte = src.p + (r.color_type == 3 ? r.plte_offset : 0);
        for (int y = 0; y < r.height; ++y) {            // every row is kept: the next one reads it as the row above
            unsigned char* line = lines + y * stride + 1;
            PngRow s = {line[-1], 0u, 0u, 0u};
            for (int x = 0; x < r.width; ++x) {
                const uint32_t up = y ? png_load_px(line - stride + (long)x * bpp, bpp) : 0u;
                png_unfilter_step(line, x, bpp, r.color_type, up, s, plte, o + 3L * y * r.width, true);
            }
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
