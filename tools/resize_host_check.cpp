// The resize's per-axis code (csrc/resize_core.h) compiled for the host, as a stand-alone program: it runs the record
// check, the taps and the two passes of csrc/resize.hip as plain loops over a record table, in buffers of exactly the
// needed sizes, so a sanitizer build (-fsanitize=address,undefined -ffp-contract=off) sees every read and write and
// every integer operation the specification asks for.
//
//   resize_host_check IN OUT
//
// IN:  8 int64 (magic 0x5a53524444534142, n, src_bytes, C, OH, OW, 0, 0), n records of 64 bytes, the src_bytes bytes of
//      the packed images (tests/test_resize_filters.py writes the file).
// OUT: the n * C * OH * OW output bytes (planar, as the launch writes them), one int32 status word.
// Exit status 0 whatever the records hold (a bad record is a status bit and zeros, not a failure); 2 for a bad IN file.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../vit-inductive-bias-distillation_amd/csrc/resize_core.h"

using namespace basd;

namespace {

constexpr long long kMagic = 0x5a53524444534142LL;

struct Buffer {                        // malloc'ed to the byte: the sanitizer guards both ends
    unsigned char* p = nullptr;
    long n = 0;
    explicit Buffer(long bytes) : p((unsigned char*)malloc(bytes > 0 ? (size_t)bytes : 1)), n(bytes) {}
    ~Buffer() { free(p); }
    Buffer(const Buffer&) = delete;
    Buffer& operator=(const Buffer&) = delete;
};

// The taps of `count` output indices from `first` on: spans[i] and k + i * ksize, each in a buffer of its exact size.
struct Axis {
    int ksize;
    Buffer spans, k;
    Axis(int in, int out, int first, int count, int filter)
        : ksize(resize_ksize(in, out, filter)), spans((long)count * (long)sizeof(ResizeSpan)),
          k((long)count * ksize * (long)sizeof(int)) {
        for (int i = 0; i < count; ++i) span(i) = resize_taps(in, out, first + i, ksize, filter, taps(i));
    }
    ResizeSpan& span(int i) { return ((ResizeSpan*)spans.p)[i]; }
    int* taps(int i) { return (int*)k.p + (long)i * ksize; }
};

void resize_record(const BasdResizeRecord& r, const unsigned char* src, int C, int OH, int OW, unsigned char* d) {
    Axis hx(r.win_w, r.res_w, r.out_x, OW, r.filter), vy(r.win_h, r.res_h, r.out_y, OH, r.filter);
    const unsigned char* window = src + r.src_offset + ((long)r.win_y * r.src_w + r.win_x) * C;
    const long src_pitch = (long)r.src_w * C;
    // horizontal: the source rows the vertical taps need (first taps and ends do not decrease), planar per row
    const int row0 = vy.span(0).first;
    const int nsrc = vy.span(OH - 1).first + vy.span(OH - 1).count - row0;
    const long pitch = (long)C * OW;
    Buffer stage(nsrc * pitch);
    for (int rr = 0; rr < nsrc; ++rr)
        for (int col = 0; col < OW; ++col) {
            const ResizeSpan t = hx.span(col);
            const int* k = hx.taps(col);
            const unsigned char* p = window + (long)(row0 + rr) * src_pitch + (long)t.first * C;
            for (int c = 0; c < C; ++c) {
                int acc = 1 << 21;
                for (int j = 0; j < t.count; ++j) acc += k[j] * (int)p[(long)C * j + c];
                stage.p[rr * pitch + (long)c * OW + col] = (unsigned char)resize_clip(acc);
            }
        }
    // vertical
    for (int y = 0; y < OH; ++y) {
        const ResizeSpan t = vy.span(y);
        const int* k = vy.taps(y);
        for (int c = 0; c < C; ++c)
            for (int col = 0; col < OW; ++col) {
                int acc = 1 << 21;
                const unsigned char* q = stage.p + (t.first - row0) * pitch + (long)c * OW + col;
                for (int j = 0; j < t.count; ++j) acc += k[j] * (int)q[j * pitch];
                d[((long)c * OH + y) * OW + col] = (unsigned char)resize_clip(acc);
            }
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    long long head[8];
    if (fread(head, 8, 8, f) != 8 || head[0] != kMagic) return 2;
    const long n = head[1], src_bytes = head[2];
    const int C = (int)head[3], OH = (int)head[4], OW = (int)head[5];
    if (n < 0 || n > 65536 || src_bytes < 0 || (C != 1 && C != 3) || head[4] < 1 || head[5] < 1 || head[4] > 4096 ||
        head[5] > 4096)
        return 2;
    std::vector<BasdResizeRecord> table((size_t)n);
    const long chw = (long)C * OH * OW;
    Buffer src(src_bytes), out(n * chw);
    if (!src.p || !out.p) return 2;
    if (n && fread(table.data(), sizeof(BasdResizeRecord), (size_t)n, f) != (size_t)n) return 2;
    if (src_bytes && fread(src.p, 1, (size_t)src_bytes, f) != (size_t)src_bytes) return 2;
    fclose(f);
    memset(out.p, 0xA5, (size_t)(n * chw));            // what a record does not write stays recognisable
    int status = 0;
    for (long i = 0; i < n; ++i) {
        const int bad = resize_check(table[i], src_bytes, C, OH, OW);
        if (bad) {
            status |= bad;
            memset(out.p + i * chw, 0, (size_t)chw);
            continue;
        }
        resize_record(table[i], src.p, C, OH, OW, out.p + i * chw);
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(out.p, 1, (size_t)(n * chw), f);
    fwrite(&status, 4, 1, f);
    fclose(f);
    return 0;
}
