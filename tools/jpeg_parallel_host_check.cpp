// The parallel entropy stage of csrc/jpeg.hip (basd_jpeg_decode_parallel) on the host, as a stand-alone program: the
// lanes' passes are the functions of csrc/jpeg_core.h that the kernel calls, run here lane after lane and phase by
// phase (speculate, the synchronisation rounds, the prefix sums, write), in buffers of exactly the batch's sizes, so a
// sanitizer build (-fsanitize=address,undefined) sees every read and write the kernels would make.
//
//   jpeg_parallel_host_check IN OUT LANES SUB_BYTES
//
// IN and OUT: the files of tools/jpeg_host_check.cpp (same format).  LANES: 1..1024 sub-sequences per chunk; SUB_BYTES:
// a multiple of 8 in BASD_JPEG_SUB_BYTES_MIN .. BASD_JPEG_SUB_BYTES_MAX.  As the kernel, an image of 64 segments or
// more goes through jpeg_decode_segment.
// Standard output: per image that was decoded in chunks "image I chunks C max_rounds R swept S" (S of its chunks went
// through the sweep; a chunk's rounds: the first pass, every round in which a lane decoded again, of which there are
// at most LANES / 4, and the sweep by one lane that follows where the chunk has not settled by then), then
// "rounds N: C chunks" per count, "swept_chunks C" and
// "max_rounds R".  In every chunk the program also holds the handover to its word: a sub-sequence entered from its true
// state, and entered one sub-sequence earlier (another reader, other refills), must hand over equal states; if not it
// says so on standard error and exits with status 3.
// Exit status 0 whatever the streams hold (a bad stream is a status word, not a failure); 2 for a bad call.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "../vit-inductive-bias-distillation_amd/csrc/jpeg_core.h"

using namespace basd;

namespace {

constexpr long long kMagic = 0x4745504a44534142LL;
constexpr int kSerialSegments = 64;    // kJpegLanes of csrc/jpeg.hip

struct Buffer {                        // malloc'ed to the byte: 16-byte aligned, and the sanitizer guards both ends
    unsigned char* p = nullptr;
    long n = 0;
    explicit Buffer(long bytes) : p((unsigned char*)malloc(bytes > 0 ? (size_t)bytes : 1)), n(bytes) {}
    ~Buffer() { free(p); }
};

long status_bytes(long B) { return (B * 4 + 127) & ~127L; }

int lanes = 0, sub_bytes = 0;
std::map<int, long> histogram;         // rounds -> chunks
int image_rounds = 0;
long image_chunks = 0, image_swept = 0, swept_chunks = 0;

struct Lane {
    JpegSubState guess, entry;
    JpegSubPass pass;
    int sub_end;
    bool live;
};

[[noreturn]] void handover_differs(int seg, long sub, const JpegSubState& a, const JpegSubState& b) {
    fprintf(stderr, "segment %d, sub-sequence %ld: exit state (%d, %#x) from its own entry, (%d, %#x) from the one ahead\n",
            seg, sub, a.pos, (unsigned)a.rest, b.pos, (unsigned)b.rest);
    exit(3);
}

// jpeg_segment_parallel, the lanes one after the other
int segment(const BasdJpegRecord& r, const JpegGeometry& g, const unsigned char* src, int seg, const JpegHuff* tables,
            short* coef) {
    int start, end;
    long first, last;
    const int bad = jpeg_segment_range(r, g, src, seg, start, end, first, last);
    if (bad) return bad;
    const long nblocks = (last - first) * g.bpm;
    short* to = coef + first * g.bpm * 64;
    memset(to, 0, (size_t)nblocks * 128);
    JpegSubSegment sg;
    sg.src = src; sg.stream_at = r.src_offset; sg.end = end; sg.bpm = g.bpm; sg.luma = r.ncomp == 1 ? 1 : g.bpm - 2;
    sg.tables = tables;
    const long nsub = end - start > sub_bytes ? ((long)(end - start) + sub_bytes - 1) / sub_bytes : 1;
    JpegSubState carried = {start, 0};
    unsigned carry[4] = {0, 0, 0, 0};
    std::vector<Lane> lane((size_t)lanes);
    std::vector<JpegSubState> want((size_t)lanes);
    for (long chunk = 0; chunk * lanes < nsub; ++chunk) {
        for (int l = 0; l < lanes; ++l) {                              // speculate
            Lane& t = lane[l];
            const long sub = chunk * lanes + l;
            t.live = sub < nsub;
            const int sub_begin = t.live ? start + (int)(sub * sub_bytes) : end;
            t.sub_end = sub + 1 >= nsub ? kJpegSubOpenEnd : sub_begin + sub_bytes;
            t.guess = {sub_begin, t.live ? 0 : kJpegSubNone};
            t.entry = l ? t.guess : carried;
            t.pass = jpeg_sub_pass<false>(sg, t.entry, t.sub_end, nullptr, 0, 0, 0, 0, 0);
        }
        int rounds = 1;
        bool settled = false;
        const int sync_rounds = lanes / 4;                             // kJpegParRounds
        for (int round = 1; round <= sync_rounds; ++round) {           // synchronise
            for (int l = 0; l < lanes; ++l) {
                want[l] = l && lane[l].live ? lane[l - 1].pass.exit : lane[l].entry;
                if (l && lane[l].live && want[l].rest == kJpegSubNone) want[l] = lane[l].guess;
            }
            bool again = false;                                        // (the barrier: all are read before one is replaced)
            for (int l = 0; l < lanes; ++l) {
                Lane& t = lane[l];
                if (jpeg_sub_same(want[l], t.entry)) continue;
                t.entry = want[l];
                t.pass = jpeg_sub_pass<false>(sg, t.entry, t.sub_end, nullptr, 0, 0, 0, 0, 0);
                again = true;
            }
            if (!again) {
                settled = true;
                break;
            }
            ++rounds;
        }
        if (!settled) {                                                // sweep: what lane 0 does for the lanes behind the exact ones
            for (int l = sync_rounds + 1; l < lanes && lane[l].live; ++l) {
                Lane& t = lane[l];
                t.entry = lane[l - 1].pass.exit.rest == kJpegSubNone ? t.guess : lane[l - 1].pass.exit;
                t.pass = jpeg_sub_pass<false>(sg, t.entry, t.sub_end, nullptr, 0, 0, 0, 0, 0);
            }
            ++rounds;
            ++swept_chunks;
            ++image_swept;
        }
        ++histogram[rounds];
        ++image_chunks;
        if (rounds > image_rounds) image_rounds = rounds;
        // the handover is canonical: sub-sequence l entered from its true state, and reached by a reader that was opened
        // one sub-sequence earlier, end in equal states
        for (int l = 1; l < lanes; ++l) {
            if (!lane[l].live || lane[l - 1].pass.exit.rest == kJpegSubNone) continue;
            const JpegSubPass through = jpeg_sub_pass<false>(sg, lane[l - 1].entry, lane[l].sub_end, nullptr, 0, 0, 0, 0, 0);
            if (!jpeg_sub_same(through.exit, lane[l].pass.exit))
                handover_differs(seg, chunk * lanes + l, lane[l].pass.exit, through.exit);
        }
        int error = 0;
        for (int l = 0; l < lanes; ++l) {                              // scan and write
            const Lane& t = lane[l];
            const JpegSubPass done = jpeg_sub_pass<true>(sg, t.entry, t.sub_end, to, (long)carry[0], nblocks,
                                                         (int)carry[1], (int)carry[2], (int)carry[3]);
            if (done.error && !error) error = done.error;              // the lowest lane's
            carry[0] += (unsigned)t.pass.blocks;
            for (int c = 0; c < 3; ++c) carry[1 + c] += t.pass.dc[c];
        }
        carried = lane[(size_t)lanes - 1].pass.exit;
        if (error) return error;
        if (jpeg_sub_complete(carry[0], nblocks, carried.rest)) return 0;
    }
    fprintf(stderr, "segment %d: the last chunk ended without an error and before the last block\n", seg);
    exit(3);                                                           // the kernel's guard: never taken
}

// jpeg_entropy_parallel_kernel
int entropy(const BasdJpegRecord& r, const unsigned char* src, long src_bytes, long out_bytes, unsigned char* ws,
            long ws_bytes, long reserved, long image) {
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
    short* coef = (short*)(ws + r.coef_offset);
    if (r.n_seg >= kSerialSegments) {
        alignas(16) short block[64];
        for (int l = 0; l < kSerialSegments; ++l)
            for (int seg = l; seg < r.n_seg; seg += kSerialSegments) {
                const int code = jpeg_decode_segment(r, g, src, seg, tables.data(), block, coef);
                if (code) {
                    if (code > failed) failed = code;
                    break;
                }
            }
        return failed;
    }
    image_rounds = 0;
    image_chunks = 0;
    image_swept = 0;
    for (int seg = 0; seg < r.n_seg; ++seg) {
        const int code = segment(r, g, src, seg, tables.data(), coef);
        if (code > failed) failed = code;
    }
    printf("image %ld chunks %ld max_rounds %d swept %ld\n", image, image_chunks, image_rounds, image_swept);
    return failed;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 5) return 2;
    lanes = atoi(argv[3]);
    sub_bytes = atoi(argv[4]);
    if (lanes < 1 || lanes > 1024 || sub_bytes < BASD_JPEG_SUB_BYTES_MIN || sub_bytes > BASD_JPEG_SUB_BYTES_MAX ||
        (sub_bytes & 7))
        return 2;
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
        const int code = entropy(table[b], src.p, src_bytes, out_bytes, ws.p, ws_bytes, reserved, b);
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
    int most = 0;
    for (const auto& [rounds, chunks] : histogram) {
        printf("rounds %d: %ld chunks\n", rounds, chunks);
        most = rounds;
    }
    printf("swept_chunks %ld\n", swept_chunks);
    printf("max_rounds %d\n", most);
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(out.p, 1, (size_t)out_bytes, f);
    fwrite(image_status, 4, (size_t)B, f);
    fwrite(&status, 4, 1, f);
    fclose(f);
    return 0;
}
