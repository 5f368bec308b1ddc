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
// basd_jpeg_decode_parallel swaps the entropy kernel for one that works inside a segment; basd_jpeg_decode_progressive
// puts one launch ahead of the three, which decodes the scans of progressive records (both further down).
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

// kMixed: the batch may hold progressive records, which jpeg_progressive_kernel has decoded: they are passed over and
// their status words left alone (basd_jpeg_decode_progressive).  Without it such a record is a bad record.
template <bool kMixed>
__global__ void __launch_bounds__(kJpegLanes) jpeg_entropy_kernel(JpegArgs a) {
    __shared__ JpegHuff tables[6];
    __shared__ uint32_t blocks[kJpegLanes * kJpegBlockPitch];
    __shared__ int failed;
    const int lane = threadIdx.x, img = blockIdx.x;
    const BasdJpegRecord r = a.table[img];
    if (kMixed && r.kind == BASD_JPEG_KIND_PROGRESSIVE) return;        // uniform over the workgroup
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
    if (r.kind != BASD_JPEG_KIND_STREAM && r.kind != BASD_JPEG_KIND_PROGRESSIVE) return;
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

// ---- the opt-in entropy stage that decodes INSIDE a segment in parallel (basd_jpeg_decode_parallel) ------------------
// One workgroup of kJpegParLanes lanes per image.  A segment is cut into sub-sequences of `sub_bytes`; a chunk is
// kJpegParLanes of them, one per lane, and chunks follow one another with the exact state carried in LDS.  Per chunk:
// every lane decodes its sub-sequence from a guessed state (a luma block begins at its first byte), lane 0 from the
// carried one; then rounds in which a lane whose predecessor's exit state differs from the state it last entered with
// decodes again (after round n the first n + 1 sub-sequences are exact whatever the stream holds); where a chunk has
// not settled after kJpegParRounds rounds, one lane's sweep through the sub-sequences that are not yet exact, so that a
// stream that never synchronises costs the serial time and not every lane's; a prefix sum of the block counts and the
// DC sums; and one more pass that stores the coefficients into the zeroed area.  The per-lane passes are jpeg_sub_pass of jpeg_core.h; here
// are only the barriers, the LDS records (one int array per field: lane l reads and writes word l) and the sums.  An
// image with at least kJpegLanes segments has its parallelism already and goes through jpeg_decode_segment, one
// segment per lane of the first wave, as in jpeg_entropy_kernel.
#ifndef BASD_JPEG_PAR_LANES
#define BASD_JPEG_PAR_LANES 256                                        // measured: profiles/jpeg_parallel.txt
#endif
constexpr int kJpegParLanes = BASD_JPEG_PAR_LANES;
constexpr int kJpegParWaves = kJpegParLanes / 64;
constexpr int kJpegParRounds = kJpegParLanes / 4;                      // synchronisation rounds ahead of the sweep
constexpr int kJpegParSubBytes = 128;                                  // sub_bytes == 0; measured, same file
static_assert(kJpegParLanes == 64 || kJpegParLanes == 128 || kJpegParLanes == 256, "whole waves, at most four");

struct JpegParShared {
    int exit_pos[kJpegParLanes], exit_rest[kJpegParLanes];             // the lanes' exit states
    unsigned swept[4][kJpegParLanes];                                  // blocks and DC sums of the lanes a sweep decoded for
    unsigned wave_sum[kJpegParWaves][4];                               // per wave: blocks, DC sums
    int carry_pos, carry_rest;                                         // into the next chunk: the state,
    unsigned carry_sum[4];                                             // the blocks begun and the predictors
    int again[2];                                                      // did a lane decode in this round (by parity)
    int first_error;                                                   // lane << 8 | code of the lowest lane that failed
};
static_assert(6 * sizeof(JpegHuff) + kJpegLanes * kJpegBlockPitch * 4 + sizeof(JpegParShared) <= 32 * 1024,
              "several images share a CU's LDS");

// Segment `seg` by the whole workgroup: 0 or a BASD_JPEG_BAD_* code, the same in every lane.
__device__ int jpeg_segment_parallel(const BasdJpegRecord& r, const JpegGeometry& g, const unsigned char* src, int seg,
                                     const JpegHuff* tables, short* coef, int sub_bytes, JpegParShared& sh) {
    const int lane = threadIdx.x, in_wave = lane & 63, wave = lane >> 6;
    int start, end;
    long first, last;
    const int bad = jpeg_segment_range(r, g, src, seg, start, end, first, last);
    if (bad) return bad;                                               // uniform
    const long nblocks = (last - first) * g.bpm;
    short* to = coef + first * g.bpm * 64;
    for (long i = lane; i < nblocks * 8; i += kJpegParLanes) ((uint4*)to)[i] = make_uint4(0, 0, 0, 0);
    if (lane == 0) {
        sh.carry_pos = start;
        sh.carry_rest = 0;
        sh.carry_sum[0] = sh.carry_sum[1] = sh.carry_sum[2] = sh.carry_sum[3] = 0;
        sh.first_error = 0x7fffffff;
    }
    __syncthreads();                                                   // the zeros are ahead of every coefficient
    JpegSubSegment sg;
    sg.src = src; sg.stream_at = r.src_offset; sg.end = end; sg.bpm = g.bpm; sg.luma = r.ncomp == 1 ? 1 : g.bpm - 2;
    sg.tables = tables;
    const long nsub = end - start > sub_bytes ? ((long)(end - start) + sub_bytes - 1) / sub_bytes : 1;
    for (long chunk = 0; chunk * kJpegParLanes < nsub; ++chunk) {
        const JpegSubState carried = {sh.carry_pos, sh.carry_rest};
        const unsigned c_blocks = sh.carry_sum[0], c_dc0 = sh.carry_sum[1], c_dc1 = sh.carry_sum[2], c_dc2 = sh.carry_sum[3];
        const long sub = chunk * kJpegParLanes + lane;
        const bool live = sub < nsub;
        const int sub_begin = live ? start + (int)(sub * sub_bytes) : end;
        const int sub_end = sub + 1 >= nsub ? kJpegSubOpenEnd : sub_begin + sub_bytes;
        // ---- speculate
        const JpegSubState guess = {sub_begin, live ? 0 : kJpegSubNone};
        JpegSubState entry = lane ? guess : carried;
        JpegSubPass pass = jpeg_sub_pass<false>(sg, entry, sub_end, nullptr, 0, 0, 0, 0, 0);
        sh.exit_pos[lane] = pass.exit.pos;
        sh.exit_rest[lane] = pass.exit.rest;
        if (lane == 0) sh.again[0] = sh.again[1] = 0;
        __syncthreads();
        // ---- synchronise: no lane leaves this loop on its own (the test is an LDS word read behind a barrier)
        bool settled = false;
        for (int round = 1; round <= kJpegParRounds; ++round) {
            JpegSubState want = entry;
            if (lane && live) {                                        // a predecessor that ran into garbage hands over nothing:
                want.pos = sh.exit_pos[lane - 1];                      // the lane then stays with its guess, and the
                want.rest = sh.exit_rest[lane - 1];                    // sub-sequences behind it can still fall into step
                if (want.rest == kJpegSubNone) want = guess;
            }
            __syncthreads();                                           // every exit state is read before one is replaced
            if (lane == 0) sh.again[(round + 1) & 1] = 0;
            if (!jpeg_sub_same(want, entry)) {
                entry = want;
                pass = jpeg_sub_pass<false>(sg, entry, sub_end, nullptr, 0, 0, 0, 0, 0);
                sh.exit_pos[lane] = pass.exit.pos;
                sh.exit_rest[lane] = pass.exit.rest;
                sh.again[round & 1] = 1;
            }
            __syncthreads();
            if (!sh.again[round & 1]) {                                // uniform
                settled = true;
                break;
            }
        }
        // ---- sweep: a chunk that has not settled by now belongs to a stream that does not fall into step (a flat
        // picture, blocks without an end-of-block code), and every further round would make one more sub-sequence exact
        // with all lanes decoding.  The sub-sequences 0 .. kJpegParRounds are exact; lane 0 walks through the others
        // once, in order, and the lanes take their states and counts from LDS.  The time stays within the bound of
        // kJpegParLanes passes (kJpegParRounds + 1 in parallel, at most kJpegParLanes - kJpegParRounds - 1 here).
        if (!settled) {                                                // uniform
            if (lane == 0) {
                for (int l = kJpegParRounds + 1; l < kJpegParLanes && chunk * kJpegParLanes + l < nsub; ++l) {
                    const long s = chunk * kJpegParLanes + l;
                    const int begin = start + (int)(s * sub_bytes);
                    JpegSubState in = {sh.exit_pos[l - 1], sh.exit_rest[l - 1]};
                    if (in.rest == kJpegSubNone) in = JpegSubState{begin, 0};
                    const JpegSubPass p = jpeg_sub_pass<false>(sg, in, s + 1 >= nsub ? kJpegSubOpenEnd : begin + sub_bytes,
                                                               nullptr, 0, 0, 0, 0, 0);
                    sh.exit_pos[l] = p.exit.pos;
                    sh.exit_rest[l] = p.exit.rest;
                    sh.swept[0][l] = (unsigned)p.blocks;
                    sh.swept[1][l] = p.dc[0]; sh.swept[2][l] = p.dc[1]; sh.swept[3][l] = p.dc[2];
                }
            }
            __syncthreads();
            if (lane > kJpegParRounds && live) {
                entry.pos = sh.exit_pos[lane - 1];
                entry.rest = sh.exit_rest[lane - 1];
                if (entry.rest == kJpegSubNone) entry = guess;
                pass.exit.pos = sh.exit_pos[lane];
                pass.exit.rest = sh.exit_rest[lane];
                pass.blocks = (int)sh.swept[0][lane];
                pass.dc[0] = sh.swept[1][lane]; pass.dc[1] = sh.swept[2][lane]; pass.dc[2] = sh.swept[3][lane];
            }
        }
        // ---- scan: inclusive in the wave, then the waves ahead
        unsigned v0 = (unsigned)pass.blocks, v1 = pass.dc[0], v2 = pass.dc[1], v3 = pass.dc[2];
        for (int d = 1; d < 64; d *= 2) {
            const unsigned t0 = __shfl_up(v0, d), t1 = __shfl_up(v1, d), t2 = __shfl_up(v2, d), t3 = __shfl_up(v3, d);
            if (in_wave >= d) { v0 += t0; v1 += t1; v2 += t2; v3 += t3; }
        }
        if (in_wave == 63) { sh.wave_sum[wave][0] = v0; sh.wave_sum[wave][1] = v1; sh.wave_sum[wave][2] = v2; sh.wave_sum[wave][3] = v3; }
        __syncthreads();
        for (int w = 0; w < kJpegParWaves; ++w)
            if (w < wave) { v0 += sh.wave_sum[w][0]; v1 += sh.wave_sum[w][1]; v2 += sh.wave_sum[w][2]; v3 += sh.wave_sum[w][3]; }
        v0 += c_blocks; v1 += c_dc0; v2 += c_dc1; v3 += c_dc2;          // inclusive, with what the chunks ahead carried
        // ---- write
        const JpegSubPass done = jpeg_sub_pass<true>(sg, entry, sub_end, to, (long)(v0 - (unsigned)pass.blocks), nblocks,
                                                     (int)(v1 - pass.dc[0]), (int)(v2 - pass.dc[1]), (int)(v3 - pass.dc[2]));
        if (done.error) atomicMin(&sh.first_error, (lane << 8) | done.error);
        if (lane == kJpegParLanes - 1) {
            sh.carry_pos = pass.exit.pos;
            sh.carry_rest = pass.exit.rest;
            sh.carry_sum[0] = v0; sh.carry_sum[1] = v1; sh.carry_sum[2] = v2; sh.carry_sum[3] = v3;
        }
        __syncthreads();
        const int error = sh.first_error, rest = sh.carry_rest;
        const unsigned begun = sh.carry_sum[0];
        __syncthreads();                                               // read by all before the next chunk or segment writes
        if (error != 0x7fffffff) return error & 255;                   // the two exits: an error of the write pass,
        if (jpeg_sub_complete(begun, nblocks, rest)) return 0;         // or the last block decoded to its end
    }
    // Not reached, kept so that the loop ends whatever happens: the last chunk's last live lane has no end, so its write
    // pass stops only at the block count or at an error, and one of the two exits above was taken.
    return BASD_JPEG_TRUNCATED;
}

template <bool kMixed>                                                 // as in jpeg_entropy_kernel
__global__ void __launch_bounds__(kJpegParLanes) jpeg_entropy_parallel_kernel(JpegArgs a, int sub_bytes) {
    __shared__ JpegHuff tables[6];
    __shared__ uint32_t blocks[kJpegLanes * kJpegBlockPitch];
    __shared__ JpegParShared sh;
    __shared__ int failed;
    const int lane = threadIdx.x, img = blockIdx.x;
    const BasdJpegRecord r = a.table[img];
    if (kMixed && r.kind == BASD_JPEG_KIND_PROGRESSIVE) return;        // uniform over the workgroup
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
        if (r.n_seg >= kJpegLanes) {                                   // uniform: a lane per segment, as the serial stage
            short* block = (short*)(blocks + (lane & (kJpegLanes - 1)) * kJpegBlockPitch);
            for (int seg = lane; seg < r.n_seg && lane < kJpegLanes; seg += kJpegLanes) {
                const int code = jpeg_decode_segment(r, g, a.src, seg, tables, block, coef);
                if (code) {
                    atomicMax(&failed, code);
                    break;
                }
            }
        } else {                                                       // fewer segments than the serial stage has lanes:
            int worst = 0;                                             // its status is the largest of their codes
            for (int seg = 0; seg < r.n_seg; ++seg) {
                const int code = jpeg_segment_parallel(r, g, a.src, seg, tables, coef, sub_bytes, sh);
                worst = code > worst ? code : worst;
            }
            if (lane == 0 && worst) failed = worst;
        }
    }
    __syncthreads();
    if (lane == 0) {
        *image_status = failed;
        if (failed) atomicOr(a.status, 1 << (failed - 1));
    }
}

// ---- progressive streams (basd_jpeg_decode_progressive; the scheme is in include/basd_hip.h) ----------------------------
// One workgroup of kJpegProgWaves waves per image.  The record and every row of its scan table are checked first; the
// rows then live in LDS.  The scans run level by level: scans of one level touch disjoint coefficients, so they run at
// the same time, kJpegProgWaves of them in a round, the n-th to wave n (scans of different kinds would serialise in one
// wave), and lane l of the wave takes the scan's segments l, l + 64, ...  Coefficients are read and written in place in
// the workspace; the barrier behind a round orders them for the next level's readers.  Every barrier is reached by
// every lane: what a round does depends on the rows in LDS alone.
constexpr int kJpegProgWaves = 8;                                    // Pillow's script has 5 scans in its first level, the
                                                                       // hand-made ones of the tests up to 7: one round each
constexpr int kJpegProgLanes = 64 * kJpegProgWaves;

struct JpegProgShared {
    JpegHuff tables[kJpegProgWaves][3];
    BasdJpegScan scans[BASD_JPEG_MAX_SCANS];
    int code[BASD_JPEG_MAX_SCANS];                                     // per scan: the largest code of its segments
    int failed_scan;                                                   // the first scan in stream order that failed
    int bad_rows, levels;
};
static_assert(sizeof(BasdJpegScan) == 64, "the scan table has 64-byte rows");
static_assert(sizeof(JpegProgShared) <= 48 * 1024, "three images share a CU's LDS");

__global__ void __launch_bounds__(kJpegProgLanes) jpeg_progressive_kernel(JpegArgs a, int max_scans, int max_segments) {
    __shared__ JpegProgShared sh;
    const int lane = threadIdx.x, in_wave = lane & 63, wave = lane >> 6, img = blockIdx.x;
    const BasdJpegRecord r = a.table[img];
    if (r.kind != BASD_JPEG_KIND_PROGRESSIVE) return;                  // uniform: the baseline stage's, or raw
    int* image_status = (int*)a.ws + img;
    const int bad = jpeg_check_progressive(r, a.src_bytes, a.out_bytes, a.ws_bytes, a.ws_reserved, max_scans);
    if (bad) {                                                         // uniform
        if (lane == 0) {
            *image_status = bad;
            atomicOr(a.status, 1 << (bad - 1));
        }
        return;
    }
    if (lane == 0) {
        sh.failed_scan = r.n_scans;
        sh.bad_rows = sh.levels = 0;
    }
    __syncthreads();
    if (lane < r.n_scans) {                                            // n_scans <= 64: one row per lane of wave 0
        BasdJpegScan s;
        __builtin_memcpy(&s, __builtin_assume_aligned(a.src + r.src_offset + r.scan_offset + 64L * lane, 8), 64);
        if (jpeg_check_scan(r, s, a.src_bytes, max_segments)) atomicMax(&sh.levels, s.level + 1);
        else atomicOr(&sh.bad_rows, 1);
        sh.scans[lane] = s;
        sh.code[lane] = 0;
    }
    __syncthreads();
    if (sh.bad_rows) {                                                 // uniform: no row is followed
        if (lane == 0) {
            *image_status = BASD_JPEG_BAD_RECORD;
            atomicOr(a.status, 1 << (BASD_JPEG_BAD_RECORD - 1));
        }
        return;
    }
    const JpegGeometry g = jpeg_geometry(r);
    short* coef = (short*)(a.ws + r.coef_offset);
    for (long i = lane; i < g.blocks * 8; i += kJpegProgLanes) ((uint4*)coef)[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();                                                   // the zeros are ahead of every coefficient
    const unsigned char* stream = a.src + r.src_offset;
    const int levels = sh.levels;
    for (int level = 0; level < levels; ++level) {
        for (int next = 0;;) {                                         // a round: the next kJpegProgWaves scans of the level
            int mine = -1, found = 0;
            for (; next < r.n_scans && found < kJpegProgWaves; ++next)
                if (sh.scans[next].level == level) {
                    if (found == wave) mine = next;
                    ++found;
                }
            if (found == 0) break;                                     // uniform
            // behind a failure in scan j only scans ahead of j may still matter
            const bool run = mine >= 0 && mine < sh.failed_scan;
            JpegHuff* tables = sh.tables[wave];
            if (run && in_wave < 3) {
                const BasdJpegScan& s = sh.scans[mine];
                bool ok = true;
                if (s.ss == 0 && s.ah == 0) {
                    if (in_wave < r.ncomp && (s.ncomp > 1 || in_wave == s.comp))
                        ok = jpeg_build_huff(stream, r.src_len, jpeg_pick(s.dc, in_wave), &tables[in_wave]);
                } else if (s.ss > 0 && in_wave == 0) {
                    ok = jpeg_build_huff(stream, r.src_len, s.ac, &tables[0]);
                }
                if (!ok) atomicMax(&sh.code[mine], BASD_JPEG_BAD_TABLE);
            }
            __syncthreads();                                           // failed_scan is written behind here, read ahead
            if (run && sh.code[mine] != 0) {                           // uniform over the wave: a bad table
                if (in_wave == 0) atomicMin(&sh.failed_scan, mine);
            } else if (run) {
                const BasdJpegScan s = sh.scans[mine];
                int row;
                if (!jpeg_scan_segments_ok(s, jpeg_scan_units(r, g, s, row))) {
                    if (in_wave == 0) {
                        atomicMax(&sh.code[mine], BASD_JPEG_BAD_RESTART);
                        atomicMin(&sh.failed_scan, mine);
                    }
                } else {
                    for (int seg = in_wave; seg < s.n_seg; seg += 64) {
                        const int code = jpeg_scan_segment(r, g, s, a.src, seg, tables, coef);
                        if (code) {                                    // the scan's other segments are still decoded
                            atomicMax(&sh.code[mine], code);
                            atomicMin(&sh.failed_scan, mine);
                        }
                    }
                }
            }
            __syncthreads();                                           // the round's coefficients are ahead of the next reader
        }
    }
    if (lane == 0) {
        const int failed = sh.failed_scan < r.n_scans ? sh.code[sh.failed_scan] : 0;
        *image_status = failed;
        if (failed) atomicOr(a.status, 1 << (failed - 1));
    }
}

}  // namespace basd

namespace {

// The argument rules shared by the three entry points, and the launches' common argument.
int jpeg_arguments(const unsigned char* src, long src_bytes, unsigned char* out, long out_bytes, int B,
                   const BasdJpegRecord* table, unsigned char* ws, long ws_bytes, int* status, long max_blocks,
                   long max_pixels, basd::JpegArgs& a) {
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
    a = basd::JpegArgs{};
    a.src = src; a.src_bytes = src_bytes; a.out = out; a.out_bytes = out_bytes; a.table = table;
    a.ws = ws; a.ws_bytes = ws_bytes; a.ws_reserved = reserved; a.status = status;
    return BASD_OK;
}

bool jpeg_sub_bytes_ok(int sub_bytes) {
    return sub_bytes == 0 ||
           (sub_bytes >= BASD_JPEG_SUB_BYTES_MIN && sub_bytes <= BASD_JPEG_SUB_BYTES_MAX && (sub_bytes & 7) == 0);
}

// The two launches behind every entropy stage (always both: a batch of raw records alone has no blocks: one idle
// workgroup per image).
void jpeg_idct_and_pixels(const basd::JpegArgs& a, int B, long max_blocks, long max_pixels, hipStream_t stream) {
    const long idct_groups = (max_blocks + basd::kJpegIdctBlock - 1) / basd::kJpegIdctBlock;
    const long pixel_groups = (max_pixels + basd::kJpegPixelBlock - 1) / basd::kJpegPixelBlock;
    basd::jpeg_idct_kernel<<<dim3((unsigned)(idct_groups > 0 ? idct_groups : 1), (unsigned)B), basd::kJpegIdctBlock, 0,
                             stream>>>(a);
    basd::jpeg_pixel_kernel<<<dim3((unsigned)(pixel_groups > 0 ? pixel_groups : 1), (unsigned)B), basd::kJpegPixelBlock,
                              0, stream>>>(a);
}

}  // namespace

extern "C" {

long basd_jpeg_status_bytes(int B) { return B < 0 ? 0 : ((long)B * 4 + 127) & ~127L; }

int basd_jpeg_decode(const unsigned char* src, long src_bytes, unsigned char* out, long out_bytes, int B,
                     const BasdJpegRecord* table, unsigned char* ws, long ws_bytes, int* status, long max_blocks,
                     long max_pixels, hipStream_t stream) {
    basd::JpegArgs a;
    BASD_TRY(jpeg_arguments(src, src_bytes, out, out_bytes, B, table, ws, ws_bytes, status, max_blocks, max_pixels, a));
    if (B == 0) return BASD_OK;
    basd::jpeg_entropy_kernel<false><<<(unsigned)B, basd::kJpegLanes, 0, stream>>>(a);
    jpeg_idct_and_pixels(a, B, max_blocks, max_pixels, stream);
    BASD_RETURN_LAST();
}

int basd_jpeg_decode_parallel(const unsigned char* src, long src_bytes, unsigned char* out, long out_bytes, int B,
                              const BasdJpegRecord* table, unsigned char* ws, long ws_bytes, int* status,
                              long max_blocks, long max_pixels, int sub_bytes, hipStream_t stream) {
    basd::JpegArgs a;
    BASD_CHECK_ARG(B >= 0 && jpeg_sub_bytes_ok(sub_bytes));
    BASD_TRY(jpeg_arguments(src, src_bytes, out, out_bytes, B, table, ws, ws_bytes, status, max_blocks, max_pixels, a));
    if (B == 0) return BASD_OK;
    basd::jpeg_entropy_parallel_kernel<false><<<(unsigned)B, basd::kJpegParLanes, 0, stream>>>(
        a, sub_bytes ? sub_bytes : basd::kJpegParSubBytes);
    jpeg_idct_and_pixels(a, B, max_blocks, max_pixels, stream);
    BASD_RETURN_LAST();
}

int basd_jpeg_decode_progressive(const unsigned char* src, long src_bytes, unsigned char* out, long out_bytes, int B,
                                 const BasdJpegRecord* table, unsigned char* ws, long ws_bytes, int* status,
                                 long max_blocks, long max_pixels, int sub_bytes, int parallel, int max_scans,
                                 int max_segments, hipStream_t stream) {
    basd::JpegArgs a;
    BASD_CHECK_ARG(B >= 0 && (parallel == 0 || parallel == 1) && jpeg_sub_bytes_ok(sub_bytes) &&
                   (parallel || sub_bytes == 0));
    BASD_CHECK_ARG(max_scans >= 0 && max_scans <= BASD_JPEG_MAX_SCANS && max_segments >= 0);
    BASD_TRY(jpeg_arguments(src, src_bytes, out, out_bytes, B, table, ws, ws_bytes, status, max_blocks, max_pixels, a));
    if (B == 0) return BASD_OK;
    // four launches: the progressive records' coefficients, the others' (which leaves those alone), idct, pixels
    basd::jpeg_progressive_kernel<<<(unsigned)B, basd::kJpegProgLanes, 0, stream>>>(a, max_scans, max_segments);
    if (parallel)
        basd::jpeg_entropy_parallel_kernel<true><<<(unsigned)B, basd::kJpegParLanes, 0, stream>>>(
            a, sub_bytes ? sub_bytes : basd::kJpegParSubBytes);
    else
        basd::jpeg_entropy_kernel<true><<<(unsigned)B, basd::kJpegLanes, 0, stream>>>(a);
    jpeg_idct_and_pixels(a, B, max_blocks, max_pixels, stream);
    BASD_RETURN_LAST();
}

}  // extern "C"
