// The per-image arithmetic of the JPEG decoder (specification: include/basd_hip.h) as host + device functions: the
// record check, the Huffman tables, the bit reader, one entropy-coded segment, the four kinds of progressive scan, the
// block IDCT, the upsampling taps and the colour formula.  csrc/jpeg.hip wraps them in kernels; tools/jpeg_host_check.cpp
// (and tools/jpeg_progressive_host_check.cpp) compile the same text for the host and run it under the sanitizers.  Nothing here allocates, and nothing reads or writes outside the ranges
// the record check has admitted.
#pragma once
#include <stdint.h>

#include "../../include/basd_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BASD_HD __host__ __device__ __forceinline__
#else
#define BASD_HD inline
#endif
#if defined(__clang__)
#define BASD_UNROLL _Pragma("unroll")
#else
#define BASD_UNROLL
#endif

namespace basd {

constexpr int kJpegLookBits = 9;

struct JpegHuff {                      // 1420 bytes
    unsigned short look[1 << kJpegLookBits];   // (length << 8) | value of the code the next 9 bits start with; 0: longer
    int maxcode[18];                   // per length the largest code, -1: none
    int valoff[17];                    // index of a code's value = valoff[length] + code
    unsigned char vals[256];
};

// ---- geometry ---------------------------------------------------------------------------------------------------
struct JpegGeometry {
    int mcux, mcuy, bpm;               // MCUs per row / column, blocks per MCU
    long mcus, blocks;
    int yw, yh, cw, ch;                // padded plane sizes (luma, chroma), multiples of 8
    int cwr, chr;                      // real chroma samples
};

BASD_HD JpegGeometry jpeg_geometry(const BasdJpegRecord& r) {
    JpegGeometry g;
    const int hs = r.ncomp == 1 ? 1 : r.hs, vs = r.ncomp == 1 ? 1 : r.vs;
    g.mcux = (r.width + 8 * hs - 1) / (8 * hs);
    g.mcuy = (r.height + 8 * vs - 1) / (8 * vs);
    g.bpm = r.ncomp == 1 ? 1 : hs * vs + 2;
    g.mcus = (long)g.mcux * g.mcuy;
    g.blocks = g.mcus * g.bpm;
    g.yw = g.mcux * hs * 8;
    g.yh = g.mcuy * vs * 8;
    g.cw = g.mcux * 8;
    g.ch = g.mcuy * 8;
    g.cwr = (r.width + hs - 1) / hs;
    g.chr = (r.height + vs - 1) / vs;
    return g;
}

// Is the image's output range inside the output?  (What the pixel kernel needs before it may zero a failed image.)
BASD_HD bool jpeg_out_ok(const BasdJpegRecord& r, long out_bytes) {
    if (r.width < 1 || r.height < 1 || r.width > BASD_JPEG_MAX_SIDE || r.height > BASD_JPEG_MAX_SIDE) return false;
    const long n = 3L * r.width * r.height;
    return r.out_offset >= 0 && r.out_offset <= out_bytes && n <= out_bytes - r.out_offset;
}

// The output range and the source range of a record (every kind has both).
BASD_HD bool jpeg_ranges_ok(const BasdJpegRecord& r, long src_bytes, long out_bytes) {
    if (!jpeg_out_ok(r, out_bytes)) return false;
    return !(r.src_len < 0 || r.src_len > 0x7fffffff - 16 || r.src_offset < 0 || r.src_offset > src_bytes ||
             r.src_len > src_bytes - r.src_offset);
}

// The frame of a stream, baseline or progressive: components, sampling, its places in the workspace, its DQT tables.
BASD_HD bool jpeg_frame_ok(const BasdJpegRecord& r, long ws_bytes, long ws_reserved) {
    if (r.ncomp != 1 && r.ncomp != 3) return false;
    if (r.ncomp == 3 && !((r.hs == 1 && r.vs == 1) || (r.hs == 2 && r.vs == 1) || (r.hs == 2 && r.vs == 2))) return false;
    const JpegGeometry g = jpeg_geometry(r);
    if (r.coef_offset < ws_reserved || (r.coef_offset & 15) || r.coef_offset > ws_bytes ||
        g.blocks * 128 > ws_bytes - r.coef_offset)
        return false;
    if (r.plane_offset < ws_reserved || (r.plane_offset & 7) || r.plane_offset > ws_bytes ||
        g.blocks * 64 > ws_bytes - r.plane_offset)
        return false;
    for (int c = 0; c < r.ncomp; ++c)
        if (r.quant[c] < 0 || r.quant[c] > r.src_len - 64) return false;
    return true;
}

// Every field of a record against the three buffers: 0, or BASD_JPEG_BAD_RECORD.  (A progressive record is one here:
// only basd_jpeg_decode_progressive takes it, through jpeg_check_progressive.)
BASD_HD int jpeg_check_record(const BasdJpegRecord& r, long src_bytes, long out_bytes, long ws_bytes, long ws_reserved) {
    if (!jpeg_ranges_ok(r, src_bytes, out_bytes)) return BASD_JPEG_BAD_RECORD;
    if (r.kind == BASD_JPEG_KIND_RAW) return (long)r.src_len == 3L * r.width * r.height ? 0 : BASD_JPEG_BAD_RECORD;
    if (r.kind != BASD_JPEG_KIND_STREAM) return BASD_JPEG_BAD_RECORD;
    if (!jpeg_frame_ok(r, ws_bytes, ws_reserved)) return BASD_JPEG_BAD_RECORD;
    if (r.restart < 0 || r.n_seg < 1) return BASD_JPEG_BAD_RECORD;
    if (r.seg_offset < 0 || (r.seg_offset & 3) || r.seg_offset > src_bytes || 4L * r.n_seg > src_bytes - r.seg_offset)
        return BASD_JPEG_BAD_RECORD;
    for (int c = 0; c < r.ncomp; ++c)
        if (r.dc[c] < 0 || r.dc[c] > r.src_len - 16 || r.ac[c] < 0 || r.ac[c] > r.src_len - 16)
            return BASD_JPEG_BAD_RECORD;
    return 0;
}

// ---- Huffman tables -----------------------------------------------------------------------------------------------
// The table whose 16 counts start at stream[off] (off <= len - 16 is the caller's); false: BASD_JPEG_BAD_TABLE.
BASD_HD bool jpeg_build_huff(const unsigned char* stream, int len, int off, JpegHuff* h) {
    int total = 0;
    for (int l = 1; l <= 16; ++l) total += stream[off + l - 1];
    if (total > 256 || total > len - off - 16) return false;
    for (int i = 0; i < (1 << kJpegLookBits); ++i) h->look[i] = 0;
    const unsigned char* vals = stream + off + 16;
    int code = 0, p = 0;
    h->maxcode[0] = -1;
    for (int l = 1; l <= 16; ++l) {
        const int n = stream[off + l - 1];
        if (code + n > (1 << l)) return false;                        // not a prefix code
        h->valoff[l] = p - code;
        for (int i = 0; i < n; ++i, ++p, ++code) {
            const unsigned char v = vals[p];
            h->vals[p] = v;
            if (l <= kJpegLookBits) {
                const int first = code << (kJpegLookBits - l);        // < 2^9: code < 2^l
                for (int j = 0; j < (1 << (kJpegLookBits - l)); ++j) h->look[first + j] = (unsigned short)((l << 8) | v);
            }
        }
        h->maxcode[l] = n ? code - 1 : -1;
        code <<= 1;
    }
    h->maxcode[17] = 0x7fffffff;
    return true;
}

// ---- the bit reader -------------------------------------------------------------------------------------------
// Reads the bytes [pos, end) behind `base` (8-byte aligned; positions are 32-bit and count from it) through aligned
// 8-byte words of the byte buffer.  The buffer is a multiple of 16 bytes long and 16-byte aligned, so a word that holds
// a byte of the range lies inside it; bytes of a word outside the range are never looked at.  Up to 64 bits wait in
// `acc`, left-aligned; a refill takes four bytes at once where none of them is FF, single bytes otherwise.
struct JpegBits {
    const unsigned char* base;
    int pos, end;
    uint64_t word, ahead;              // the word that holds base[pos], and the one after it
    uint64_t acc;
    int nbits;                         // valid bits of acc; below zero: more bits were taken than the data has
    bool more;                         // bytes are left (no marker met, end not reached)
};

BASD_HD uint64_t jpeg_load_word(const JpegBits& b, int at) {
    // `at` is a multiple of 8; a word that starts at or past `end` holds nothing of the range and is not read
    uint64_t w = 0;
    if (at < b.end) __builtin_memcpy(&w, __builtin_assume_aligned(b.base + at, 8), 8);
    return w;
}

// [begin, begin + len) of the byte buffer `src`; len <= 2^31 - 17
BASD_HD void jpeg_bits_open(JpegBits& b, const unsigned char* src, long begin, int len) {
    const long at = begin & ~7L;
    b.base = src + at;
    b.pos = (int)(begin - at);
    b.end = b.pos + len;
    b.acc = 0;
    b.nbits = 0;
    b.more = len > 0;
    b.word = jpeg_load_word(b, 0);
    b.ahead = jpeg_load_word(b, 8);
}

BASD_HD void jpeg_bits_advance(JpegBits& b, int n) {    // pos += n (n <= 4), into the next word where it crosses
    const int next = b.pos + n;
    if ((next ^ b.pos) & 8) {
        b.word = b.ahead;
        b.ahead = jpeg_load_word(b, (next & ~7) + 8);
    }
    b.pos = next;
}

BASD_HD void jpeg_bits_fill(JpegBits& b) {              // to more than 31 bits, where the data has them
    if (b.nbits >= 32 || !b.more) return;
    if (b.pos + 4 <= b.end && b.nbits >= 0) {
        const int sh = 8 * (b.pos & 7);
        const uint32_t w = (uint32_t)((b.word >> sh) | ((b.ahead << 1) << (63 - sh)));       // base[pos .. pos + 4)
        if (((~w - 0x01010101u) & w & 0x80808080u) == 0) {                 // no byte of w can be FF
            b.acc |= (uint64_t)__builtin_bswap32(w) << (32 - b.nbits);
            b.nbits += 32;
            jpeg_bits_advance(b, 4);
            return;
        }
    }
    while (b.nbits <= 56 && b.more) {
        if (b.pos >= b.end) { b.more = false; break; }
        const unsigned v = (unsigned)(b.word >> (8 * (b.pos & 7))) & 255u;
        jpeg_bits_advance(b, 1);
        if (v == 0xFF) {
            if (b.pos >= b.end) { b.more = false; break; }
            const unsigned next = (unsigned)(b.word >> (8 * (b.pos & 7))) & 255u;
            if (next != 0) { b.more = false; break; }                 // a marker: the data ends here
            jpeg_bits_advance(b, 1);                                  // the stuffed zero
        }
        b.acc |= (uint64_t)v << (56 - b.nbits);
        b.nbits += 8;
    }
}

BASD_HD unsigned jpeg_bits_peek(const JpegBits& b, int n) { return (uint32_t)(b.acc >> 32) >> (32 - n); }   // 1 <= n <= 16
BASD_HD void jpeg_bits_skip(JpegBits& b, int n) {
    b.acc <<= n;
    b.nbits -= n;
}

// One symbol: >= 0, or -BASD_JPEG_BAD_CODE.  At least 16 bits (or all that are left) wait in acc.
BASD_HD int jpeg_symbol(JpegBits& b, const JpegHuff* h) {
    const unsigned e = h->look[jpeg_bits_peek(b, kJpegLookBits)];
    if (e) {
        jpeg_bits_skip(b, (int)(e >> 8));
        return (int)(e & 255u);
    }
    for (int l = kJpegLookBits + 1; l <= 16; ++l) {
        const int code = (int)jpeg_bits_peek(b, l);
        if (code <= h->maxcode[l]) {
            jpeg_bits_skip(b, l);
            const int at = h->valoff[l] + code;
            return at >= 0 && at < 256 ? h->vals[at] : -BASD_JPEG_BAD_CODE;
        }
    }
    return -BASD_JPEG_BAD_CODE;
}

BASD_HD int jpeg_extend(JpegBits& b, int s) {           // 1 <= s <= 15
    const int v = (int)jpeg_bits_peek(b, s);
    jpeg_bits_skip(b, s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// One block into block[64] (int16 in the stream's zigzag order, zeroed here): 0 or a BASD_JPEG_BAD_* code.  A symbol
// and its value bits are at most 31 bits: one refill ahead of each symbol.
BASD_HD int jpeg_decode_block(JpegBits& b, const JpegHuff* dc, const JpegHuff* ac, int& pred, short* block) {
    __builtin_memset(__builtin_assume_aligned(block, 4), 0, 128);
    jpeg_bits_fill(b);
    int s = jpeg_symbol(b, dc);
    if (b.nbits < 0) return BASD_JPEG_TRUNCATED;                      // the bits of the symbol were padding
    if (s < 0) return -s;
    if (s > 15) return BASD_JPEG_BAD_CODE;
    if (s) pred += jpeg_extend(b, s);
    if (b.nbits < 0) return BASD_JPEG_TRUNCATED;
    if (pred < -32768 || pred > 32767) return BASD_JPEG_BAD_VALUE;
    block[0] = (short)pred;
    for (int k = 1; k < 64;) {
        jpeg_bits_fill(b);
        const int rs = jpeg_symbol(b, ac);
        if (b.nbits < 0) return BASD_JPEG_TRUNCATED;
        if (rs < 0) return -rs;
        const int r = rs >> 4;
        s = rs & 15;
        if (s) {
            k += r;
            if (k > 63) return BASD_JPEG_BAD_INDEX;
            block[k] = (short)jpeg_extend(b, s);
            ++k;
        } else if (r == 15) {
            k += 16;
        } else {
            break;
        }
    }
    return b.nbits < 0 ? BASD_JPEG_TRUNCATED : 0;
}

// Segment `seg` of an image whose record has passed jpeg_check_record: its MCUs, block by block, through `block`
// (64 int16 of the caller's) into the coefficient area.  0 or a BASD_JPEG_BAD_* code.
BASD_HD int jpeg_decode_segment(const BasdJpegRecord& r, const JpegGeometry& g, const unsigned char* src, int seg,
                                const JpegHuff* tables, short* block, short* coef) {
    const unsigned char* stream = src + r.src_offset;
    int start, end = r.src_len + 2;
    __builtin_memcpy(&start, __builtin_assume_aligned(src + r.seg_offset + 4L * seg, 4), 4);
    if (seg + 1 < r.n_seg) __builtin_memcpy(&end, __builtin_assume_aligned(src + r.seg_offset + 4L * (seg + 1), 4), 4);
    if (end < 2) return BASD_JPEG_BAD_RESTART;
    end -= 2;
    if (start < 2 || start > r.src_len || end < start || end > r.src_len) return BASD_JPEG_BAD_RESTART;
    if (seg > 0 && (stream[start - 2] != 0xFF || stream[start - 1] != 0xD0 + ((seg - 1) & 7)))
        return BASD_JPEG_BAD_RESTART;
    const long per = r.restart > 0 ? r.restart : g.mcus;
    const long first = (long)seg * per;
    const long last = first + per < g.mcus ? first + per : g.mcus;
    JpegBits b;
    jpeg_bits_open(b, src, r.src_offset + start, end - start);
    const int luma = r.ncomp == 1 ? 1 : g.bpm - 2;
    int pred_y = 0, pred_cb = 0, pred_cr = 0;
    short* to = coef + first * g.bpm * 64;
    for (long m = first; m < last; ++m) {
        for (int j = 0; j < g.bpm; ++j, to += 64) {
            const int bad = j < luma        ? jpeg_decode_block(b, tables, tables + 3, pred_y, block)
                            : j == luma     ? jpeg_decode_block(b, tables + 1, tables + 4, pred_cb, block)
                                            : jpeg_decode_block(b, tables + 2, tables + 5, pred_cr, block);
            if (bad) return bad;
            __builtin_memcpy(__builtin_assume_aligned(to, 16), __builtin_assume_aligned(block, 4), 128);
        }
    }
    return 0;
}

// Does the record's segment count fit its frame?
BASD_HD bool jpeg_segments_ok(const BasdJpegRecord& r, const JpegGeometry& g) {
    const long want = r.restart > 0 ? (g.mcus + r.restart - 1) / r.restart : 1;
    return (long)r.n_seg == want;
}

// ---- decoding inside a segment in parallel (basd_jpeg_decode_parallel) -----------------------------------------------
// A segment's bytes are cut into sub-sequences of `sub_bytes`; one lane decodes one sub-sequence, first from a guessed
// state, then again from the state its predecessor handed over, until nothing changes (csrc/jpeg.hip holds the rounds,
// the barriers and the prefix sums; tools/jpeg_parallel_host_check.cpp runs the same functions as loops).  What is
// handed over is CANONICAL: it names a bit of the stream, not a state of the reader, so two decoders that stand at the
// same bit hand over equal states whatever their refills were.
//   pos    offset in the stream of the first byte of which no bit has been taken (a stuffed 00 counts to its FF);
//   rest   k | j << 6 | rem << 9 | bits << 12: the zigzag index of the next coefficient (0: a block begins), the slot of
//          the block in its MCU, how many bits of the data byte ahead of `pos` are still to be taken, and those bits
//          (so a decoder that resumes never looks behind `pos`); -1: no state (a bad code, or the data ran out).
struct JpegSubState {
    int pos, rest;
};
constexpr int kJpegSubNone = -1;
constexpr int kJpegSubOpenEnd = 0x7fffffff;              // `sub_end` of a segment's last sub-sequence: it has no end

BASD_HD bool jpeg_sub_same(const JpegSubState& a, const JpegSubState& b) { return a.pos == b.pos && a.rest == b.rest; }

// What one pass of a lane over its sub-sequence gives.
struct JpegSubPass {
    JpegSubState exit;
    int blocks;                        // blocks that BEGAN in the sub-sequence
    unsigned dc[3];                    // count pass: per component the sum of the DC differences met (modulo 2^32: a
                                       // true prefix of them is a predictor and fits 16 bits); write pass: unused
    int error;                         // write pass: 0 or the BASD_JPEG_BAD_* code the serial decoder meets here
};

// One segment's constants for the passes.
struct JpegSubSegment {
    const unsigned char* src;          // the byte buffer
    long stream_at;                    // r.src_offset
    int end;                           // offset in the stream at which the segment's data ends
    int bpm, luma;                     // blocks per MCU; slot of the Cb block (slots below it are luma)
    const JpegHuff* tables;
};

// The range of segment `seg`, the checks of jpeg_decode_segment: 0 or BASD_JPEG_BAD_RESTART.
BASD_HD int jpeg_segment_range(const BasdJpegRecord& r, const JpegGeometry& g, const unsigned char* src, int seg,
                               int& start, int& end, long& first, long& last) {
    const unsigned char* stream = src + r.src_offset;
    end = r.src_len + 2;
    __builtin_memcpy(&start, __builtin_assume_aligned(src + r.seg_offset + 4L * seg, 4), 4);
    if (seg + 1 < r.n_seg) __builtin_memcpy(&end, __builtin_assume_aligned(src + r.seg_offset + 4L * (seg + 1), 4), 4);
    if (end < 2) return BASD_JPEG_BAD_RESTART;
    end -= 2;
    if (start < 2 || start > r.src_len || end < start || end > r.src_len) return BASD_JPEG_BAD_RESTART;
    if (seg > 0 && (stream[start - 2] != 0xFF || stream[start - 1] != 0xD0 + ((seg - 1) & 7)))
        return BASD_JPEG_BAD_RESTART;
    const long per = r.restart > 0 ? r.restart : g.mcus;
    first = (long)seg * per;
    last = first + per < g.mcus ? first + per : g.mcus;
    return 0;
}

// A reader that resumes at the bit `s` names; `bias`: what to add to b.pos to get an offset in the stream.
BASD_HD void jpeg_sub_open(JpegBits& b, int& bias, const JpegSubSegment& g, const JpegSubState& s) {
    jpeg_bits_open(b, g.src, g.stream_at + s.pos, g.end - s.pos);
    bias = s.pos - b.pos;
    const int rem = (s.rest >> 9) & 7;
    if (rem) {
        b.acc = (uint64_t)((s.rest >> 12) & 127) << (64 - rem);
        b.nbits = rem;
    }
}

// The bit the reader stands at (b.nbits >= 0), as the `pos`, `rem` and `bits` of a JpegSubState.  Whole bytes that
// wait in `acc` are pushed back: each is one byte of the stream, or two where it is FF (its stuffed 00).  `opened`:
// b.pos at jpeg_sub_open.  Once the data has ended on an FF that is not followed by 00, b.pos stands behind that FF.
BASD_HD void jpeg_sub_tell(const JpegBits& b, int bias, int opened, int& pos, int& rem, int& bits) {
    int fed = b.pos;
    if (!b.more && fed > opened && b.base[fed - 1] == 0xFF) --fed;     // an FF that was taken is followed by its 00
    rem = b.nbits & 7;
    bits = rem ? (int)(b.acc >> (64 - rem)) : 0;
    const uint64_t whole = ~(b.acc << rem);                            // the waiting bytes, inverted (behind them: FF)
    const uint64_t low = 0x7f7f7f7f7f7f7f7fULL;
    const uint64_t not_ff = (((whole & low) + low) | whole) & ~low;     // bit 7 of every byte that was not FF
    pos = fed + bias - (b.nbits >> 3) - (8 - __builtin_popcountll(not_ff));
}

// Has a segment of `nblocks` blocks been decoded to its end, given the blocks begun up to a chunk's end and the state
// handed over there by passes that do not know the block count?  More blocks begun: the last one ended (what follows
// is padding read as a block).  Exactly `nblocks` begun: it ended if the next symbol is a DC symbol (index 0), or if
// there is no state -- the last block itself was decoded without an error by the write pass (the caller has seen to
// that), so what failed is the symbol behind it.  Else the block runs on into the next chunk.
BASD_HD bool jpeg_sub_complete(unsigned begun, long nblocks, int rest) {
    if ((long)begun != nblocks) return (long)begun > nblocks;
    return rest == kJpegSubNone || (rest & 63) == 0;
}

BASD_HD int jpeg_sub_rest(int j, int k, int rem, int bits) { return k | (j << 6) | (rem << 9) | (bits << 12); }

// One pass of a lane: from state `in` up to the first symbol that begins at or behind `sub_end` (a symbol of whose first
// byte bits are left begins in that byte; kJpegSubOpenEnd: no end).  kWrite false (speculation and synchronisation):
// nothing is written, `blocks` and `dc` are counted, and whatever goes wrong only makes the exit state kJpegSubNone.
// kWrite true: `in` is the true state; block `block_at` (index in the segment) is the first that begins here, `pred`
// the predictors ahead of it; coefficients are stored one by one into the zeroed area `coef` (the segment's), a block
// at or past `block_end` is never begun, and an error is the serial decoder's.
template <bool kWrite>
BASD_HD JpegSubPass jpeg_sub_pass(const JpegSubSegment& g, JpegSubState in, int sub_end, short* coef, long block_at,
                                  long block_end, int pred0, int pred1, int pred2) {
    JpegSubPass out = {};
    out.exit.pos = 0;
    out.exit.rest = kJpegSubNone;
    if (in.rest == kJpegSubNone) return out;
    int j = (in.rest >> 6) & 7, k = in.rest & 63;
    short* to = coef;                                                  // the block under way (write pass)
    if (kWrite) {
        if ((k ? block_at - 1 : block_at) >= block_end) return out;   // the segment's blocks ended ahead of this lane
        if (k && block_at < 1) return out;                             // (a true state inside a block follows its beginning)
        to = coef + (block_at - 1) * 64;                               // looked at only where k > 0
    }
    JpegBits b;
    int bias;
    jpeg_sub_open(b, bias, g, in);
    const int opened = b.pos;
    int bad = 0;
    for (;;) {
        jpeg_bits_fill(b);
        if (b.pos + bias >= sub_end) {                                 // else the bytes fed, and so the bit ahead, lie before it
            int pos, rem, bits;
            jpeg_sub_tell(b, bias, opened, pos, rem, bits);
            if (pos - (rem ? 1 : 0) >= sub_end) {
                out.exit.pos = pos;
                out.exit.rest = jpeg_sub_rest(j, k, rem, bits);
                return out;
            }
        }
        const int c = j < g.luma ? 0 : j == g.luma ? 1 : 2;
        if (k == 0) {
            if (kWrite && block_at + out.blocks >= block_end) return out;     // the segment is complete: padding follows
            int s = jpeg_symbol(b, g.tables + c);
            if (b.nbits < 0) { bad = BASD_JPEG_TRUNCATED; break; }
            if (s < 0) { bad = -s; break; }
            if (s > 15) { bad = BASD_JPEG_BAD_CODE; break; }
            const int diff = s ? jpeg_extend(b, s) : 0;
            if (b.nbits < 0) { bad = BASD_JPEG_TRUNCATED; break; }
            if (kWrite) {
                int& pred = c == 0 ? pred0 : c == 1 ? pred1 : pred2;
                pred += diff;
                if (pred < -32768 || pred > 32767) { bad = BASD_JPEG_BAD_VALUE; break; }
                to = coef + (block_at + out.blocks) * 64;
                to[0] = (short)pred;
            } else {
                out.dc[c] += (unsigned)diff;
            }
            ++out.blocks;
            k = 1;
            continue;
        }
        const int rs = jpeg_symbol(b, g.tables + 3 + c);
        if (b.nbits < 0) { bad = BASD_JPEG_TRUNCATED; break; }
        if (rs < 0) { bad = -rs; break; }
        const int s = rs & 15;
        if (s) {
            k += rs >> 4;
            if (k > 63) { bad = BASD_JPEG_BAD_INDEX; break; }
            const int v = jpeg_extend(b, s);
            if (b.nbits < 0) { bad = BASD_JPEG_TRUNCATED; break; }
            if (kWrite) to[k] = (short)v;
            ++k;
        } else if ((rs >> 4) == 15) {
            k += 16;
        } else {
            k = 64;
        }
        if (k > 63) {                                                  // the block is complete
            k = 0;
            j = j + 1 == g.bpm ? 0 : j + 1;
        }
    }
    if (kWrite) out.error = bad;
    return out;
}

// ---- progressive streams (basd_jpeg_decode_progressive) -----------------------------------------------------------------
// The record of a progressive stream against the buffers, its scan table included (not yet the rows: jpeg_check_scan):
// 0, or BASD_JPEG_BAD_RECORD.
BASD_HD int jpeg_check_progressive(const BasdJpegRecord& r, long src_bytes, long out_bytes, long ws_bytes, long ws_reserved,
                                   int max_scans) {
    if (r.kind != BASD_JPEG_KIND_PROGRESSIVE || !jpeg_ranges_ok(r, src_bytes, out_bytes) ||
        !jpeg_frame_ok(r, ws_bytes, ws_reserved))
        return BASD_JPEG_BAD_RECORD;
    if (r.n_scans < 1 || r.n_scans > BASD_JPEG_MAX_SCANS || r.n_scans > max_scans) return BASD_JPEG_BAD_RECORD;
    const long at = r.src_offset + (long)r.scan_offset;
    if (r.scan_offset < 0 || (at & 7) || at > src_bytes || (long)sizeof(BasdJpegScan) * r.n_scans > src_bytes - at)
        return BASD_JPEG_BAD_RECORD;
    return 0;
}

BASD_HD int jpeg_pick(const int v[3], int c);            // (below)

// Row `s` of a scan table whose record has passed jpeg_check_progressive: is every field inside its bounds?
BASD_HD bool jpeg_check_scan(const BasdJpegRecord& r, const BasdJpegScan& s, long src_bytes, int max_segments) {
    if (s.n_seg < 1 || s.n_seg > max_segments || s.restart < 0) return false;
    const long at = r.src_offset + (long)s.seg_offset;
    if (s.seg_offset < 0 || (at & 3) || at > src_bytes || 4L * s.n_seg > src_bytes - at) return false;
    if (s.data_end < 0 || s.data_end > r.src_len) return false;
    if (s.comp < 0 || s.comp >= r.ncomp || !(s.ncomp == 1 || (s.ncomp == r.ncomp && s.comp == 0))) return false;
    if (s.al < 0 || s.al > 13 || s.ah < 0 || s.ah > 14 || s.level < 0 || s.level >= r.n_scans) return false;
    if (s.ss == 0) {
        if (s.se != 0) return false;
        if (s.ah == 0)
            for (int c = 0; c < r.ncomp; ++c)
                if ((s.ncomp > 1 || c == s.comp) && (jpeg_pick(s.dc, c) < 0 || jpeg_pick(s.dc, c) > r.src_len - 16)) return false;
    } else {
        if (s.ss < 1 || s.se < s.ss || s.se > 63 || s.ncomp != 1) return false;
        if (s.ac < 0 || s.ac > r.src_len - 16) return false;
    }
    return true;
}

// The scan units of a scan (MCUs of an interleaved scan, the component's own blocks otherwise) and, for a one-component
// scan, the blocks in a row of its grid.
BASD_HD long jpeg_scan_units(const BasdJpegRecord& r, const JpegGeometry& g, const BasdJpegScan& s, int& row) {
    if (s.ncomp > 1) {
        row = g.mcux;
        return g.mcus;
    }
    const int cw = s.comp == 0 ? r.width : g.cwr, ch = s.comp == 0 ? r.height : g.chr;
    row = (cw + 7) / 8;
    return (long)row * ((ch + 7) / 8);
}

BASD_HD bool jpeg_scan_segments_ok(const BasdJpegScan& s, long units) {
    return (long)s.n_seg == (s.restart > 0 ? (units + s.restart - 1) / s.restart : 1);
}

// Block (bx, by) of component `comp`'s own grid: its index in the interleaved order of the coefficient area.
BASD_HD long jpeg_component_block(const BasdJpegRecord& r, const JpegGeometry& g, int comp, int bx, int by) {
    if (r.ncomp == 1) return (long)by * g.mcux + bx;
    if (comp) return ((long)by * g.mcux + bx) * g.bpm + (g.bpm - 3 + comp);
    return ((long)(by / r.vs) * g.mcux + bx / r.hs) * g.bpm + (by % r.vs) * r.hs + bx % r.hs;
}

BASD_HD int jpeg_bit(JpegBits& b) {                     // one bit; b.nbits < 0 behind it: the data had none
    if (b.nbits <= 0) jpeg_bits_fill(b);
    const int v = (int)(b.acc >> 63);
    jpeg_bits_skip(b, 1);
    return v;
}

// The four kinds of scan on one block (64 int16 in zigzag order, in the coefficient area): 0 or a BASD_JPEG_BAD_* code.
BASD_HD int jpeg_prog_dc_first(JpegBits& b, const JpegHuff* dc, int& pred, int al, short* block) {
    jpeg_bits_fill(b);
    const int s = jpeg_symbol(b, dc);
    if (b.nbits < 0) return BASD_JPEG_TRUNCATED;
    if (s < 0) return -s;
    if (s > 15) return BASD_JPEG_BAD_VALUE;
    if (s) pred += jpeg_extend(b, s);
    if (b.nbits < 0) return BASD_JPEG_TRUNCATED;
    if (pred < -32768 || pred > 32767) return BASD_JPEG_BAD_VALUE;
    block[0] = (short)(unsigned short)(pred * (1 << al));             // wraps to 16 bits
    return 0;
}

BASD_HD int jpeg_prog_dc_refine(JpegBits& b, int al, short* block) {
    if (jpeg_bit(b)) block[0] = (short)(block[0] | (1 << al));
    return b.nbits < 0 ? BASD_JPEG_TRUNCATED : 0;
}

BASD_HD int jpeg_prog_ac_first(JpegBits& b, const JpegHuff* ac, int ss, int se, int al, int& eobrun, short* block) {
    if (eobrun > 0) {
        --eobrun;
        return 0;
    }
    for (int k = ss; k <= se;) {
        jpeg_bits_fill(b);
        const int rs = jpeg_symbol(b, ac);
        if (b.nbits < 0) return BASD_JPEG_TRUNCATED;
        if (rs < 0) return -rs;
        const int r = rs >> 4, s = rs & 15;
        if (s) {
            k += r;
            if (k > se) return BASD_JPEG_BAD_INDEX;
            block[k] = (short)(unsigned short)(jpeg_extend(b, s) * (1 << al));
            ++k;
        } else if (r == 15) {
            k += 16;
        } else {
            eobrun = (1 << r) - 1;
            if (r) {
                eobrun += (int)jpeg_bits_peek(b, r);
                jpeg_bits_skip(b, r);
            }
            break;
        }
    }
    return b.nbits < 0 ? BASD_JPEG_TRUNCATED : 0;
}

BASD_HD void jpeg_prog_correct(JpegBits& b, short* at, int p1) {
    const int v = *at;
    if (jpeg_bit(b) && !(v & p1)) *at = (short)(unsigned short)(v + (v >= 0 ? p1 : -p1));
}

BASD_HD int jpeg_prog_ac_refine(JpegBits& b, const JpegHuff* ac, int ss, int se, int al, int& eobrun, short* block) {
    const int p1 = 1 << al;
    int k = ss;
    if (eobrun == 0) {
        while (k <= se) {
            jpeg_bits_fill(b);
            const int rs = jpeg_symbol(b, ac);
            if (b.nbits < 0) return BASD_JPEG_TRUNCATED;
            if (rs < 0) return -rs;
            int r = rs >> 4, value = 0;
            if (rs & 15) {
                if ((rs & 15) != 1) return BASD_JPEG_BAD_CODE;
                value = jpeg_bit(b) ? p1 : -p1;
            } else if (r != 15) {
                eobrun = 1 << r;
                if (r) {
                    eobrun += (int)jpeg_bits_peek(b, r);
                    jpeg_bits_skip(b, r);
                }
                break;
            }
            for (; k <= se; ++k) {                                     // the walk
                if (block[k]) jpeg_prog_correct(b, block + k, p1);
                else if (--r < 0) break;
            }
            if (b.nbits < 0) return BASD_JPEG_TRUNCATED;
            if (value) {
                if (k > se) return BASD_JPEG_BAD_INDEX;
                block[k] = (short)value;
            }
            ++k;
        }
    }
    if (eobrun > 0) {
        for (; k <= se; ++k)
            if (block[k]) jpeg_prog_correct(b, block + k, p1);
        --eobrun;
    }
    return b.nbits < 0 ? BASD_JPEG_TRUNCATED : 0;
}

// Segment `seg` of scan `s` (its row has passed jpeg_check_scan and its segment count jpeg_scan_segments_ok), in place
// in the coefficient area `coef`; `tables`: DC first scans, the table of FRAME component c at tables[c]; AC scans, the
// table at tables[0].  0 or a BASD_JPEG_BAD_* code.
BASD_HD int jpeg_scan_segment(const BasdJpegRecord& r, const JpegGeometry& g, const BasdJpegScan& s,
                              const unsigned char* src, int seg, const JpegHuff* tables, short* coef) {
    const unsigned char* stream = src + r.src_offset;
    const unsigned char* starts = stream + s.seg_offset;
    int start, end = s.data_end + 2;
    __builtin_memcpy(&start, __builtin_assume_aligned(starts + 4L * seg, 4), 4);
    if (seg + 1 < s.n_seg) __builtin_memcpy(&end, __builtin_assume_aligned(starts + 4L * (seg + 1), 4), 4);
    if (end < 2) return BASD_JPEG_BAD_RESTART;
    end -= 2;
    if (start < 2 || start > r.src_len || end < start || end > r.src_len) return BASD_JPEG_BAD_RESTART;
    if (seg > 0 && (stream[start - 2] != 0xFF || stream[start - 1] != 0xD0 + ((seg - 1) & 7)))
        return BASD_JPEG_BAD_RESTART;
    int row;
    const long units = jpeg_scan_units(r, g, s, row);
    const long per = s.restart > 0 ? s.restart : units;
    const long first = (long)seg * per;
    const long last = first + per < units ? first + per : units;
    JpegBits b;
    jpeg_bits_open(b, src, r.src_offset + start, end - start);
    const int luma = r.ncomp == 1 ? 1 : g.bpm - 2;
    const int per_unit = s.ncomp > 1 ? g.bpm : 1;
    int pred0 = 0, pred1 = 0, pred2 = 0, eobrun = 0;
    for (long u = first; u < last; ++u) {
        for (int j = 0; j < per_unit; ++j) {
            int c = s.comp;
            long at = u * g.bpm + j;
            if (s.ncomp > 1) c = j < luma ? 0 : j == luma ? 1 : 2;
            else at = jpeg_component_block(r, g, c, (int)(u % row), (int)(u / row));
            short* block = coef + at * 64;
            int bad;
            if (s.ss == 0 && s.ah == 0)
                bad = jpeg_prog_dc_first(b, tables + c, c == 0 ? pred0 : c == 1 ? pred1 : pred2, s.al, block);
            else if (s.ss == 0)
                bad = jpeg_prog_dc_refine(b, s.al, block);
            else if (s.ah == 0)
                bad = jpeg_prog_ac_first(b, tables, s.ss, s.se, s.al, eobrun, block);
            else
                bad = jpeg_prog_ac_refine(b, tables, s.ss, s.se, s.al, eobrun, block);
            if (bad) return bad;
        }
    }
    return 0;
}

// ---- IDCT ---------------------------------------------------------------------------------------------------------
BASD_HD void jpeg_idct_1d(const int64_t c[8], int64_t out[8]) {
    int64_t z1 = (c[2] + c[6]) * 4433;
    const int64_t t2 = z1 - c[6] * 15137, t3 = z1 + c[2] * 6270;
    const int64_t t0 = (c[0] + c[4]) * 8192, t1 = (c[0] - c[4]) * 8192;
    const int64_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    int64_t a0 = c[7], a1 = c[5], a2 = c[3], a3 = c[1];
    z1 = a0 + a3;
    int64_t z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const int64_t z5 = (z3 + z4) * 9633;
    a0 *= 2446; a1 *= 16819; a2 *= 25172; a3 *= 12299;
    z1 *= -7373; z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
    out[0] = t10 + a3; out[7] = t10 - a3;
    out[1] = t11 + a2; out[6] = t11 - a2;
    out[2] = t12 + a1; out[5] = t12 - a1;
    out[3] = t13 + a0; out[4] = t13 - a0;
}

// coef: 64 int16 and q: the table's 64 bytes, both in zigzag order (unzig: where the coefficient of a place in the block
// sits in them; every index is a constant once the loops are unrolled); dst: 8 rows of 8 bytes, `pitch` apart.
BASD_HD void jpeg_idct_block(const short* coef, const unsigned char* q, unsigned char* dst, long pitch) {
    const unsigned char unzig[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                                     41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                                     46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};
    int ws[64];
    BASD_UNROLL
    for (int x = 0; x < 8; ++x) {
        int64_t c[8], o[8];
        BASD_UNROLL
        for (int y = 0; y < 8; ++y) c[y] = (int64_t)coef[unzig[8 * y + x]] * (int64_t)q[unzig[8 * y + x]];
        jpeg_idct_1d(c, o);
        BASD_UNROLL
        for (int y = 0; y < 8; ++y) ws[8 * y + x] = (int)((o[y] + 1024) >> 11);
    }
    BASD_UNROLL
    for (int y = 0; y < 8; ++y) {
        int64_t c[8], o[8];
        BASD_UNROLL
        for (int x = 0; x < 8; ++x) c[x] = ws[8 * y + x];
        jpeg_idct_1d(c, o);
        uint32_t lo = 0, hi = 0;
        BASD_UNROLL
        for (int x = 0; x < 8; ++x) {
            int64_t v = ((o[x] + 131072) >> 18) + 128;
            v = v < 0 ? 0 : v > 255 ? 255 : v;
            if (x < 4) lo |= (uint32_t)v << (8 * x);
            else hi |= (uint32_t)v << (8 * (x - 4));
        }
        const uint64_t row = (uint64_t)lo | ((uint64_t)hi << 32);     // 8-byte aligned: the pitch is a multiple of 8
        __builtin_memcpy(__builtin_assume_aligned(dst + y * pitch, 8), &row, 8);
    }
}

BASD_HD int jpeg_pick(const int v[3], int c) { return c == 0 ? v[0] : c == 1 ? v[1] : v[2]; }   // v[c] without an indexed read

// Block `blk` (scan order) of an image: where its 8 x 8 samples go, and which table dequantises it.
BASD_HD void jpeg_block_place(const BasdJpegRecord& r, const JpegGeometry& g, long blk, int& comp, long& offset,
                              int& pitch) {
    const long m = blk / g.bpm;
    const int j = (int)(blk - m * g.bpm);
    const int mx = (int)(m % g.mcux), my = (int)(m / g.mcux);
    const int hs = r.ncomp == 1 ? 1 : r.hs, vs = r.ncomp == 1 ? 1 : r.vs;
    if (j < hs * vs) {
        comp = 0;
        pitch = g.yw;
        offset = ((long)(my * vs + j / hs) * 8) * g.yw + (long)(mx * hs + j % hs) * 8;
    } else {
        comp = j - hs * vs + 1;
        pitch = g.cw;
        offset = (long)g.yw * g.yh + (long)(comp - 1) * g.cw * g.ch + ((long)my * 8) * g.cw + (long)mx * 8;
    }
}

// ---- pixels -------------------------------------------------------------------------------------------------------
BASD_HD int jpeg_clamp(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// The upsampled chroma sample at luma position (x, y) of a plane `p` (pitch g.cw, g.cwr x g.chr real samples).
BASD_HD int jpeg_upsample(const BasdJpegRecord& r, const JpegGeometry& g, const unsigned char* p, int x, int y) {
    if (r.hs == 1) return p[(long)y * g.cw + x];
    const int i = x >> 1, n = g.cwr;
    if (r.vs == 1) {
        const unsigned char* row = p + (long)y * g.cw;
        if (n <= 2) return row[i];
        if (x == 0) return row[0];
        if (x == 2 * n - 1) return row[n - 1];
        return (x & 1) ? (3 * row[i] + row[i + 1] + 2) >> 2 : (3 * row[i] + row[i - 1] + 1) >> 2;
    }
    const int rr = y >> 1;
    if (n <= 2) return p[(long)rr * g.cw + i];
    int nb = (y & 1) ? rr + 1 : rr - 1;
    nb = nb < 0 ? 0 : nb > g.chr - 1 ? g.chr - 1 : nb;
    const unsigned char* a = p + (long)rr * g.cw;
    const unsigned char* c = p + (long)nb * g.cw;
    const int cs = 3 * a[i] + c[i];
    if (x == 0) return (4 * cs + 8) >> 4;
    if (x == 2 * n - 1) return (4 * cs + 7) >> 4;
    if (x & 1) return (3 * cs + (3 * a[i + 1] + c[i + 1]) + 7) >> 4;
    return (3 * cs + (3 * a[i - 1] + c[i - 1]) + 8) >> 4;
}

// Pixel (x, y) of a decoded image from its planes, as R | G << 8 | B << 16.
BASD_HD unsigned jpeg_pixel(const BasdJpegRecord& r, const JpegGeometry& g, const unsigned char* planes, int x, int y) {
    const int Y = planes[(long)y * g.yw + x];
    if (r.ncomp == 1) return (unsigned)Y * 0x010101u;
    const unsigned char* pcb = planes + (long)g.yw * g.yh;
    const unsigned char* pcr = pcb + (long)g.cw * g.ch;
    const int cb = jpeg_upsample(r, g, pcb, x, y) - 128, cr = jpeg_upsample(r, g, pcr, x, y) - 128;
    const int R = jpeg_clamp(Y + ((91881 * cr + 32768) >> 16));
    const int B = jpeg_clamp(Y + ((116130 * cb + 32768) >> 16));
    const int G = jpeg_clamp(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
    return (unsigned)R | ((unsigned)G << 8) | ((unsigned)B << 16);
}

}  // namespace basd
