// The per-image code of the PNG decoder (specification: include/basd_hip.h) as host + device functions: the record
// check, the Huffman tables, the bit reader, one deflate block, the match copy, the Adler-32 sums and one pixel's
// unfilter.  Every function that several lanes work on takes (lane, lanes): csrc/png.hip calls them with a wave's 64
// lanes, tools/png_host_check.cpp compiles the same text for the host and calls them with lanes = 1 under the
// sanitizers.  Nothing here allocates, and nothing reads or writes outside the ranges the record check has admitted.
#pragma once
#include <stdint.h>

#include "../../include/basd_hip.h"

#ifndef BASD_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define BASD_HD __host__ __device__ __forceinline__
#else
#define BASD_HD inline
#endif
#endif
// Orders what the lanes of the (one-wave) workgroup wrote to LDS or to the workspace ahead of what they read next.
#if defined(__HIP_DEVICE_COMPILE__)
#define BASD_PNG_SYNC() __syncthreads()
#else
#define BASD_PNG_SYNC() ((void)0)
#endif

namespace basd {

constexpr int kPngLookBits = 9;
constexpr int kPngWindow = 32768;                  // deflate's largest distance
constexpr int kPngMaxSyms = 288;

struct PngHuff {                                   // 2276 bytes
    unsigned short look[1 << kPngLookBits];        // (length << 9) | symbol of the code the next 9 bits begin with; 0: none
    unsigned short count[16];                      // codes per length
    unsigned short offs[16], next[16];             // lane 0's cursors while it assigns the codes
    unsigned short symbol[kPngMaxSyms];            // the symbols ordered by (length, symbol)
    unsigned short code[kPngMaxSyms];              // a symbol's canonical code
    int bad;                                       // the lengths are no code
};

struct PngInflateShared {                          // 39,948 bytes: LDS on the device
    PngHuff lit, dist, clen;
    unsigned char clens[32];                       // the 19 lengths of the code-length code
    unsigned char lens[320];                       // up to 286 + 30 lengths (288 + 32 of the fixed codes)
    unsigned char window[kPngWindow];              // byte i of the output sits at i % 32768
};

// ---- the record -------------------------------------------------------------------------------------------------
BASD_HD int png_bpp(int color_type) {
    return color_type == 0 ? 1 : color_type == 2 ? 3 : color_type == 3 ? 1 : color_type == 4 ? 2 : color_type == 6 ? 4 : 0;
}

BASD_HD bool png_out_ok(const BasdPngRecord& r, long out_bytes) {
    if (r.width < 1 || r.height < 1 || r.width > BASD_PNG_MAX_SIDE || r.height > BASD_PNG_MAX_SIDE) return false;
    const long n = 3L * r.width * r.height;
    return r.out_offset >= 0 && r.out_offset <= out_bytes && n <= out_bytes - r.out_offset;
}

// bytes of the filtered scanlines (the sides are in range): at most 16384 * 65537 < 2^31
BASD_HD long png_filtered_bytes(const BasdPngRecord& r) {
    return (long)r.height * ((long)r.width * png_bpp(r.color_type) + 1);
}

// Every field of a record against the three buffers: 0, or BASD_PNG_BAD_RECORD.
BASD_HD int png_check_record(const BasdPngRecord& r, long src_bytes, long out_bytes, long ws_bytes, long ws_reserved) {
    if (!png_out_ok(r, out_bytes)) return BASD_PNG_BAD_RECORD;
    if (r.src_len < 0 || r.src_len > 0x7fffffff - 16 || r.src_offset < 0 || r.src_offset > src_bytes ||
        r.src_len > src_bytes - r.src_offset)
        return BASD_PNG_BAD_RECORD;
    if (r.kind == BASD_PNG_KIND_RAW) return (long)r.src_len == 3L * r.width * r.height ? 0 : BASD_PNG_BAD_RECORD;
    if (r.kind != BASD_PNG_KIND_STREAM || png_bpp(r.color_type) == 0) return BASD_PNG_BAD_RECORD;
    if (r.ws_offset < ws_reserved || (r.ws_offset & 15) || r.ws_offset > ws_bytes ||
        png_filtered_bytes(r) > ws_bytes - r.ws_offset)
        return BASD_PNG_BAD_RECORD;
    if (r.color_type == 3 && (r.plte_offset < 0 || r.plte_offset > src_bytes || 768 > src_bytes - r.plte_offset))
        return BASD_PNG_BAD_RECORD;
    return 0;
}

// ---- the bit reader -------------------------------------------------------------------------------------------
// Bits of p[pos .. len), least significant first.  acc holds nbits valid bits; whatever it holds above them is what
// the stream holds there (zeros past its end), so OR-ing a byte in twice does no harm.  A drop of more bits than are
// left sets `over` (BASD_PNG_TRUNCATED for the caller) and leaves zeros.
struct PngBits {
    const unsigned char* p;
    int pos, len;
    uint64_t acc;
    int nbits, over;
};

BASD_HD void png_bits_open(PngBits& b, const unsigned char* p, int begin, int len) {
    b.p = p;
    b.len = len;
    b.pos = begin < len ? begin : len;
    b.acc = 0;
    b.nbits = 0;
    b.over = 0;
}

BASD_HD void png_fill(PngBits& b) {                // to at least 56 bits, where the stream has them
    if (b.pos + 8 <= b.len) {
        uint64_t w;
        __builtin_memcpy(&w, b.p + b.pos, 8);
        b.acc |= w << b.nbits;                      // nbits <= 63
        const int n = (63 - b.nbits) >> 3;
        b.pos += n;
        b.nbits += 8 * n;
    } else {
        while (b.nbits <= 56 && b.pos < b.len) {
            b.acc |= (uint64_t)b.p[b.pos++] << b.nbits;
            b.nbits += 8;
        }
    }
}

BASD_HD void png_drop(PngBits& b, int n) {
    if (n > b.nbits) {
        b.over = 1;
        b.acc = 0;
        b.nbits = 0;
    } else {
        b.acc >>= n;
        b.nbits -= n;
    }
}

BASD_HD unsigned png_take(PngBits& b, int n) {      // n <= 16, behind a png_fill
    const unsigned v = (unsigned)b.acc & ((1u << n) - 1u);
    png_drop(b, n);
    return v;
}

// ---- Huffman tables -----------------------------------------------------------------------------------------------
BASD_HD unsigned png_reverse(unsigned code, int len) {
    unsigned r = 0;
    for (int i = 0; i < len; ++i) r |= ((code >> i) & 1u) << (len - 1 - i);
    return r;
}

// The code of lens[0 .. n) (each <= 15) into h; `codes`: the code-length code, which must be complete.  h.bad says
// whether the lengths are a code; it is the same in every lane behind the call.
BASD_HD void png_build_huff(PngHuff& h, const unsigned char* lens, int n, bool codes, int lane, int lanes) {
    BASD_PNG_SYNC();                                // the lengths are written, the old table is no longer read
    for (int i = lane; i < (1 << kPngLookBits); i += lanes) h.look[i] = 0;
    if (lane == 0) {
        for (int l = 0; l < 16; ++l) h.count[l] = 0;
        for (int s = 0; s < n; ++s) h.count[lens[s]]++;
        int left = 1, longest = 0, bad = 0;
        for (int l = 1; l <= 15; ++l) {
            left = 2 * left - h.count[l];
            if (left < 0) {
                bad = 1;                            // over-subscribed
                break;
            }
            if (h.count[l]) longest = l;
        }
        if (!bad && left > 0 && (codes || longest > 1)) bad = 1;       // incomplete
        h.bad = bad;
        if (!bad) {
            unsigned at = 0, code = 0;
            h.count[0] = 0;
            for (int l = 1; l <= 15; ++l) {
                code = (code + h.count[l - 1]) << 1;
                h.offs[l] = (unsigned short)at;
                h.next[l] = (unsigned short)code;
                at += h.count[l];
            }
            for (int s = 0; s < n; ++s) {
                const int l = lens[s];
                if (l) {
                    h.symbol[h.offs[l]++] = (unsigned short)s;
                    h.code[s] = h.next[l]++;
                }
            }
        }
    }
    BASD_PNG_SYNC();
    if (!h.bad) {
        for (int s = lane; s < n; s += lanes) {
            const int l = lens[s];
            if (l && l <= kPngLookBits) {
                const unsigned short entry = (unsigned short)((l << 9) | s);
                for (unsigned k = png_reverse(h.code[s], l); k < (1u << kPngLookBits); k += 1u << l) h.look[k] = entry;
            }
        }
    }
    BASD_PNG_SYNC();
}

// The next symbol, behind a png_fill; -1 (and 15 bits taken) where the bits begin with no code.
BASD_HD int png_symbol(PngBits& b, const PngHuff& h) {
    const unsigned bits = (unsigned)b.acc & 0x7fffu;
    const unsigned e = h.look[bits & ((1u << kPngLookBits) - 1u)];
    if (e) {
        png_drop(b, (int)(e >> 9));
        return (int)(e & 511u);
    }
    int code = 0, first = 0, index = 0;
    for (int l = 1; l <= 15; ++l) {
        code |= (int)((bits >> (l - 1)) & 1u);
        const int count = h.count[l];
        if (code - count < first) {
            png_drop(b, l);
            return h.symbol[index + (code - first)];
        }
        index += count;
        first = (first + count) << 1;
        code <<= 1;
    }
    png_drop(b, 15);
    return -1;
}

BASD_HD int png_order(int i) {                     // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, 5 bits each
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 |
                        10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (int)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31u);
}

// ---- the copies ---------------------------------------------------------------------------------------------------
// Byte pos + j of the match is byte pos - dist + j % dist: always a byte from before the match, so the lanes need no
// order among themselves, only behind the bytes written before (the sync).  1 <= dist <= pos, dist <= 32768.
BASD_HD void png_match(unsigned char* dst, unsigned char* window, int pos, int dist, int len, int lane, int lanes) {
    BASD_PNG_SYNC();
    for (int j = lane; j < len; j += lanes) {
        const unsigned char v = window[(pos - dist + j % dist) & (kPngWindow - 1)];
        window[(pos + j) & (kPngWindow - 1)] = v;
        dst[pos + j] = v;
    }
}

BASD_HD void png_stored(unsigned char* dst, unsigned char* window, int pos, const unsigned char* from, int len, int lane,
                        int lanes) {
    for (int j = lane; j < len; j += lanes) {
        const unsigned char v = from[j];
        window[(pos + j) & (kPngWindow - 1)] = v;
        dst[pos + j] = v;
    }
}

// ---- one block ------------------------------------------------------------------------------------------------
// Decodes the block at the reader into dst[pos ..) (pos <= n is kept); 0 or a BASD_PNG_* code, the same in every lane.
BASD_HD int png_block(PngBits& b, unsigned char* dst, int n, PngInflateShared& sh, int& pos, int& final, int lane,
                      int lanes) {
    png_fill(b);
    final = (int)png_take(b, 1);
    const int type = (int)png_take(b, 2);
    if (b.over) return BASD_PNG_TRUNCATED;
    if (type == 3) return BASD_PNG_BAD_BLOCK;
    if (type == 0) {
        png_drop(b, b.nbits & 7);
        png_fill(b);
        const unsigned len = png_take(b, 16), nlen = png_take(b, 16);
        if (b.over) return BASD_PNG_TRUNCATED;
        if ((len ^ 0xffffu) != nlen) return BASD_PNG_BAD_STORED;
        const int at = b.pos - (b.nbits >> 3);     // the first byte no bit was taken from
        if ((int)len > n - pos) return BASD_PNG_WRONG_LENGTH;
        if ((int)len > b.len - at) return BASD_PNG_TRUNCATED;
        png_stored(dst, sh.window, pos, b.p + at, (int)len, lane, lanes);
        pos += (int)len;
        b.pos = at + (int)len;
        b.acc = 0;
        b.nbits = 0;
        return 0;
    }
    int nlit = 288, ndist = 32;
    BASD_PNG_SYNC();                                // the tables' lengths are no longer read
    if (type == 1) {
        for (int s = lane; s < 320; s += lanes) sh.lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5;
    } else {
        nlit = (int)png_take(b, 5) + 257;
        ndist = (int)png_take(b, 5) + 1;
        const int ncode = (int)png_take(b, 4) + 4;
        if (b.over) return BASD_PNG_TRUNCATED;
        if (nlit > 286 || ndist > 30) return BASD_PNG_BAD_LENGTHS;
        if (lane == 0)
            for (int i = 0; i < 19; ++i) sh.clens[i] = 0;
        for (int i = 0; i < ncode; ++i) {
            png_fill(b);
            const unsigned v = png_take(b, 3);
            if (lane == 0) sh.clens[png_order(i)] = (unsigned char)v;
        }
        if (b.over) return BASD_PNG_TRUNCATED;
        png_build_huff(sh.clen, sh.clens, 19, true, lane, lanes);
        if (sh.clen.bad) return BASD_PNG_BAD_LENGTHS;
        const int total = nlit + ndist;
        int i = 0, prev = 0;
        while (i < total) {
            png_fill(b);
            const int sym = png_symbol(b, sh.clen);
            if (b.over) return BASD_PNG_TRUNCATED;
            if (sym < 0) return BASD_PNG_BAD_CODE;
            if (sym < 16) {
                if (lane == 0) sh.lens[i] = (unsigned char)sym;
                prev = sym;
                ++i;
                continue;
            }
            int value = 0, repeat;
            if (sym == 16) {
                if (i == 0) return BASD_PNG_BAD_LENGTHS;
                value = prev;
                repeat = 3 + (int)png_take(b, 2);
            } else if (sym == 17) {
                repeat = 3 + (int)png_take(b, 3);
            } else {
                repeat = 11 + (int)png_take(b, 7);
            }
            if (b.over) return BASD_PNG_TRUNCATED;
            if (repeat > total - i) return BASD_PNG_BAD_LENGTHS;
            for (int k = lane; k < repeat; k += lanes) sh.lens[i + k] = (unsigned char)value;
            prev = value;
            i += repeat;
        }
        BASD_PNG_SYNC();
        if (sh.lens[256] == 0) return BASD_PNG_BAD_LENGTHS;
    }
    png_build_huff(sh.lit, sh.lens, nlit, false, lane, lanes);
    png_build_huff(sh.dist, sh.lens + nlit, ndist, false, lane, lanes);
    if (sh.lit.bad || sh.dist.bad) return BASD_PNG_BAD_LENGTHS;
    for (;;) {
        png_fill(b);
        const int sym = png_symbol(b, sh.lit);
        if (b.over) return BASD_PNG_TRUNCATED;
        if (sym < 0) return BASD_PNG_BAD_CODE;
        if (sym < 256) {
            if (pos >= n) return BASD_PNG_WRONG_LENGTH;
            if (lane == 0) {
                sh.window[pos & (kPngWindow - 1)] = (unsigned char)sym;
                dst[pos] = (unsigned char)sym;
            }
            ++pos;
            continue;
        }
        if (sym == 256) return 0;
        if (sym > 285) return BASD_PNG_BAD_CODE;
        const int i = sym - 257;
        int len;
        if (i < 8) {
            len = 3 + i;
        } else if (i == 28) {
            len = 258;
        } else {
            const int e = (i >> 2) - 1;
            len = 3 + ((4 + (i & 3)) << e) + (int)png_take(b, e);
        }
        const int d = png_symbol(b, sh.dist);
        if (b.over) return BASD_PNG_TRUNCATED;
        if (d < 0 || d > 29) return BASD_PNG_BAD_CODE;
        int dist;
        if (d < 4) {
            dist = 1 + d;
        } else {
            const int e = (d >> 1) - 1;
            dist = 1 + ((2 + (d & 1)) << e) + (int)png_take(b, e);
        }
        if (b.over) return BASD_PNG_TRUNCATED;
        if (dist > pos) return BASD_PNG_BAD_DISTANCE;
        if (len > n - pos) return BASD_PNG_WRONG_LENGTH;
        png_match(dst, sh.window, pos, dist, len, lane, lanes);
        pos += len;
    }
}

// The whole stream src[0 .. src_len) (zlib header first) into dst[0 .. n): 0 and the offset of the 4 Adler-32 bytes, or
// a BASD_PNG_* code.
BASD_HD int png_inflate(const unsigned char* src, int src_len, unsigned char* dst, int n, PngInflateShared& sh, int lane,
                        int lanes, int& end_pos) {
    PngBits b;
    png_bits_open(b, src, 2, src_len);
    int pos = 0, final = 0;
    end_pos = 0;
    while (!final) {
        const int code = png_block(b, dst, n, sh, pos, final, lane, lanes);
        if (code) return code;
    }
    if (pos != n) return BASD_PNG_WRONG_LENGTH;
    png_drop(b, b.nbits & 7);
    const int at = b.pos - (b.nbits >> 3);
    if (4 > src_len - at) return BASD_PNG_TRUNCATED;
    end_pos = at;
    return 0;
}

// ---- the Adler-32 and the filter bytes ----------------------------------------------------------------------------
// The lane's share of sum b_i and of sum (n - i) b_i mod 65521 over data[0 .. n), n < 2^31.
BASD_HD void png_adler_partial(const unsigned char* data, long n, int lane, int lanes, uint64_t& a, uint64_t& b) {
    a = 0;
    b = 0;
    unsigned k = 0;
    for (long i = lane; i < n; i += lanes) {
        const uint64_t v = data[i];
        a += v;
        b += (uint64_t)(n - i) * v;                 // < 2^39: 4096 of them stay below 2^52
        if ((++k & 4095u) == 0) b %= 65521u;
    }
    b %= 65521u;
}

BASD_HD uint32_t png_adler_finish(uint64_t a_sum, uint64_t b_sum, long n) {
    return (uint32_t)(((uint64_t)n + b_sum) % 65521u) << 16 | (uint32_t)((1u + a_sum) % 65521u);
}

BASD_HD uint32_t png_be32(const unsigned char* p) {
    return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | (uint32_t)p[3];
}

// Is a filter byte of the lane's rows above 4?
BASD_HD int png_bad_filters(const unsigned char* data, int height, long stride, int lane, int lanes) {
    int bad = 0;
    for (int y = lane; y < height; y += lanes) bad |= data[y * stride] > 4;
    return bad;
}

// ---- unfiltering ------------------------------------------------------------------------------------------------
// A pixel is its bpp bytes in a 32-bit word, the first byte lowest.
BASD_HD uint32_t png_load_px(const unsigned char* p, int bpp) {
    uint32_t v = p[0];
    if (bpp > 1) v |= (uint32_t)p[1] << 8;
    if (bpp > 2) v |= (uint32_t)p[2] << 16;
    if (bpp > 3) v |= (uint32_t)p[3] << 24;
    return v;
}

BASD_HD void png_store_px(unsigned char* p, uint32_t v, int bpp) {
    p[0] = (unsigned char)v;
    if (bpp > 1) p[1] = (unsigned char)(v >> 8);
    if (bpp > 2) p[2] = (unsigned char)(v >> 16);
    if (bpp > 3) p[3] = (unsigned char)(v >> 24);
}

BASD_HD int png_paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (pa <= pb && pa <= pc) ? a : pb <= pc ? b : c;
}

// The pixel `raw` of a scanline of filter type ft (<= 4) with its neighbours a (left), b (above), c (above left).
BASD_HD uint32_t png_recon(int ft, uint32_t raw, uint32_t a, uint32_t b, uint32_t c, int bpp) {
    uint32_t out = 0;
    for (int k = 0; k < 4; ++k) {
        if (k >= bpp) break;
        const int x = (raw >> (8 * k)) & 255, ak = (a >> (8 * k)) & 255, bk = (b >> (8 * k)) & 255, ck = (c >> (8 * k)) & 255;
        const int pred = ft == 0 ? 0 : ft == 1 ? ak : ft == 2 ? bk : ft == 3 ? (ak + bk) >> 1 : png_paeth(ak, bk, ck);
        out |= (uint32_t)((x + pred) & 255) << (8 * k);
    }
    return out;
}

BASD_HD void png_store_rgb(unsigned char* o, uint32_t px, int color_type, const unsigned char* plte) {
    unsigned char r, g, b;
    if (color_type == 3) {
        const unsigned char* e = plte + 3 * (px & 255u);
        r = e[0]; g = e[1]; b = e[2];
    } else if (color_type == 0 || color_type == 4) {
        r = g = b = (unsigned char)px;
    } else {
        r = (unsigned char)px; g = (unsigned char)(px >> 8); b = (unsigned char)(px >> 16);
    }
    o[0] = r; o[1] = g; o[2] = b;
}

struct PngRow {                                     // a scanline on its way from left to right
    int ft;
    uint32_t a, c, last;                            // left, above left, and the pixel reconstructed last
};

// Pixel x of the scanline whose bytes (behind the filter byte) are `line`: `up` is the pixel above (0 in row 0).  The
// pixel is written as RGB at rgb + 3 x; `keep` writes it back into the line as well, for a later row to read as `up`.
BASD_HD void png_unfilter_step(unsigned char* line, int x, int bpp, int color_type, uint32_t up, PngRow& s,
                               const unsigned char* plte, unsigned char* rgb, bool keep) {
    const uint32_t px = png_recon(s.ft, png_load_px(line + (long)x * bpp, bpp), s.a, up, s.c, bpp);
    s.c = up;
    s.a = px;
    s.last = px;
    if (keep) png_store_px(line + (long)x * bpp, px, bpp);
    png_store_rgb(rgb + 3L * x, px, color_type, plte);
}

}  // namespace basd
