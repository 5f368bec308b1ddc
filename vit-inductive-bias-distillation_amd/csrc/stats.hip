// Per-channel sum and sum of squares of uint8 pixels in ONE launch, accumulated exactly into nine 64-bit words (the
// contract is in include/basd_hip.h).
//
// A streaming pass over bytes: every byte is read once, nothing is written but at most nine atomic adds per workgroup.
// Both layouts are byte streams with a periodic channel pattern.  HWC is ONE segment of images * pixels * C bytes whose
// byte i belongs to channel i mod C (period CS = C); CHW is images * C segments of `pixels` bytes, each of one channel
// (period CS = 1, the sums of segment s go to channel s mod C).  A segment is cut at its first 16-byte boundary into a
// head of h < 16 bytes, nvec 16-byte vectors and a tail of < 16 bytes.  The vectors are walked in tiles of 192 (3 KiB:
// three loads of one vector per lane, each load 1 KiB contiguous over the wave), one wave per tile, by a capped grid
// with a grid stride; the wave that has a segment's tile 0 also takes its head and tail, one byte per lane.
//
// v_dot4_u32_u8 gives both sums of a dword: the sum of a channel's bytes is a dot with a 0/1 byte mask, the sum of
// their squares a dot of the masked dword with itself.  Which bytes of a dword belong to which channel depends on the
// dword's offset in the stream mod CS only; 3072, 1024 and 16 are multiples of 1, 2 and 4 and are 0, 1 and 1 mod 3, so
// with vector v = 192 tile + 64 j + lane starting at stream offset h + 16 v
//     channel of byte b of dword k of load j  =  (j 1024 + 4 k + b  +  h + 16 lane)  mod CS
// The first part is a compile-time constant (the masks), the second is fixed per lane for the whole launch: every lane
// sums in channels RELATIVE to its own phase (h + 16 lane) mod CS and rotates its sums once before the reduction.
#include "basd_common.h"
#include "../../include/basd_hip.h"

namespace basd {

// Every workgroup ends with ONE wave instruction of atomic adds to the same 72 bytes of `state`, and adds to one
// line are applied one after the other at the memory side.  So the workgroups are few and large: 16 waves, two per CU
// (all 32 wave slots of a CU, 96 KiB of loads in flight per CU).  profiles/channel_stats.txt has the times per grid
// (the max_blocks lines): a cap of 256 was 2-4 us faster there than this one and has not been adopted yet.
constexpr int kStatsWaves = 16;
constexpr int kStatsBlock = kStatsWaves * kWave;
constexpr int kStatsMaxGrid = 512;             // 256 CUs x 2 workgroups; the tiles are walked with a grid stride
constexpr int kStatsLoads = 3;                 // vectors per lane and tile
constexpr int kStatsTileVecs = kStatsLoads * kWave;
constexpr int kStatsMaxChannels = 4;

typedef unsigned int v4u __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

// bytes of dword k of load j that belong to the lane-relative channel c: 0x01 in each such byte
template <int CS>
__host__ __device__ constexpr unsigned stats_mask(int j, int k, int c) {
    unsigned m = 0;
    for (int b = 0; b < 4; ++b)
        if ((j * 1024 + 4 * k + b) % CS == c) m |= 1u << (8 * b);
    return m;
}

struct StatsArgs {
    const unsigned char* src;
    long seg_bytes;          // bytes of one segment
    unsigned tiles_per_seg;  // >= 1: tile 0 of a segment exists even without a vector (it takes the head and the tail)
    unsigned items;          // segments * tiles_per_seg
    int C;
    long long count;         // images * pixels, added to state[0] by workgroup 0
    u64* state;
};

template <int CS>
__global__ void __launch_bounds__(kStatsBlock) channel_stats_kernel(StatsArgs a) {
    // CS > 1: one segment, sums per lane-relative channel; CS == 1: sums per channel, segment s is channel s mod C
    constexpr int NS = CS > 1 ? CS : kStatsMaxChannels;
    __shared__ u64 part[2 * kStatsMaxChannels];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    u64 s1[NS], s2[NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) s1[c] = s2[c] = 0;
    unsigned phase = 0;                                        // (h + 16 lane) mod CS
    const unsigned stride = gridDim.x * kStatsWaves;
    for (unsigned it = blockIdx.x * kStatsWaves + wid; it < a.items; it += stride) {
        const unsigned seg = CS > 1 ? 0u : it / a.tiles_per_seg;
        const unsigned tile = CS > 1 ? it : it - seg * a.tiles_per_seg;
        const unsigned char* base = a.src + (long)seg * a.seg_bytes;
        const long to_boundary = (long)((0 - (uintptr_t)base) & 15);
        const long h = to_boundary < a.seg_bytes ? to_boundary : a.seg_bytes;
        const long nvec = (a.seg_bytes - h) >> 4;
        phase = (unsigned)(h + 16 * lane) % CS;
        v4u w[kStatsLoads];
#pragma unroll
        for (int j = 0; j < kStatsLoads; ++j) {
            const long v = (long)tile * kStatsTileVecs + j * kWave + lane;
            w[j] = v4u{0u, 0u, 0u, 0u};                        // a zero vector adds nothing to either sum
            if (v < nvec) w[j] = *(const v4u*)(base + h + 16 * v);
        }
        // The partial sums of ONE tile are 32 bits wide: at most 12 dwords and one head / tail byte reach one of them,
        // 12 * 4 * 255^2 + 255^2 = 3 186 225 < 2^32.  Everything that outlives a tile is 64 bits wide.
        unsigned p1[CS], p2[CS];
#pragma unroll
        for (int c = 0; c < CS; ++c) p1[c] = p2[c] = 0;
        if (tile == 0) {
            // head bytes [0, h) and tail bytes [h + 16 nvec, seg_bytes): fewer than 16 each, one per lane
            const long tail0 = h + 16 * nvec;
            const long i = lane < h ? (long)lane : tail0 + (lane - h);
            if (i < a.seg_bytes) {
                const unsigned x = base[i];
                const unsigned rel = ((unsigned)(i % CS) + CS - phase) % CS;
#pragma unroll
                for (int c = 0; c < CS; ++c)
                    if (rel == (unsigned)c) {
                        p1[c] = x;
                        p2[c] = x * x;
                    }
            }
        }
#pragma unroll
        for (int j = 0; j < kStatsLoads; ++j) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
#pragma unroll
                for (int c = 0; c < CS; ++c) {
                    const unsigned m = stats_mask<CS>(j, k, c);             // a constant once unrolled
                    if (m != 0u) {
                        const unsigned x = w[j][k] & (m * 255u);
                        p1[c] = __builtin_amdgcn_udot4(w[j][k], m, p1[c], false);
                        p2[c] = __builtin_amdgcn_udot4(x, x, p2[c], false);
                    }
                }
            }
        }
        if constexpr (CS > 1) {
#pragma unroll
            for (int c = 0; c < CS; ++c) {
                s1[c] += p1[c];
                s2[c] += p2[c];
            }
        } else {
            const unsigned ch = seg % (unsigned)a.C;           // wave-uniform
#pragma unroll
            for (int c = 0; c < NS; ++c)
                if (ch == (unsigned)c) {
                    s1[c] += p1[0];
                    s2[c] += p2[0];
                }
        }
    }
    // the lane's relative channel r is channel (r + phase) mod CS: the one segment of CS > 1 has one h, so `phase` is
    // the same in every iteration (a wave without an item has sums of zero)
    u64 t1[NS], t2[NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        t1[c] = s1[c];
        t2[c] = s2[c];
        if constexpr (CS > 1) {
#pragma unroll
            for (int r = 0; r < CS; ++r)
                if ((r + phase) % CS == (unsigned)c) {
                    t1[c] = s1[r];
                    t2[c] = s2[r];
                }
        }
    }
    // within the wave by shuffles, then one lane per wave adds the wave's sums into LDS (64-bit LDS atomics, 16 adders
    // per word): integer sums do not depend on their order
    if (threadIdx.x < 2 * kStatsMaxChannels) part[threadIdx.x] = 0;
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        t1[c] = group_sum(t1[c], kWave);
        t2[c] = group_sum(t2[c], kWave);
    }
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < NS; ++c) {
            __hip_atomic_fetch_add(&part[c], t1[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_add(&part[kStatsMaxChannels + c], t2[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
    __syncthreads();
    // word 0: the pixel count (workgroup 0); words 1..4: sums; words 5..8: sums of squares; channels >= C are not touched
    const int word = threadIdx.x;
    if (word < 1 + 2 * kStatsMaxChannels) {
        u64 v = 0;
        bool mine = false;
        if (word == 0) {
            mine = blockIdx.x == 0;
            v = (u64)a.count;
        } else {
            const int c = (word - 1) % kStatsMaxChannels;
            mine = c < a.C;
            v = part[word - 1];
        }
        if (mine && v != 0) __hip_atomic_fetch_add(a.state + word, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace basd

extern "C" {

int basd_channel_stats(const unsigned char* src, int layout, long images, int C, long pixels, long long* state,
                       int max_blocks, hipStream_t stream) {
    BASD_CHECK_ARG(layout == BASD_LAYOUT_HWC || layout == BASD_LAYOUT_CHW);
    BASD_CHECK_ARG(C >= 1 && C <= basd::kStatsMaxChannels && images >= 0 && pixels >= 0 && max_blocks >= 0);
    if (images == 0 || pixels == 0) return BASD_OK;
    BASD_CHECK_ARG(src && state);
    BASD_CHECK_ARG(pixels <= (1L << 40) / images);            // images * pixels * C stays far inside 63 bits
    basd::StatsArgs a = {};
    a.src = src;
    a.C = C;
    a.count = (long long)(images * pixels);
    a.state = (basd::u64*)state;
    const bool hwc = layout == BASD_LAYOUT_HWC;
    const long segments = hwc ? 1 : images * C;
    a.seg_bytes = hwc ? images * pixels * C : pixels;
    const long tiles = ((a.seg_bytes >> 4) + basd::kStatsTileVecs - 1) / basd::kStatsTileVecs;
    const long tiles_per_seg = tiles > 0 ? tiles : 1;
    BASD_CHECK_ARG(tiles_per_seg < (1L << 31) / segments);    // 32-bit item indices (HWC: below 6 TiB)
    a.tiles_per_seg = (unsigned)tiles_per_seg;
    a.items = (unsigned)(segments * tiles_per_seg);
    long grid = ((long)a.items + basd::kStatsWaves - 1) / basd::kStatsWaves;
    if (grid > basd::kStatsMaxGrid) grid = basd::kStatsMaxGrid;
    if (max_blocks > 0 && grid > max_blocks) grid = max_blocks;
    const int cs = hwc ? C : 1;
    if (cs == 1) {
        basd::channel_stats_kernel<1><<<(int)grid, basd::kStatsBlock, 0, stream>>>(a);
    } else if (cs == 2) {
        basd::channel_stats_kernel<2><<<(int)grid, basd::kStatsBlock, 0, stream>>>(a);
    } else if (cs == 3) {
        basd::channel_stats_kernel<3><<<(int)grid, basd::kStatsBlock, 0, stream>>>(a);
    } else {
        basd::channel_stats_kernel<4><<<(int)grid, basd::kStatsBlock, 0, stream>>>(a);
    }
    BASD_RETURN_LAST();
}

}  // extern "C"
