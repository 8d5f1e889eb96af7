// The 128 x 128 pair-tile sweep: one q x n (or upper-triangle n x n) reduction over rows of 16-byte slots, as k_distance
// (distance.hip), k_distance_rect_tile (nearest.hip) and k_compared (compared.hip) run it.  Its one description, and what the three
// share: the geometry, the row padding, the split-K plan, the arguments, the LDS-DMA request, the triangle enumeration, the tile /
// part decode and the distance predicate.  The slab loop itself stands in each kernel: as one inlined function template it compiles,
// for the distance predicate, to a loop that spills about 50 registers at three waves per SIMD (profiles/r31/pair_tiles.md).
//
// Operands (HBM): a matrix of rows of uint4 slots, every row padded with zero slots to a multiple of PAIR_SLOTS.  Two readings:
//   packed matrix  packed[row][word] = uint4 { valid, code_hi, code_lo, lower } for 32 consecutive sites, bit i = site 32*word + i;
//                  A=0 C=1 G=2 T=3.  A slot is one word.  Per pair and word (DistanceWord):
//                      mismatches += popcount( ((xh ^ yh) | (xl ^ yl)) & xv & yv )
//                  which gfx950 does in 4 VALU ops per 32 site-compares (v_xor, 2 x v_bitop3, v_bcnt).
//   valid plane    one uint32 per 32 sites (compared.hip).  A slot is four words, so a ds_read_b128 feeds 4 words x 8 partners x
//                  2 VALU ops (v_and, v_bcnt with accumulate) = 64 lane-ops where the packed reading feeds 32: half the LDS reads
//                  per VALU op, half the VALU ops per 32 sites.
// This is integer VALU + LDS work (no MFMA): a 128 x 128 block of pairs per workgroup, 8 x 8 pairs per lane; slabs of PAIR_SLOTS
// slots of both operands stream into a double-buffered LDS area (32 KiB) with LDS-DMA (global_load_lds_dwordx4: no staging
// registers, no LDS store instructions) one slab ahead of the arithmetic, one s_waitcnt vmcnt(0) and one barrier per slab.  Slot s
// of row r holds slot s ^ ((r >> 2) & 3) of the slab, which makes the 16 rows a wave reads at once fall into 16 different bank
// groups.  Rows past either matrix read that matrix's last row and are never stored.
// Two choices, flags of the kernels:
//   kSquare  one matrix against itself: the tiles of the upper triangle, each stored with its mirror image; else a plain grid of
//            tiles, row-major.  Tile tile_rank + g * tile_nranks is the g-th of a rank (ranks share one output).
//   kSplit   a few tiles only: every tile is shared by k_parts workgroups, each sums its range of k_chunk slots and adds it to
//            the (zeroed) output with integer atomics — sums of integers: the result does not depend on the order.
#pragma once

#include "internal.h"

#define PAIR_TILE 128
#define PAIR_SLOTS 4                // 16-byte slots per row and slab
#define PAIR_THREADS 256

// words (of 32 sites) of a row of the packed matrix: the padding words come out all zero (no valid site)
static inline uint32_t padded_words(uint32_t n_sites) { return ((n_sites + 31) / 32 + PAIR_SLOTS - 1) / PAIR_SLOTS * PAIR_SLOTS; }

// Split-K on the host: with fewer tiles than CUs and at least 4 slabs of kw slots, the slots are cut in about wanted_parts ranges
// of whole slabs, none below 2 slabs.  Returns whether the output has to be zeroed for a kSplit launch of tiles * k_parts workgroups.
static inline bool pair_split_plan(uint32_t slots, uint32_t kw, uint64_t tiles, uint32_t n_cu, uint64_t wanted_parts, uint32_t *k_chunk, uint32_t *k_parts) {
    *k_chunk = slots;
    *k_parts = 1;
    if (tiles >= n_cu || slots < 4 * kw) return false;
    const uint64_t max_parts = slots / (2 * kw);
    const uint64_t parts = wanted_parts < max_parts ? wanted_parts : max_parts;
    *k_chunk = (uint32_t)(((slots + parts - 1) / parts + kw - 1) / kw * kw);
    *k_parts = (slots + *k_chunk - 1) / *k_chunk;
    return true;
}

struct PairArgs {
    const uint4 *pq, *pdb;          // the operands (kSquare: the same)
    uint32_t q, n, slots;           // rows of either, slots per row
    uint32_t tiles_n;               // tiles along the database (kSquare: along either side)
    uint64_t total_tiles;
    uint32_t tile_rank, tile_nranks;    // k_distance alone: the others take every tile
    uint32_t k_parts, k_chunk;      // split-K: the slots are cut in k_parts ranges of k_chunk slots (k_compared has no split and reads neither)
    int32_t *out;
    uint64_t stride;                // elements
};

// one 16-byte LDS-DMA request per lane: the wave's 64 lanes fill the 1 KiB from lds_byte (wave-uniform) on
__device__ __forceinline__ void lds_dma16(const uint4 *gp, uint32_t lds_byte) {
    const uint32_t m0v = __builtin_amdgcn_readfirstlane(lds_byte);
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(gp), "s"(m0v) : "memory");
}

__device__ __forceinline__ void triangle_coords(uint64_t t, uint32_t nt, uint32_t &bi, uint32_t &bj) {
    // row-major enumeration of the upper triangle: row b starts at b*nt - b*(b-1)/2
    double fn = (double)nt + 0.5;
    int64_t b = (int64_t)(fn - sqrt(fn * fn - 2.0 * (double)t));
    if (b < 0) b = 0;
    if (b >= nt) b = nt - 1;
    auto start = [&](int64_t r) { return (uint64_t)r * nt - (uint64_t)r * (uint64_t)(r - 1) / 2; };
    while (b > 0 && start(b) > t) --b;
    while (b + 1 < (int64_t)nt && start(b + 1) <= t) ++b;
    bi = (uint32_t)b;
    bj = (uint32_t)(b + (t - start(b)));
}

// workgroup gg of a launch -> its tile and its range of slots (multiples of the slab)
template <bool kSplit>
__device__ __forceinline__ uint64_t pair_part(uint64_t gg, const PairArgs &a, uint32_t &k_begin, uint32_t &k_end) {
    k_begin = kSplit ? (uint32_t)(gg % a.k_parts) * a.k_chunk : 0;
    k_end = kSplit && k_begin + a.k_chunk < a.slots ? k_begin + a.k_chunk : a.slots;
    return kSplit ? gg / a.k_parts : gg;
}

// the distance predicate (utils.py:1135-1165) on one word of two packed rows
struct DistanceWord {
    __device__ __forceinline__ int32_t operator()(const uint4 &x, const uint4 &y, int32_t acc) const {
        // ((xh ^ yh) | (xl ^ yl)) & xv & yv as v_xor + two 3-input bit ops (truth tables 0xBE, 0x80)
        const uint32_t u = __builtin_amdgcn_bitop3_b32(x.y, y.y, x.z ^ y.z, 0xBE);
        return acc + __popc(__builtin_amdgcn_bitop3_b32(u, x.x, y.x, 0x80));
    }
};
