// Compared(i, j): at how many columns a pair of samples was compared at all — the number behind the trust in a small distance.
//
// Additive: utils.calculate_sequence_distance (snppipeline/utils.py:1135-1165) counts a column for a pair iff, after upper-casing,
// both bytes are in {A,C,G,T} and they differ; a column where either sample holds '-' or 'N' is silently a match, and nothing in
// distance.py:93-106 says how many columns that were.  Compared(i, j) is that predicate without "and differ": the popcount of
// valid_i & valid_j over the `valid` plane of the packed matrix of distance.hip.  Distance <= Compared <= min of the two diagonals.
//
//   a. k_valid_plane: the `valid` words of a packed matrix (uint4 {valid, hi, lo, lower} per 32 sites) as a dense plane, one
//      uint32 per 32 sites, a row padded with zero words to a multiple of CMP_KW words — one slab of the tile kernel.  Every word
//      of the destination is written: the padding is zero whatever lay there, and no bit at or beyond n_sites is taken whatever
//      the packed matrix holds.  A lane per output word, coalesced on both sides.
//   b. k_compared: the q x n block of two planes (the same plane twice: the symmetric matrix, upper-triangle tiles and their
//      mirror images, as k_distance): the slab scheme pair_tiles.h describes, a slot of which holds four words of the plane here.
//      No split over the word range for shapes of few tiles (k_distance's kSplit): 125 samples x 50 000 sites are microseconds
//      of work on one CU.
//   c. k_compared_pairs: Compared of listed pairs (a[p], b[p]) — a indexes the rows of one plane, b of a second, possibly the
//      same — without the matrix: a wave per pair (grid-stride over the pairs), 16 bytes of each row per lane and step, a wave
//      sum, out[p].  No atomic: every output position is its pair's index.  A pass over the lists refuses a pair that names a
//      row outside its matrix before anything is written.
#include "pair_tiles.h"
#include "prims.h"

#define CMP_TILE 128
#define CMP_KW 16                // words (of 32 sites) per slab of the tile kernel: 4 to a 16-byte slot
static_assert(CMP_TILE == PAIR_TILE && CMP_KW == 4 * PAIR_SLOTS, "the geometry of pair_tiles.h under the names the plane is padded by");
#define CMP_THREADS 256          // the plane and pair kernels
#define CMP_PAIR_WAVES (CMP_THREADS / 64)
#define CMP_PAIR_GRID_CAP 1024   // workgroups: more pairs than 4 x this go round the grid-stride loop

static inline uint32_t plane_words(uint32_t n_sites) { return ((n_sites + 31) / 32 + CMP_KW - 1) / CMP_KW * CMP_KW; }
extern "C" size_t snpgpu_valid_plane_row_bytes(uint32_t n_sites) { return (size_t)plane_words(n_sites) * 4; }

namespace {

__global__ __launch_bounds__(CMP_THREADS) void k_valid_plane(const uint4 *packed, uint32_t n_rows, uint32_t n_sites, uint32_t packed_words, uint32_t *plane,
                                                             uint32_t words) {
    const uint64_t total = (uint64_t)n_rows * words;
    for (uint64_t g = (uint64_t)blockIdx.x * CMP_THREADS + threadIdx.x; g < total; g += (uint64_t)gridDim.x * CMP_THREADS) {
        const uint32_t row = (uint32_t)(g / words), w = (uint32_t)(g % words);
        uint32_t v = 0;
        if (w < packed_words && 32u * w < n_sites) {
            v = packed[(size_t)row * packed_words + w].x;
            const uint32_t left = n_sites - 32u * w;
            if (left < 32u) v &= (1u << left) - 1u;
        }
        plane[g] = v;
    }
}

// acc + popcount(m) in the one instruction that does both.  Written out: left to itself the compiler regroups the four sums of a
// slot into popcounts onto zero and two three-operand adds — 5 VALU ops per 2 words instead of 4 (seen in the ISA, and as 21.9 ms
// against 17.6 ms for the 10 000 x 200 000 matrix, profiles/r22/compared.md).
__device__ __forceinline__ int32_t count_onto(uint32_t m, int32_t acc) {
    int32_t sum;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(sum) : "v"(m), "v"(acc));
    return sum;
}

__device__ __forceinline__ int32_t both_valid(const uint4 &x, const uint4 &y, int32_t acc) {
    acc = count_onto(x.x & y.x, acc);
    acc = count_onto(x.y & y.y, acc);
    acc = count_onto(x.z & y.z, acc);
    return count_onto(x.w & y.w, acc);
}

// kSquare: pq == pdb, q == n; the tiles of the upper triangle, each stored with its mirror image.
template <bool kSquare>
__global__ __launch_bounds__(PAIR_THREADS, 3) void k_compared(PairArgs a) {
    // [buffer][operand][row][slot]; a wave's 64 DMA lanes fill 64 consecutive 16-byte slots
    __shared__ uint4 slab[2][2][PAIR_TILE][PAIR_SLOTS];
    constexpr int kPieces = PAIR_TILE * PAIR_SLOTS / PAIR_THREADS;
    const uint32_t tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (uint64_t t = blockIdx.x; t < a.total_tiles; t += gridDim.x) {
        uint32_t bi, bj;
        if (kSquare) triangle_coords(t, a.tiles_n, bi, bj);
        else { bi = (uint32_t)(t / a.tiles_n); bj = (uint32_t)(t % a.tiles_n); }
        const uint32_t r0 = bi * PAIR_TILE, c0 = bj * PAIR_TILE;
        int32_t acc[8][8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[i][j] = 0;

        // DMA: chunk p = e * 256 + tid of an operand's slab is slot (p & 3) of row (p >> 2); slot s of row r holds the words
        // 4 (s ^ ((r >> 2) & 3)) ... + 3 of the slab
        uint32_t row_of[2][kPieces], kk_of[kPieces];
#pragma unroll
        for (int e = 0; e < kPieces; ++e) {
            const uint32_t p = e * PAIR_THREADS + tid, rr = p >> 2;
            kk_of[e] = (p & 3u) ^ ((rr >> 2) & 3u);
            row_of[0][e] = r0 + rr < a.q ? r0 + rr : a.q - 1;
            row_of[1][e] = c0 + rr < a.n ? c0 + rr : a.n - 1;
        }
        auto request = [&](uint32_t k0, int buf) {
#pragma unroll
            for (int op = 0; op < 2; ++op)
#pragma unroll
                for (int e = 0; e < kPieces; ++e) {
                    const uint4 *gp = (op ? a.pdb : a.pq) + ((size_t)row_of[op][e] * a.slots + (k0 + kk_of[e]));
                    lds_dma16(gp, (uint32_t)(uintptr_t)((__attribute__((address_space(3))) char *)&slab[buf][op][0][0]) + (e * PAIR_THREADS + wave * 64) * 16);
                }
        };
        __syncthreads();                                            // the previous tile's last slab has been read
        request(0, 0);
        int buf = 0;
        for (uint32_t k0 = 0; k0 < a.slots; k0 += PAIR_SLOTS, buf ^= 1) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // my part of this slab has landed ...
            __syncthreads();                                        // ... everybody's has, and the slab before has been read
            if (k0 + PAIR_SLOTS < a.slots) request(k0 + PAIR_SLOTS, buf ^ 1);
#pragma unroll
            for (int kk = 0; kk < PAIR_SLOTS; ++kk) {
                uint4 x[8], y[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) { const uint32_t r = ty + 16 * i; x[i] = slab[buf][0][r][kk ^ ((r >> 2) & 3u)]; }
#pragma unroll
                for (int j = 0; j < 8; ++j) { const uint32_t c = tx + 16 * j; y[j] = slab[buf][1][c][kk ^ ((c >> 2) & 3u)]; }
#pragma unroll
                for (int i = 0; i < 8; ++i)
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[i][j] = both_valid(x[i], y[j], acc[i][j]);
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint32_t r = r0 + ty + 16 * i;
            if (r >= a.q) continue;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint32_t c = c0 + tx + 16 * j;
                if (c >= a.n) continue;
                a.out[(size_t)r * a.stride + c] = acc[i][j];
                if (kSquare && bi != bj) a.out[(size_t)c * a.stride + r] = acc[i][j];
            }
        }
    }
}

// *status raised by a pair that names a row outside its matrix
__global__ __launch_bounds__(CMP_THREADS) void k_compared_check(const uint32_t *ia, const uint32_t *ib, uint64_t n_pairs, uint32_t n_a, uint32_t n_b, uint32_t *status) {
    for (uint64_t p = (uint64_t)blockIdx.x * CMP_THREADS + threadIdx.x; p < n_pairs; p += (uint64_t)gridDim.x * CMP_THREADS)
        if (ia[p] >= n_a || ib[p] >= n_b) *status = 1u;
}

__global__ __launch_bounds__(CMP_THREADS) void k_compared_pairs(const uint4 *pa, const uint4 *pb, uint32_t slots, const uint32_t *ia, const uint32_t *ib,
                                                                uint64_t n_pairs, int32_t *out) {
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t p = (uint64_t)blockIdx.x * CMP_PAIR_WAVES + (threadIdx.x >> 6); p < n_pairs; p += (uint64_t)gridDim.x * CMP_PAIR_WAVES) {
        const uint4 *ra = pa + (size_t)ia[p] * slots, *rb = pb + (size_t)ib[p] * slots;
        int32_t cnt = 0;
        for (uint32_t s = lane; s < slots; s += 64) cnt = both_valid(ra[s], rb[s], cnt);
        const uint32_t total = wave_inclusive_sum((uint32_t)cnt);
        if (lane == 63) out[p] = (int32_t)total;
    }
}

}  // namespace

extern "C" {

int snpgpu_valid_plane_dev(snpgpu_ctx *ctx, const void *d_packed, uint32_t n_rows, uint32_t n_sites, void *d_plane) {
    if (!ctx) return SNPGPU_E_ARG;
    if (n_rows == 0 || n_sites == 0) return SNPGPU_OK;
    if (!d_packed || !d_plane || (((uintptr_t)d_packed | (uintptr_t)d_plane) & 15))
        return snpgpu_set_error(ctx, SNPGPU_E_ARG, "the packed matrix or the plane is null or not 16-byte aligned");
    HIP_TRY(ctx, snpgpu_enter(ctx));
    const uint32_t words = plane_words(n_sites);
    const uint64_t blocks = ((uint64_t)n_rows * words + CMP_THREADS - 1) / CMP_THREADS, cap = (uint64_t)ctx->n_cu * 32;
    k_valid_plane<<<(unsigned)(blocks < cap ? blocks : cap), CMP_THREADS, 0, ctx->stream>>>((const uint4 *)d_packed, n_rows, n_sites,
                                                                                           padded_words(n_sites), (uint32_t *)d_plane, words);
    HIP_TRY(ctx, hipGetLastError());
    return SNPGPU_OK;
}

int snpgpu_compared_rect_dev(snpgpu_ctx *ctx, const void *d_plane_q, uint32_t q, const void *d_plane_db, uint32_t n, uint32_t n_sites, int32_t *d_out,
                             uint64_t out_stride) {
    if (!ctx) return SNPGPU_E_ARG;
    if (q == 0 || n == 0) return SNPGPU_OK;
    if (!d_out || ((uintptr_t)d_out & 3) || out_stride < n) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "the output is null, not 4-byte aligned or its pitch is below n");
    if (n_sites && (!d_plane_q || !d_plane_db || (((uintptr_t)d_plane_q | (uintptr_t)d_plane_db) & 15)))
        return snpgpu_set_error(ctx, SNPGPU_E_ARG, "a plane is null or not 16-byte aligned");
    HIP_TRY(ctx, snpgpu_enter(ctx));
    hipStream_t st = ctx->stream;
    if (n_sites == 0) {                                         // no sites at all: nothing was compared
        HIP_TRY(ctx, hipMemset2DAsync(d_out, out_stride * 4, 0, (size_t)n * 4, q, st));
        return SNPGPU_OK;
    }
    PairArgs a;
    a.pq = (const uint4 *)d_plane_q;
    a.pdb = (const uint4 *)d_plane_db;
    a.q = q;
    a.n = n;
    a.slots = plane_words(n_sites) / 4;
    a.tile_rank = 0;
    a.tile_nranks = 1;
    a.k_parts = 1;
    a.k_chunk = a.slots;
    a.out = d_out;
    a.stride = out_stride;
    a.tiles_n = (n + PAIR_TILE - 1) / PAIR_TILE;
    const bool square = d_plane_q == d_plane_db && q == n;
    a.total_tiles = square ? (uint64_t)a.tiles_n * (a.tiles_n + 1) / 2 : (uint64_t)((q + PAIR_TILE - 1) / PAIR_TILE) * a.tiles_n;
    const uint64_t cap = (uint64_t)ctx->n_cu * 64;
    const unsigned grid = (unsigned)(a.total_tiles < cap ? a.total_tiles : cap);
    if (square) k_compared<true><<<grid, PAIR_THREADS, 0, st>>>(a);
    else k_compared<false><<<grid, PAIR_THREADS, 0, st>>>(a);
    HIP_TRY(ctx, hipGetLastError());
    return SNPGPU_OK;
}

int snpgpu_compared_pairs_dev(snpgpu_ctx *ctx, const void *d_plane_a, uint32_t n_a, const void *d_plane_b, uint32_t n_b, uint32_t n_sites, const uint32_t *d_a,
                              const uint32_t *d_b, uint64_t n_pairs, int32_t *d_out) {
    if (!ctx) return SNPGPU_E_ARG;
    if (n_pairs == 0) return SNPGPU_OK;
    if (!d_a || !d_b || !d_out || (((uintptr_t)d_a | (uintptr_t)d_b | (uintptr_t)d_out) & 3))
        return snpgpu_set_error(ctx, SNPGPU_E_ARG, "the pair lists or the output are null or not 4-byte aligned");
    if (n_sites && n_a && n_b && (!d_plane_a || !d_plane_b || (((uintptr_t)d_plane_a | (uintptr_t)d_plane_b) & 15)))
        return snpgpu_set_error(ctx, SNPGPU_E_ARG, "a plane is null or not 16-byte aligned");
    HIP_TRY(ctx, snpgpu_enter(ctx));
    hipStream_t st = ctx->stream;
    void *ws = nullptr;
    const int rc = snpgpu_scratch(ctx, 8, &ws);
    if (rc != SNPGPU_OK) return rc;
    uint32_t *d_status = (uint32_t *)ws, status = 0;
    const uint64_t check_blocks = (n_pairs + CMP_THREADS - 1) / CMP_THREADS;
    HIP_TRY(ctx, hipMemsetAsync(d_status, 0, 4, st));
    k_compared_check<<<(unsigned)(check_blocks < CMP_PAIR_GRID_CAP ? check_blocks : CMP_PAIR_GRID_CAP), CMP_THREADS, 0, st>>>(d_a, d_b, n_pairs, n_a, n_b, d_status);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(&status, d_status, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (status) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "a pair names a row outside the %u and %u rows of its matrices", n_a, n_b);
    if (n_sites == 0) {
        HIP_TRY(ctx, hipMemsetAsync(d_out, 0, (size_t)n_pairs * 4, st));
        return SNPGPU_OK;
    }
    const uint64_t blocks = (n_pairs + CMP_PAIR_WAVES - 1) / CMP_PAIR_WAVES;
    k_compared_pairs<<<(unsigned)(blocks < CMP_PAIR_GRID_CAP ? blocks : CMP_PAIR_GRID_CAP), CMP_THREADS, 0, st>>>((const uint4 *)d_plane_a, (const uint4 *)d_plane_b,
                                                                                                               plane_words(n_sites) / 4, d_a, d_b, n_pairs, d_out);
    HIP_TRY(ctx, hipGetLastError());
    return SNPGPU_OK;
}

int snpgpu_compared(snpgpu_ctx *ctx, const uint8_t *symbols, uint32_t n, uint32_t n_sites, int32_t *out_matrix) {
    if (!ctx) return SNPGPU_E_ARG;
    if (n == 0) return SNPGPU_OK;
    if (!out_matrix || (n_sites && !symbols)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null compared argument");
    HIP_TRY(ctx, snpgpu_enter(ctx));
    const size_t out_bytes = (size_t)n * n * 4;
    DevSymbols dev;
    int rc = dev.open(ctx, symbols, n, n_sites, DevSymbols::PLANE, nullptr, out_bytes);
    if (rc == SNPGPU_OK) rc = snpgpu_compared_rect_dev(ctx, dev.plane(), n, dev.plane(), n, n_sites, (int32_t *)dev.extra(), n);
    if (rc != SNPGPU_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(out_matrix, dev.extra(), out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return SNPGPU_OK;
}

int snpgpu_compared_pairs(snpgpu_ctx *ctx, const uint8_t *symbols_a, uint32_t n_a, const uint8_t *symbols_b, uint32_t n_b, uint32_t n_sites, const uint32_t *a,
                          const uint32_t *b, uint64_t n_pairs, int32_t *out) {
    if (!ctx) return SNPGPU_E_ARG;
    if (!symbols_b) n_b = n_a;                                  // both indices address symbols_a
    if (n_pairs && (!a || !b || !out)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null compared-pairs argument");
    if (n_sites && ((n_a && !symbols_a))) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null compared-pairs argument");
    for (uint64_t p = 0; p < n_pairs; ++p)
        if (a[p] >= n_a || b[p] >= n_b)
            return snpgpu_set_error(ctx, SNPGPU_E_ARG, "pair %llu names row %u of %u", (unsigned long long)p, a[p] >= n_a ? a[p] : b[p], a[p] >= n_a ? n_a : n_b);
    if (n_pairs == 0) return SNPGPU_OK;
    HIP_TRY(ctx, snpgpu_enter(ctx));
    if (n_sites == 0) {
        for (uint64_t p = 0; p < n_pairs; ++p) out[p] = 0;
        return SNPGPU_OK;
    }
    hipStream_t st = ctx->stream;
    DevSymbols dev_a, dev_b;                                    // the lists and the counts behind the first plane
    int rc = dev_a.open(ctx, symbols_a, n_a, n_sites, DevSymbols::PLANE, nullptr, (size_t)n_pairs * 12);
    if (rc == SNPGPU_OK && symbols_b) rc = dev_b.open(ctx, symbols_b, n_b, n_sites, DevSymbols::PLANE);
    if (rc != SNPGPU_OK) return rc;
    uint32_t *d_a = (uint32_t *)dev_a.extra(), *d_b = d_a + n_pairs;
    int32_t *d_out = (int32_t *)(d_b + n_pairs);
    HIP_TRY(ctx, hipMemcpyAsync(d_a, a, (size_t)n_pairs * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_b, b, (size_t)n_pairs * 4, hipMemcpyHostToDevice, st));
    rc = snpgpu_compared_pairs_dev(ctx, dev_a.plane(), n_a, symbols_b ? dev_b.plane() : dev_a.plane(), n_b, n_sites, d_a, d_b, n_pairs, d_out);
    if (rc != SNPGPU_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(out, d_out, (size_t)n_pairs * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return SNPGPU_OK;
}

}  // extern "C"
