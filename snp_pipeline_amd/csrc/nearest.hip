// Query-against-database nearest neighbours of the distance step: q query rows against n database rows, and per query the K
// closest database samples within T.
//
// Additive: distance.calculate_snp_distances (snppipeline/distance.py:93-106) knows one symmetric matrix over one snpma.fasta;
// a user who holds n isolates and receives q new ones wants q rows of the (n + q)^2 matrix.  The predicate is the one
// distance.hip counts (utils.py:1135-1165): both bytes in ACGT after upper-casing, and different.
//
//   a. k_distance_rect_*: the q x n block of distances of two packed matrices (snpgpu_pack_matrix_dev, the same n_sites) into an
//      int32 matrix with a row pitch.  Rows past either matrix read that matrix's last row and are never stored.  Two tile shapes:
//        tile    128 query rows x 128 database rows, 8 x 8 pairs per lane: the sweep pair_tiles.h describes on a plain grid of tiles,
//                VALU-bound.
//        narrow  the slab scheme of that sweep (LDS-DMA one slab ahead into a double buffer, one barrier per slab) in another
//                geometry: 16 query rows x 64 database rows, slabs of 16 words, 16 pairs per lane: the four lanes 4 r .. 4 r + 3 share
//                database row r of the tile, lane 4 r + p takes the words 4 j + p of a slab against all 16 queries, and the four
//                partial sums meet in two lane exchanges at the end of the tile.  A database row contributes 256 contiguous
//                bytes per slab (16 lanes of one DMA instruction); the query words of a step are read from LDS at four
//                addresses by the whole wave (broadcasts).  Slot s of row r holds word s ^ ((r & 3) << 2), so the 16 lanes LDS
//                serves together — four rows with four different r & 3 — read 16 different bank groups.  40 KiB of LDS: four
//                workgroups per CU, whose barriers fall at different times, keep the loads of a CU in flight.  Few queries
//                make the sweep of the database HBM-bound; this shape does an eighth of the vector work of the
//                tile shape per database word.
//      Split-K on both routes (pair_split_plan): fewer tiles than CUs and at least 4 slabs of the route.
//   b. k_nearest_rows: per row of such a matrix the entries <= T, ordered by (d, column), the first K of them.  A workgroup per
//      row: count the entries <= T; when K cuts them, find the K-th smallest value d* by a radix select (4 passes of 8 bits over
//      the keys with the sign bit flipped, a 256-bin LDS histogram per pass); the row keeps every entry < d* and the first
//      K - less entries == d* in column order.  The row counts go through a scan (one wait for the total), an emit pass places
//      every kept entry by workgroup prefix sums in column order, and prim_sort — stable — by (row, d) leaves (row, d, column).
//      No atomic decides a position: the same matrix gives the same bytes.
#include "pair_tiles.h"
#include "prims.h"

#define RECT_NQ 16                       // narrow route: query rows
#define RECT_NDB 64                      // ... database rows: four lanes each
#define RECT_NKW 16                      // ... words per slab: 256 contiguous bytes of a row (a power of two, 16 ... 64)
#define RECT_NROWS (RECT_NDB + RECT_NQ)
#define RECT_NARROW_LDS (2 * RECT_NROWS * RECT_NKW * 16)
#define RECT_NARROW_PER_CU (160 * 1024 / RECT_NARROW_LDS)     // workgroups of the narrow route a CU's LDS holds
#define RECT_AUTO_NARROW_MAX_Q 64        // route 0: narrow up to here (measured, profiles/r21/nearest.md: 1.2 ms against 1.4 ms at 64
                                         // queries x 10 000 x 200 000, 2.6 ms against 1.4 ms at 128)
#define NEAREST_THREADS 256
#define NEAREST_ROW_GRID_CAP 1024        // workgroups of the row kernels: more rows than this go round their grid-stride loop

namespace {

template <bool kSplit>
__global__ __launch_bounds__(PAIR_THREADS, 3) void k_distance_rect_tile(PairArgs a) {
    // [buffer][operand][row][slot]; a wave's 64 DMA lanes fill 64 consecutive 16-byte slots
    __shared__ uint4 slab[2][2][PAIR_TILE][PAIR_SLOTS];
    constexpr int kPieces = PAIR_TILE * PAIR_SLOTS / PAIR_THREADS;
    const uint32_t tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (uint64_t gg = blockIdx.x;; gg += gridDim.x) {
        uint32_t k_begin, k_end;
        const uint64_t t = pair_part<kSplit>(gg, a, k_begin, k_end);
        if (t >= a.total_tiles) break;
        const uint32_t r0 = (uint32_t)(t / a.tiles_n) * PAIR_TILE, c0 = (uint32_t)(t % a.tiles_n) * PAIR_TILE;
        int32_t acc[8][8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[i][j] = 0;

        // DMA: chunk p = e * 256 + tid of an operand's slab is slot (p & 3) of row (p >> 2)
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
        request(k_begin, 0);
        int buf = 0;
        for (uint32_t k0 = k_begin; k0 < k_end; k0 += PAIR_SLOTS, buf ^= 1) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // my part of this slab has landed ...
            __syncthreads();                                        // ... everybody's has, and the slab before has been read
            if (k0 + PAIR_SLOTS < k_end) request(k0 + PAIR_SLOTS, buf ^ 1);
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
                    for (int j = 0; j < 8; ++j) acc[i][j] = DistanceWord()(x[i], y[j], acc[i][j]);
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
                if (kSplit) { if (acc[i][j]) atomicAdd(&a.out[(size_t)r * a.stride + c], acc[i][j]); }
                else a.out[(size_t)r * a.stride + c] = acc[i][j];
            }
        }
    }
}

template <bool kSplit>
__global__ __launch_bounds__(PAIR_THREADS) void k_distance_rect_narrow(PairArgs a) {
    // [buffer][row][slot]: rows 0 .. 63 the database rows of the tile, 64 .. 79 the query rows
    extern __shared__ uint4 rect_lds[];
    const uint32_t tid = threadIdx.x;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t lds0 = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) char *)rect_lds);
    // DMA: chunk p = e * 256 + tid of a slab is slot p % RECT_NKW of row p / RECT_NKW: RECT_NKW consecutive lanes read the
    // contiguous bytes a row contributes.  The first pieces are database rows, the last RECT_NQ * RECT_NKW / 256 the query
    // rows; neither the slot nor (row & 3) depends on e.
    constexpr int kPieces = RECT_NROWS * RECT_NKW / PAIR_THREADS, kDbPieces = RECT_NDB * RECT_NKW / PAIR_THREADS, kRowsPerPiece = PAIR_THREADS / RECT_NKW;
    const uint32_t dma_row = tid / RECT_NKW, word_of = (tid % RECT_NKW) ^ ((dma_row & 3u) << 2);
    // arithmetic: the four lanes 4 r .. 4 r + 3 share database row r of the tile; lane 4 r + p takes the words 4 j + p
    const uint32_t my_row = tid >> 2, my_part = tid & 3u, my_swizzle = (my_row & 3u) << 2;
    for (uint64_t gg = blockIdx.x;; gg += gridDim.x) {
        uint32_t k_begin, k_end;                                    // words: a slot of the packed matrix is one word
        const uint64_t t = pair_part<kSplit>(gg, a, k_begin, k_end);
        if (t >= a.total_tiles) break;
        const uint32_t r0 = (uint32_t)(t / a.tiles_n) * RECT_NQ, c0 = (uint32_t)(t % a.tiles_n) * RECT_NDB;
        int32_t acc[RECT_NQ];
#pragma unroll
        for (int i = 0; i < RECT_NQ; ++i) acc[i] = 0;
        const uint4 *row_ptr[kPieces];
#pragma unroll
        for (int e = 0; e < kDbPieces; ++e) {
            const uint32_t c = c0 + e * kRowsPerPiece + dma_row;
            row_ptr[e] = a.pdb + (size_t)(c < a.n ? c : a.n - 1) * a.slots;
        }
#pragma unroll
        for (int e = kDbPieces; e < kPieces; ++e) {
            const uint32_t r = r0 + (e - kDbPieces) * kRowsPerPiece + dma_row;
            row_ptr[e] = a.pq + (size_t)(r < a.q ? r : a.q - 1) * a.slots;
        }
        auto request = [&](uint32_t k0, int buf) {
            // the last slab of a range may be short (rows are padded to 4 words, not to a slab): its missing words read the
            // row's last word instead and are never used
            const uint32_t w = k0 + word_of < a.slots ? k0 + word_of : a.slots - 1;
#pragma unroll
            for (int e = 0; e < kPieces; ++e)
                lds_dma16(row_ptr[e] + w, lds0 + ((uint32_t)buf * RECT_NROWS * RECT_NKW + e * PAIR_THREADS + wave * 64) * 16);
        };
        __syncthreads();                                            // the previous tile's last slab has been read
        request(k_begin, 0);
        int buf = 0;
        for (uint32_t k0 = k_begin; k0 < k_end; k0 += RECT_NKW, buf ^= 1) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // my part of this slab has landed ...
            __syncthreads();                                        // ... everybody's has, and the slab before has been read
            if (k0 + RECT_NKW < k_end) request(k0 + RECT_NKW, buf ^ 1);
            const uint32_t nw = k_end - k0 < RECT_NKW ? k_end - k0 : RECT_NKW;       // a multiple of 4: every lane has nw / 4 words
            const uint4 *db = rect_lds + (size_t)buf * RECT_NROWS * RECT_NKW + my_row * RECT_NKW, *qs = rect_lds + ((size_t)buf * RECT_NROWS + RECT_NDB) * RECT_NKW;
            for (uint32_t k = my_part; k < nw; k += 4) {
                const uint4 y = db[k ^ my_swizzle];
#pragma unroll
                for (uint32_t i = 0; i < RECT_NQ; ++i) acc[i] = DistanceWord()(qs[i * RECT_NKW + (k ^ ((i & 3u) << 2))], y, acc[i]);
            }
        }
#pragma unroll
        for (uint32_t i = 0; i < RECT_NQ; ++i) {                    // the four partial sums of a row
            acc[i] += __shfl_xor(acc[i], 1);
            acc[i] += __shfl_xor(acc[i], 2);
        }
        const uint32_t c = c0 + my_row;
        if (my_part == 0 && c < a.n) {
#pragma unroll
            for (uint32_t i = 0; i < RECT_NQ; ++i) {
                const uint32_t r = r0 + i;
                if (r >= a.q) continue;
                if (kSplit) { if (acc[i]) atomicAdd(&a.out[(size_t)r * a.stride + c], acc[i]); }
                else a.out[(size_t)r * a.stride + c] = acc[i];
            }
        }
    }
}

// ---- selection ----
struct AddU64 {
    __device__ uint64_t operator()(const uint64_t &a, const uint64_t &b) const { return a + b; }
};
struct Entry { uint32_t row; int32_t d; uint32_t col; };
struct EntryLess {
    __device__ bool operator()(const Entry &a, const Entry &b) const { return a.row != b.row ? a.row < b.row : a.d < b.d; }
};

// kEmit = false: row_cnt[r] = entries row r keeps, cut[r] = the value below which every entry is kept, take_eq[r] = how many
// entries equal to it are kept, in column order (all of them: 0xFFFFFFFF).  kEmit = true: the kept entries to `out` from
// row_off[r] on, in column order.
template <bool kEmit>
__global__ __launch_bounds__(NEAREST_THREADS) void k_nearest_rows(const int32_t *mat, uint64_t stride, uint32_t n, uint32_t rows, uint32_t k, int32_t thr,
                                                                  uint64_t *row_cnt, int32_t *cut, uint32_t *take_eq, const uint64_t *row_off, Entry *out) {
    __shared__ uint32_t red_a[17], red_b[17];
    __shared__ uint32_t hist[256];
    __shared__ uint32_t chosen[2];                                   // the bin of the pass, the rank inside it
    const uint32_t tid = threadIdx.x;
    for (uint32_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const int32_t *row = mat + (uint64_t)r * stride;
        if (!kEmit) {
            uint32_t cnt = 0, within;
            for (uint32_t c = tid; c < n; c += NEAREST_THREADS) cnt += row[c] <= thr;
            (void)block_exclusive_sum(cnt, red_a, within);
            __syncthreads();
            if (k == 0 || within <= k) {
                if (tid == 0) { row_cnt[r] = within; cut[r] = thr; take_eq[r] = 0xFFFFFFFFu; }
                continue;
            }
            // more than k entries within thr: the k-th smallest of the row is one of them
            uint32_t prefix = 0, mask = 0, want = k;                // the keys that match prefix under mask hold the want-th smallest
            for (int shift = 24; shift >= 0; shift -= 8) {
                hist[tid] = 0;
                __syncthreads();
                for (uint32_t c = tid; c < n; c += NEAREST_THREADS) {
                    const uint32_t key = (uint32_t)row[c] ^ 0x80000000u;
                    if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
                }
                __syncthreads();
                const uint32_t h = hist[tid];
                uint32_t all;
                const uint32_t before = block_exclusive_sum(h, red_b, all);
                if (before < want && want <= before + h) { chosen[0] = tid; chosen[1] = want - before; }
                __syncthreads();
                prefix |= chosen[0] << shift;
                mask |= 255u << shift;
                want = chosen[1];
                __syncthreads();
            }
            if (tid == 0) { row_cnt[r] = k; cut[r] = (int32_t)(prefix ^ 0x80000000u); take_eq[r] = want; }
        } else {
            const int32_t d_cut = cut[r];
            const uint32_t eq_room = take_eq[r];
            uint64_t run = row_off[r];
            uint32_t eq_run = 0;
            for (uint32_t c0 = 0; c0 < n; c0 += NEAREST_THREADS) {
                const uint32_t c = c0 + tid;
                const int32_t v = c < n ? row[c] : 0;
                const uint32_t eq = c < n && v == d_cut, lt = c < n && v < d_cut;
                uint32_t eq_all, sel_all;
                const uint32_t eq_before = eq_run + block_exclusive_sum(eq, red_a, eq_all);
                const uint32_t sel = lt | (eq & (uint32_t)(eq_before < eq_room));
                const uint32_t at = block_exclusive_sum(sel, red_b, sel_all);
                if (sel) { Entry e; e.row = r; e.d = v; e.col = c; out[run + at] = e; }
                run += sel_all;
                eq_run += eq_all;
            }
        }
    }
}

__global__ __launch_bounds__(NEAREST_THREADS) void k_nearest_split(const Entry *in, uint64_t n, uint32_t *col, int32_t *dist) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const Entry e = in[i];
        col[i] = e.col;
        dist[i] = e.d;
    }
}

// The count pass and the scan into the context's scratch: *d_off = rows + 1 offsets there (cut / take_eq behind them), *total on
// the host (waits for the stream).
int nearest_count(snpgpu_ctx *ctx, const int32_t *d_matrix, uint32_t q, uint32_t n, uint64_t row_stride, uint32_t k, int32_t threshold, uint64_t **d_off,
                  int32_t **d_cut, uint32_t **d_take, uint64_t *total) {
    void *ws = nullptr;
    const size_t w_aggr = prim_gscan_blocks(q) + 2;
    const int rc = snpgpu_scratch(ctx, ((size_t)q + 1 + w_aggr) * 8 + (size_t)q * 8 + 64, &ws);
    if (rc != SNPGPU_OK) return rc;
    uint64_t *off = (uint64_t *)ws, *aggr = off + q + 1;
    int32_t *cut = (int32_t *)(aggr + w_aggr);
    uint32_t *take = (uint32_t *)(cut + q);
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipMemsetAsync(off, 0, 8, st));
    k_nearest_rows<false><<<q < NEAREST_ROW_GRID_CAP ? q : NEAREST_ROW_GRID_CAP, NEAREST_THREADS, 0, st>>>(d_matrix, row_stride, n, q, k, threshold, off + 1, cut, take,
                                                                                                         nullptr, nullptr);
    prim_inclusive_scan(st, off + 1, off + 1, (uint64_t)q, aggr, AddU64());
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(total, off + q, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    *d_off = off;
    *d_cut = cut;
    *d_take = take;
    return SNPGPU_OK;
}

// The emit pass, the sort by (row, d) and the two arrays; `total` entries, at least one.
int nearest_emit(snpgpu_ctx *ctx, const int32_t *d_matrix, uint32_t q, uint32_t n, uint64_t row_stride, const uint64_t *d_off, const int32_t *d_cut,
                 const uint32_t *d_take, uint64_t total, uint32_t *d_col, int32_t *d_dist) {
    void *d = nullptr;
    const hipError_t he = hipMalloc(&d, 3 * total * sizeof(Entry) + 64);
    if (he != hipSuccess) return snpgpu_set_error(ctx, SNPGPU_E_NOMEM, "hipMalloc failed: %s", hipGetErrorString(he));
    Entry *in = (Entry *)d, *buf_a = in + total, *buf_b = buf_a + total;
    uint32_t *flag = (uint32_t *)(buf_b + total);
    hipStream_t st = ctx->stream;
    k_nearest_rows<true><<<q < NEAREST_ROW_GRID_CAP ? q : NEAREST_ROW_GRID_CAP, NEAREST_THREADS, 0, st>>>(d_matrix, row_stride, n, q, 0, 0, nullptr,
                                                                                                        const_cast<int32_t *>(d_cut), const_cast<uint32_t *>(d_take), d_off, in);
    const Entry *sorted = prim_sort(st, in, buf_a, buf_b, total, flag, EntryLess());
    const uint64_t blocks = (total + NEAREST_THREADS - 1) / NEAREST_THREADS;
    k_nearest_split<<<(unsigned)(blocks < 2048 ? blocks : 2048), NEAREST_THREADS, 0, st>>>(sorted, total, d_col, d_dist);
    hipError_t e = hipGetLastError();
    const hipError_t es = hipStreamSynchronize(st);                 // (the workspace goes before the call returns)
    if (e == hipSuccess) e = es;
    (void)hipFree(d);
    if (e != hipSuccess) return snpgpu_set_error(ctx, SNPGPU_E_HIP, "nearest failed: %s", hipGetErrorString(e));
    return SNPGPU_OK;
}

}  // namespace

extern "C" {

int snpgpu_distance_rect_packed_dev(snpgpu_ctx *ctx, const void *d_packed_q, uint32_t q, const void *d_packed_db, uint32_t n, uint32_t n_sites, int route,
                                    int32_t *d_out, uint64_t out_stride) {
    if (!ctx) return SNPGPU_E_ARG;
    if (route < 0 || route > 2) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "bad route %d (0 auto, 1 narrow, 2 tile)", route);
    if (q == 0 || n == 0) return SNPGPU_OK;
    if (!d_out || ((uintptr_t)d_out & 3) || out_stride < n) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "the output is null, not 4-byte aligned or its pitch is below n");
    if (n_sites && (!d_packed_q || !d_packed_db || (((uintptr_t)d_packed_q | (uintptr_t)d_packed_db) & 15)))
        return snpgpu_set_error(ctx, SNPGPU_E_ARG, "a packed matrix is null or not 16-byte aligned");
    HIP_TRY(ctx, snpgpu_enter(ctx));
    hipStream_t st = ctx->stream;
    PairArgs a;
    a.pq = (const uint4 *)d_packed_q;
    a.pdb = (const uint4 *)d_packed_db;
    a.q = q;
    a.n = n;
    a.slots = padded_words(n_sites);
    a.tile_rank = 0;
    a.tile_nranks = 1;
    a.out = d_out;
    a.stride = out_stride;
    if (a.slots == 0) {                                         // no sites at all: every distance is 0
        HIP_TRY(ctx, hipMemset2DAsync(d_out, out_stride * 4, 0, (size_t)n * 4, q, st));
        return SNPGPU_OK;
    }
    const bool narrow = route == 1 || (route == 0 && q <= RECT_AUTO_NARROW_MAX_Q);
    const uint32_t tiles_q = narrow ? (q + RECT_NQ - 1) / RECT_NQ : (q + PAIR_TILE - 1) / PAIR_TILE;
    a.tiles_n = narrow ? (n + RECT_NDB - 1) / RECT_NDB : (n + PAIR_TILE - 1) / PAIR_TILE;
    a.total_tiles = (uint64_t)tiles_q * a.tiles_n;
    const uint64_t cap = (uint64_t)ctx->n_cu * 64;
    const size_t lds = narrow ? RECT_NARROW_LDS : 0;
    if (narrow) {                                               // (per device; the call is cheap)
        HIP_TRY(ctx, hipFuncSetAttribute((const void *)k_distance_rect_narrow<false>, hipFuncAttributeMaxDynamicSharedMemorySize, RECT_NARROW_LDS));
        HIP_TRY(ctx, hipFuncSetAttribute((const void *)k_distance_rect_narrow<true>, hipFuncAttributeMaxDynamicSharedMemorySize, RECT_NARROW_LDS));
    }
    hipEvent_t ta = snpgpu_time_begin(ctx);
    // the parts wanted.  tile: k_distance's count.  narrow: as many as keep every workgroup resident at once (LDS bounds them per CU) —
    // a part more would start a second round of workgroups that a few CUs run alone; at least 4 parts, for tiles < n_cu
    const uint64_t parts = narrow ? (uint64_t)ctx->n_cu * RECT_NARROW_PER_CU / a.total_tiles : ((uint64_t)ctx->n_cu * 2 + a.total_tiles - 1) / a.total_tiles;
    if (pair_split_plan(a.slots, narrow ? RECT_NKW : PAIR_SLOTS, a.total_tiles, ctx->n_cu, parts, &a.k_chunk, &a.k_parts)) {
        HIP_TRY(ctx, hipMemset2DAsync(d_out, out_stride * 4, 0, (size_t)n * 4, q, st));
        const unsigned grid = (unsigned)(a.total_tiles * a.k_parts);
        if (narrow) k_distance_rect_narrow<true><<<grid, PAIR_THREADS, lds, st>>>(a);
        else k_distance_rect_tile<true><<<grid, PAIR_THREADS, 0, st>>>(a);
    } else {
        const unsigned grid = (unsigned)(a.total_tiles < cap ? a.total_tiles : cap);
        if (narrow) k_distance_rect_narrow<false><<<grid, PAIR_THREADS, lds, st>>>(a);
        else k_distance_rect_tile<false><<<grid, PAIR_THREADS, 0, st>>>(a);
    }
    snpgpu_time_end(ctx, SNPGPU_K_DISTANCE, ta);
    HIP_TRY(ctx, hipGetLastError());
    return SNPGPU_OK;
}

int snpgpu_nearest_dev(snpgpu_ctx *ctx, const int32_t *d_matrix, uint32_t q, uint32_t n, uint64_t row_stride, uint32_t k, int32_t threshold, uint64_t capacity,
                       uint64_t *d_row_off, uint32_t *d_col, int32_t *d_dist, uint64_t *out_n) {
    if (!ctx) return SNPGPU_E_ARG;
    if (!out_n || row_stride < n) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "bad nearest arguments");
    if (((uintptr_t)d_matrix & 3) || (q && n && !d_matrix)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "the matrix is null or not 4-byte aligned");
    HIP_TRY(ctx, snpgpu_enter(ctx));
    *out_n = 0;
    if (q == 0 || n == 0) {                                     // no entries: the offsets are all zero
        if (capacity && !d_row_off) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null nearest output");
        if (capacity) HIP_TRY(ctx, hipMemsetAsync(d_row_off, 0, ((size_t)q + 1) * 8, ctx->stream));
        return SNPGPU_OK;
    }
    uint64_t *d_off = nullptr, total = 0;
    int32_t *d_cut = nullptr;
    uint32_t *d_take = nullptr;
    const int rc = nearest_count(ctx, d_matrix, q, n, row_stride, k, threshold, &d_off, &d_cut, &d_take, &total);
    if (rc != SNPGPU_OK) return rc;
    *out_n = total;
    if (capacity == 0 || total > capacity) return SNPGPU_OK;
    if (!d_row_off || (total && (!d_col || !d_dist))) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null nearest output");
    HIP_TRY(ctx, hipMemcpyAsync(d_row_off, d_off, ((size_t)q + 1) * 8, hipMemcpyDeviceToDevice, ctx->stream));
    if (total == 0) return SNPGPU_OK;
    return nearest_emit(ctx, d_matrix, q, n, row_stride, d_off, d_cut, d_take, total, d_col, d_dist);
}

int snpgpu_nearest(snpgpu_ctx *ctx, const uint8_t *q_symbols, uint32_t q, const uint8_t *db_symbols, uint32_t n, uint32_t n_sites, uint32_t k, int32_t threshold,
                   uint32_t band_rows, int route, uint64_t capacity, uint64_t *out_row_off, uint32_t *out_col, int32_t *out_dist, uint64_t *out_n,
                   int32_t *out_matrix) {
    if (!ctx) return SNPGPU_E_ARG;
    if (route < 0 || route > 2) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "bad route %d (0 auto, 1 narrow, 2 tile)", route);
    if (!out_n || (n_sites && ((q && !q_symbols) || (n && !db_symbols)))) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null nearest argument");
    if (capacity && !out_row_off) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null nearest output");
    HIP_TRY(ctx, snpgpu_enter(ctx));
    *out_n = 0;
    if (q == 0 || n == 0) {
        if (capacity) for (uint32_t i = 0; i <= q; ++i) out_row_off[i] = 0;
        return SNPGPU_OK;
    }
    size_t free_b = 0, total_b = 0;
    HIP_TRY(ctx, hipMemGetInfo(&free_b, &total_b));
    const size_t row_b = snpgpu_packed_row_bytes(n_sites);
    if (band_rows == 0) {                                       // the largest band whose matrix stays within a quarter of the free memory
        const uint64_t fit = (uint64_t)(free_b / 4) / ((uint64_t)n * 4);
        band_rows = (uint32_t)(fit < 1 ? 1 : fit < q ? fit : q);
    }
    if (band_rows > q) band_rows = q;
    DevSymbols dev_db, dev_q;                                   // both matrices are uploaded and packed once; the band's matrix behind the database
    int rc = dev_db.open(ctx, db_symbols, n, n_sites, 0, nullptr, (size_t)band_rows * n * 4);
    if (rc == SNPGPU_OK) rc = dev_q.open(ctx, q_symbols, q, n_sites);
    if (rc != SNPGPU_OK) return rc;
    const char *d_dbp = (const char *)dev_db.packed(), *d_qp = (const char *)dev_q.packed();
    int32_t *d_mat = (int32_t *)dev_db.extra();
    void *d_csr = nullptr;
    hipError_t he = hipSuccess;
    hipStream_t st = ctx->stream;
    uint64_t csr_room = 0, running = 0;
    std::vector<uint64_t> h_off((size_t)band_rows + 1);
    if (capacity) out_row_off[0] = 0;
    for (uint32_t lo = 0; lo < q && he == hipSuccess && rc == SNPGPU_OK; lo += band_rows) {      // queries are independent: banding is exact
        const uint32_t rows = q - lo < band_rows ? q - lo : band_rows;
        rc = snpgpu_distance_rect_packed_dev(ctx, d_qp + (size_t)lo * row_b, rows, d_dbp, n, n_sites, route, d_mat, n);
        if (rc != SNPGPU_OK) break;
        if (out_matrix) he = hipMemcpyAsync(out_matrix + (size_t)lo * n, d_mat, (size_t)rows * n * 4, hipMemcpyDeviceToHost, st);
        if (he != hipSuccess) break;
        uint64_t *d_off = nullptr, total = 0;
        int32_t *d_cut = nullptr;
        uint32_t *d_take = nullptr;
        rc = nearest_count(ctx, d_mat, rows, n, n, k, threshold, &d_off, &d_cut, &d_take, &total);
        if (rc != SNPGPU_OK) break;
        const uint64_t before = running;
        running += total;
        if (capacity == 0 || running > capacity) continue;      // past the capacity the remaining bands are only counted
        he = hipMemcpyAsync(h_off.data(), d_off, ((size_t)rows + 1) * 8, hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipStreamSynchronize(st);
        if (he != hipSuccess) break;
        for (uint32_t i = 1; i <= rows; ++i) out_row_off[lo + i] = before + h_off[i];
        if (total == 0) continue;
        if (!out_col || !out_dist) { rc = snpgpu_set_error(ctx, SNPGPU_E_ARG, "null nearest output"); break; }
        if (total > csr_room) {
            (void)hipFree(d_csr);
            d_csr = nullptr;
            csr_room = 0;
            const hipError_t hm = hipMalloc(&d_csr, total * 8);
            if (hm != hipSuccess) { rc = snpgpu_set_error(ctx, SNPGPU_E_NOMEM, "hipMalloc failed: %s", hipGetErrorString(hm)); break; }
            csr_room = total;
        }
        uint32_t *d_col = (uint32_t *)d_csr;
        int32_t *d_dist = (int32_t *)d_csr + total;
        rc = nearest_emit(ctx, d_mat, rows, n, n, d_off, d_cut, d_take, total, d_col, d_dist);
        if (rc != SNPGPU_OK) break;
        he = hipMemcpyAsync(out_col + before, d_col, total * 4, hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipMemcpyAsync(out_dist + before, d_dist, total * 4, hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipStreamSynchronize(st);
    }
    const hipError_t hs = hipStreamSynchronize(st);
    if (he == hipSuccess) he = hs;
    (void)hipFree(d_csr);
    if (he != hipSuccess) return snpgpu_set_error(ctx, SNPGPU_E_HIP, "nearest failed: %s", hipGetErrorString(he));
    if (rc == SNPGPU_OK) *out_n = running;
    return rc;
}

}  // extern "C"
