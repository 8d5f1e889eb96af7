// K4-pack + K5: samples x sites matrix packed 4 bits/site, and the all-pairs SNP distance.
//
// Replaces utils.calculate_sequence_distance (snppipeline/utils.py:1135-1165) called for every pair by
// distance.calculate_snp_distances (snppipeline/distance.py:93-98):  a site counts for a pair iff, after
// upper-casing, both bytes are in {A,C,G,T} and they differ.
//
// The packed layout, the predicate and the slab scheme of the 128 x 128 tile sweep k_distance runs: pair_tiles.h.
#include "pair_tiles.h"

extern "C" size_t snpgpu_packed_row_bytes(uint32_t n_sites) { return (size_t)padded_words(n_sites) * 16; }

// One wavefront packs 64 consecutive sites of one row: coalesced byte loads, four ballots.
__global__ __launch_bounds__(256) void k_pack_matrix(const uint8_t *sym, uint32_t n_rows, uint32_t n_sites, size_t stride,
                                                     uint4 *packed, uint32_t words) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t groups_per_row = (words + 1) / 2;
    const uint64_t total = (uint64_t)n_rows * groups_per_row;
    for (uint64_t g = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); g < total; g += (uint64_t)gridDim.x * 4) {
        uint32_t row = (uint32_t)(g / groups_per_row);
        uint32_t grp = (uint32_t)(g % groups_per_row);
        uint32_t site = grp * 64 + lane;
        uint32_t c = site < n_sites ? sym[(size_t)row * stride + site] : 0u;
        uint32_t u = to_upper(c);
        bool v = (u == 'A') | (u == 'C') | (u == 'G') | (u == 'T');
        bool hi = (u == 'G') | (u == 'T');
        bool lo = (u == 'C') | (u == 'T');
        uint64_t V = __ballot(v), H = __ballot(v && hi), Lo = __ballot(v && lo), Lc = __ballot(c != u);
        if (lane < 2) {
            uint32_t w = grp * 2 + lane;
            if (w < words) {
                uint32_t sh = lane * 32;
                packed[(size_t)row * words + w] = make_uint4((uint32_t)(V >> sh), (uint32_t)(H >> sh), (uint32_t)(Lo >> sh), (uint32_t)(Lc >> sh));
            }
        }
    }
}

// kSplit: a few tiles only (small sample counts): every tile is shared by k_parts workgroups, each sums its range of
// words and adds it to the (zeroed) output with integer atomics — the result does not depend on the order.
template <bool kSplit>
__global__ __launch_bounds__(PAIR_THREADS, 3) void k_distance(PairArgs a) {
    // [buffer][operand][row][slot]; a wave's 64 DMA lanes fill 64 consecutive 16-byte slots
    __shared__ uint4 slab[2][2][PAIR_TILE][PAIR_SLOTS];
    const uint32_t tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (uint64_t gg = blockIdx.x;; gg += gridDim.x) {
        uint32_t k_begin, k_end;
        const uint64_t g = pair_part<kSplit>(gg, a, k_begin, k_end);
        uint64_t t = (uint64_t)a.tile_rank + g * a.tile_nranks;
        if (t >= a.total_tiles) break;
        uint32_t bi, bj;
        triangle_coords(t, a.tiles_n, bi, bj);
        const uint32_t r0 = bi * PAIR_TILE, c0 = bj * PAIR_TILE;
        int32_t acc[8][8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[i][j] = 0;

        // DMA: chunk p = e * 256 + tid of an operand's slab is slot (p & 3) of row (p >> 2).  Rows past the matrix read
        // the last row instead (their pairs are never stored).
        uint32_t row_of[2][PAIR_TILE * PAIR_SLOTS / PAIR_THREADS], kk_of[PAIR_TILE * PAIR_SLOTS / PAIR_THREADS];
#pragma unroll
        for (int e = 0; e < PAIR_TILE * PAIR_SLOTS / PAIR_THREADS; ++e) {
            const uint32_t p = e * PAIR_THREADS + tid, rr = p >> 2;
            kk_of[e] = (p & 3u) ^ ((rr >> 2) & 3u);
            row_of[0][e] = r0 + rr < a.n ? r0 + rr : a.n - 1;
            row_of[1][e] = c0 + rr < a.n ? c0 + rr : a.n - 1;
        }
        auto request = [&](uint32_t k0, int buf) {
#pragma unroll
            for (int op = 0; op < 2; ++op)
#pragma unroll
                for (int e = 0; e < PAIR_TILE * PAIR_SLOTS / PAIR_THREADS; ++e) {
                    const uint4 *gp = a.pq + ((size_t)row_of[op][e] * a.slots + (k0 + kk_of[e]));
                    lds_dma16(gp, (uint32_t)(uintptr_t)((__attribute__((address_space(3))) char *)&slab[buf][op][0][0]) + (e * PAIR_THREADS + wave * 64) * 16);
                }
        };
        __syncthreads();                                            // the previous tile's last slab has been read
        request(k_begin, 0);
        int buf = 0;
        for (uint32_t k0 = k_begin; k0 < k_end; k0 += PAIR_SLOTS, buf ^= 1) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // my part of this slab has landed ...
            __syncthreads();                                        // ... everybody's has, and slab k0 - KW has been read
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
            uint32_t r = r0 + ty + 16 * i;                          // (the pitch of the square matrix is n: 32-bit, not a.stride)
            if (r >= a.n) continue;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                uint32_t c = c0 + tx + 16 * j;
                if (c >= a.n) continue;
                if (kSplit) {
                    if (acc[i][j]) {
                        atomicAdd(&a.out[(size_t)r * a.n + c], acc[i][j]);
                        if (bi != bj) atomicAdd(&a.out[(size_t)c * a.n + r], acc[i][j]);
                    }
                } else {
                    a.out[(size_t)r * a.n + c] = acc[i][j];
                    if (bi != bj) a.out[(size_t)c * a.n + r] = acc[i][j];
                }
            }
        }
    }
}

// zero the tiles (and mirror images) a rank owns, before a split-K accumulation
__global__ __launch_bounds__(PAIR_THREADS) void k_distance_zero(PairArgs a) {
    for (uint64_t g = blockIdx.x;; g += gridDim.x) {
        uint64_t t = (uint64_t)a.tile_rank + g * a.tile_nranks;
        if (t >= a.total_tiles) break;
        uint32_t bi, bj;
        triangle_coords(t, a.tiles_n, bi, bj);
        for (uint32_t e = threadIdx.x; e < PAIR_TILE * PAIR_TILE; e += PAIR_THREADS) {
            uint32_t r = bi * PAIR_TILE + e / PAIR_TILE, c = bj * PAIR_TILE + e % PAIR_TILE;
            if (r < a.n && c < a.n) { a.out[(size_t)r * a.n + c] = 0; a.out[(size_t)c * a.n + r] = 0; }
        }
    }
}

extern "C" {

int snpgpu_pack_matrix_dev(snpgpu_ctx *ctx, const uint8_t *d_symbols, uint32_t n_rows, uint32_t n_sites,
                           size_t row_stride, void *d_packed) {
    if (!ctx) return SNPGPU_E_ARG;
    if (n_rows == 0 || n_sites == 0) return SNPGPU_OK;
    if (!d_symbols || !d_packed || row_stride < n_sites) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "bad pack arguments");
    HIP_TRY(ctx, snpgpu_enter(ctx));
    uint32_t words = padded_words(n_sites);                 // the padding words come out all zero (no valid site)
    uint64_t groups = (uint64_t)n_rows * ((words + 1) / 2);
    uint64_t blocks = (groups + 3) / 4, cap = (uint64_t)ctx->n_cu * 32;
    k_pack_matrix<<<(unsigned)(blocks < cap ? blocks : cap), 256, 0, ctx->stream>>>(d_symbols, n_rows, n_sites, row_stride, (uint4 *)d_packed, words);
    HIP_TRY(ctx, hipGetLastError());
    return SNPGPU_OK;
}

int snpgpu_distance_packed_dev(snpgpu_ctx *ctx, const void *d_packed, uint32_t n_rows, uint32_t n_sites,
                               uint32_t tile_rank, uint32_t tile_nranks, int32_t *d_out) {
    if (!ctx) return SNPGPU_E_ARG;
    if (tile_nranks == 0 || tile_rank >= tile_nranks) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "bad tile rank %u of %u", tile_rank, tile_nranks);
    if (n_rows == 0) return SNPGPU_OK;
    if (!d_out || (n_sites && !d_packed)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null distance argument");
    HIP_TRY(ctx, snpgpu_enter(ctx));
    PairArgs a;
    a.pq = a.pdb = (const uint4 *)d_packed;
    a.q = a.n = n_rows;
    a.slots = padded_words(n_sites);
    a.tiles_n = (n_rows + PAIR_TILE - 1) / PAIR_TILE;
    a.tile_rank = tile_rank;
    a.tile_nranks = tile_nranks;
    a.total_tiles = (uint64_t)a.tiles_n * (a.tiles_n + 1) / 2;
    a.out = d_out;
    a.stride = n_rows;
    a.k_parts = 1;
    a.k_chunk = a.slots;
    uint64_t mine = a.total_tiles > tile_rank ? (a.total_tiles - tile_rank + tile_nranks - 1) / tile_nranks : 0;
    if (mine == 0) return SNPGPU_OK;
    const uint64_t cap = (uint64_t)ctx->n_cu * 64;
    if (a.slots == 0) {                                         // no sites at all: every distance of the rank's tiles is 0
        k_distance_zero<<<(unsigned)(mine < cap ? mine : cap), PAIR_THREADS, 0, ctx->stream>>>(a);
        HIP_TRY(ctx, hipGetLastError());
        return SNPGPU_OK;
    }
    hipEvent_t ta = snpgpu_time_begin(ctx);
    if (pair_split_plan(a.slots, PAIR_SLOTS, mine, ctx->n_cu, ((uint64_t)ctx->n_cu * 2 + mine - 1) / mine, &a.k_chunk, &a.k_parts)) {
        k_distance_zero<<<(unsigned)mine, PAIR_THREADS, 0, ctx->stream>>>(a);       // this rank's tiles only: ranks share one output
        k_distance<true><<<(unsigned)(mine * a.k_parts), PAIR_THREADS, 0, ctx->stream>>>(a);
    } else {
        k_distance<false><<<(unsigned)(mine < cap ? mine : cap), PAIR_THREADS, 0, ctx->stream>>>(a);
    }
    snpgpu_time_end(ctx, SNPGPU_K_DISTANCE, ta);
    HIP_TRY(ctx, hipGetLastError());
    return SNPGPU_OK;
}

int snpgpu_distance(snpgpu_ctx *ctx, const uint8_t *symbols, uint32_t n_rows, uint32_t n_sites, int32_t *out) {
    if (!ctx) return SNPGPU_E_ARG;
    if (n_rows == 0) return SNPGPU_OK;
    if (!out || (n_sites && !symbols)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null distance argument");
    HIP_TRY(ctx, snpgpu_enter(ctx));
    DevSymbols dev;
    const int rc = dev.open(ctx, symbols, n_rows, n_sites, DevSymbols::MATRIX, out);
    if (rc != SNPGPU_OK) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return SNPGPU_OK;
}

}  // extern "C"

int DevSymbols::open(snpgpu_ctx *c, const uint8_t *symbols, uint32_t n_rows, uint32_t n_sites, int want, int32_t *out_matrix, size_t extra_bytes) {
    ctx = c;
    if (n_rows == 0) return SNPGPU_OK;
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    const size_t sym_bytes = (size_t)n_rows * n_sites, mat_bytes = want & MATRIX ? (size_t)n_rows * n_rows * 4 : 0;
    const size_t o_mat = up(sym_bytes), o_plane = o_mat + up(mat_bytes);
    const size_t o_extra = o_plane + up(want & PLANE ? snpgpu_valid_plane_row_bytes(n_sites) * n_rows : 0);
    hipError_t he = hipMalloc(&block, o_extra + extra_bytes + 256);
    if (he == hipSuccess) he = hipMalloc(&pack, snpgpu_packed_row_bytes(n_sites) * n_rows + 256);   // (read with 16-byte loads past the last word)
    if (he != hipSuccess) return snpgpu_set_error(ctx, SNPGPU_E_NOMEM, "hipMalloc failed: %s", hipGetErrorString(he));
    char *b = (char *)block;
    mat = (int32_t *)(b + o_mat);
    pl = b + o_plane;
    ext = b + o_extra;
    int rc = SNPGPU_OK;
    if (sym_bytes) {
        HIP_TRY(ctx, hipMemcpyAsync(b, symbols, sym_bytes, hipMemcpyHostToDevice, ctx->stream));
        rc = snpgpu_pack_matrix_dev(ctx, (const uint8_t *)b, n_rows, n_sites, n_sites, pack);
    }
    if (rc == SNPGPU_OK && (want & MATRIX)) {
        rc = snpgpu_distance_packed_dev(ctx, pack, n_rows, n_sites, 0, 1, mat);
        if (rc == SNPGPU_OK && out_matrix) HIP_TRY(ctx, hipMemcpyAsync(out_matrix, mat, mat_bytes, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (rc == SNPGPU_OK && (want & PLANE)) rc = snpgpu_valid_plane_dev(ctx, pack, n_rows, n_sites, pl);
    return rc;
}

void *DevSymbols::release_packed() {
    void *p = pack;
    pack = nullptr;
    return p;
}

DevSymbols::~DevSymbols() {
    if (!block && !pack) return;
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(block);
    (void)hipFree(pack);
}
