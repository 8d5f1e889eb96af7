// Bootstrap support values of the neighbour-joining tree (Felsenstein's bootstrap): B more runs of k_distance (distance.hip) and of
// the NJ rounds (nj.hip) over resampled columns, and how many of the B replicate trees hold each bipartition of the main tree.
//
// Additive, like nj.hip: the reference stops at the two tables (snppipeline/distance.py:93-115).  Nothing the reference writes changes,
// and without the new options every command writes what it wrote.
//
// The statement (include/snpgpu.h has it in full; tests/nj_bootstrap_cases.py restates it in Python).  Modulo 2^64:
//   G = 0x9E3779B97F4A7C15;  mix(z): z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; z ^ (z >> 31)
//   draw(seed, b, k) = mix(mix(seed + G (b + 1)) + G (k + 1));  c(b, k) = the high half of draw(seed, b, k) * s
// Replicate b is the distance matrix over the multiset of columns {c(b, k)} and its NJ tree.  Join record t of a tree of n >= 4 samples
// defines the leaf set under the new node; canonical is the side WITHOUT sample 0: W = ceil(n / 64) 64-bit words, bit i of word i / 64
// sample i, bits >= n zero.  Support(t) = the number of replicates whose tree holds main bipartition t.  NJ is stated in integers with
// a pinned tie-break, so every replicate tree is unique and so are the counts.
//
//   k_boot_columns   c(b, .) of one replicate, a thread per position, in draw order.
//   k_boot_max       the largest entry of a caller's column list into a flag (a vector atomic max): the public resample entry waits
//                    for it and refuses an index >= s before anything is written.  The driver's own lists need no check: c(b, k) < s.
//   k_boot_resample  the pack of sym[:, cols] from the pack of sym.  A wave owns 64 consecutive output sites: every lane loads its
//                    column ONCE, then for row after row loads the uint4 {valid, hi, lo, lower} of its column's word, takes its bit of
//                    each plane, and four ballots give the two output words, which lanes 0 and 1 store as k_pack_matrix does.  Lanes
//                    past the last column contribute zeros, so padding bits and padding words are zero.  BOOT_ROWS rows' loads are
//                    in flight together.  With sorted columns the 64 lanes of a wave read two or three neighbouring words of a row
//                    and the waves of a workgroup walk every source row forwards.
//   k_nj_splits      a workgroup per tree; thread w owns word w (w + blockDim.x, ...) of every slot's set: set[i] = {i}; per join
//                    set[a][w] |= set[b][w], then emit.  Word w of every set is only ever touched by one thread: no barrier and no
//                    atomic between the joins.  A slot is its smallest sample, so the set of slot a holds sample 0 iff a == 0: then the
//                    complement is emitted, its tail in the last word masked.  The sets live in n W words of global workspace per tree.
//                    Records that name a slot >= n (never from nj_run) emit zeros and touch nothing.
//   k_split_iota / prim_sort / k_split_count   the main tree's row indices sorted by their W words (lexicographic from word 0); a wave
//                    per replicate row binary-searches that order, every probe comparing 64 words at once (a ballot finds the first
//                    word that differs).  The comparison is exact on all W words: no hash, no collision path.  Main bipartitions are
//                    distinct, so a row matches at most one; the count is an integer atomicAdd (the value does not depend on the order).
// Driver (snpgpu_nj_bootstrap): upload and pack once, the main matrix and tree; per replicate columns, sort (prim_sort), resample,
// snpgpu_distance_packed_dev, nj_run into the one resampled pack and the one n x n matrix, keeping 8 bytes per join on the device; then
// bipartitions and counts in bands of trees sized from the free device memory (as nearest.hip sizes its bands).  Only the main tree and
// n - 3 counts cross the host link.  Not done: the B replicates' NJ rounds batched in one launch per round.
// Only vector atomics (global_atomic_umax in k_boot_max, global_atomic_add in k_split_count) and plain stores.
//
// gfx950, hipcc -O3 (-Rpass-analysis=kernel-resource-usage): k_boot_columns 32 VGPRs, 38 SGPRs; k_boot_max 17 VGPRs; k_boot_resample 30 VGPRs,
// 24 SGPRs; k_nj_splits 16 VGPRs, 42 SGPRs; k_split_iota 4 VGPRs; k_split_count 12 VGPRs, 46 SGPRs; none of them uses LDS.  The two sorts of
// prims.h as instantiated here: tile sort 12 (columns) / 22 (rows) VGPRs and 12 288 bytes of LDS, merge pass 46 VGPRs and 8 208 bytes.  No
// spill and no scratch in any of them.
#include "pair_tiles.h"
#include "nj_host.h"
#include "prims.h"

#define BOOT_THREADS 256
#define BOOT_ROWS 4                      // rows of a resample step whose loads are in flight together
#define BOOT_G 0x9E3779B97F4A7C15ull

namespace {

__host__ __device__ __forceinline__ uint64_t boot_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// base = mix(seed + G (b + 1)), the same for the whole replicate
__global__ __launch_bounds__(BOOT_THREADS) void k_boot_columns(uint64_t base, uint32_t s, uint32_t *out) {
    for (uint64_t k = (uint64_t)blockIdx.x * BOOT_THREADS + threadIdx.x; k < s; k += (uint64_t)gridDim.x * BOOT_THREADS)
        out[k] = (uint32_t)__umul64hi(boot_mix(base + BOOT_G * (k + 1)), (uint64_t)s);
}

__global__ __launch_bounds__(BOOT_THREADS) void k_boot_max(const uint32_t *cols, uint32_t n, uint32_t *flag) {
    uint32_t most = 0;
    for (uint64_t k = (uint64_t)blockIdx.x * BOOT_THREADS + threadIdx.x; k < n; k += (uint64_t)gridDim.x * BOOT_THREADS) {
        const uint32_t c = cols[k];
        most = c > most ? c : most;
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)most, m);
        most = o > most ? o : most;
    }
    if ((threadIdx.x & 63) == 0 && most) atomicMax(flag, most);
}

// dst_words is a multiple of PAIR_SLOTS = 4 (padded_words of pair_tiles.h), so a row is dst_words / 2 groups of 64 sites; every column is below 32 * src_words
__global__ __launch_bounds__(BOOT_THREADS) void k_boot_resample(const uint4 *src, uint32_t n_rows, uint32_t src_words, const uint32_t *cols, uint32_t n_cols,
                                                                uint4 *dst, uint32_t dst_words) {
    const uint32_t lane = threadIdx.x & 63, grp = blockIdx.x * (BOOT_THREADS / 64) + (threadIdx.x >> 6);
    if (grp >= dst_words / 2) return;                                // (the same for the whole wave; no barrier follows)
    const uint32_t site = grp * 64 + lane;
    const bool in = site < n_cols;
    const uint32_t c = in ? cols[site] : 0u, word = c >> 5, bit = c & 31u;
    for (uint32_t r0 = blockIdx.y * BOOT_ROWS; r0 < n_rows; r0 += gridDim.y * BOOT_ROWS) {
        uint4 v[BOOT_ROWS];
#pragma unroll
        for (uint32_t u = 0; u < BOOT_ROWS; ++u)
            v[u] = (in && r0 + u < n_rows) ? src[(size_t)(r0 + u) * src_words + word] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
        for (uint32_t u = 0; u < BOOT_ROWS; ++u) {
            if (r0 + u >= n_rows) break;                             // (the same for the whole wave)
            const uint64_t V = __ballot((v[u].x >> bit) & 1u), H = __ballot((v[u].y >> bit) & 1u), Lo = __ballot((v[u].z >> bit) & 1u),
                           Lc = __ballot((v[u].w >> bit) & 1u);
            if (lane < 2) {
                const uint32_t sh = lane * 32;
                dst[(size_t)(r0 + u) * dst_words + grp * 2 + lane] = make_uint4((uint32_t)(V >> sh), (uint32_t)(H >> sh), (uint32_t)(Lo >> sh), (uint32_t)(Lc >> sh));
            }
        }
    }
}

// tree blockIdx.x: its joins at a / b + tree * (n - 3), its n * W words of sets, its (n - 3) * W words of output.  n >= 4.
__global__ __launch_bounds__(BOOT_THREADS) void k_nj_splits(const uint32_t *a, const uint32_t *b, uint32_t n, uint32_t W, uint64_t *sets, uint64_t *out) {
    const uint32_t joins = n - 3;
    a += (size_t)blockIdx.x * joins;
    b += (size_t)blockIdx.x * joins;
    sets += (size_t)blockIdx.x * n * W;
    out += (size_t)blockIdx.x * joins * W;
    for (uint32_t w = threadIdx.x; w < W; w += blockDim.x) {
        const uint64_t tail = (w == W - 1 && (n & 63u)) ? (1ull << (n & 63u)) - 1 : ~0ull;
        for (uint32_t i = 0; i < n; ++i) sets[(size_t)i * W + w] = (i >> 6) == w ? 1ull << (i & 63u) : 0ull;
        for (uint32_t t = 0; t < joins; ++t) {
            const uint32_t ai = a[t], bi = b[t];
            if (ai >= n || bi >= n) { out[(size_t)t * W + w] = 0; continue; }     // (never from nj_run)
            const uint64_t v = sets[(size_t)ai * W + w] | sets[(size_t)bi * W + w];
            sets[(size_t)ai * W + w] = v;
            out[(size_t)t * W + w] = ai == 0 ? ~v & tail : v;        // (slot 0 is the one that holds sample 0)
        }
    }
}

struct U32Less {
    __device__ bool operator()(const uint32_t &x, const uint32_t &y) const { return x < y; }
};

// rows of W words, lexicographic from word 0
struct SplitLess {
    const uint64_t *rows;
    uint32_t W;
    __device__ bool operator()(const uint32_t &x, const uint32_t &y) const {
        const uint64_t *p = rows + (size_t)x * W, *q = rows + (size_t)y * W;
        for (uint32_t w = 0; w < W; ++w)
            if (p[w] != q[w]) return p[w] < q[w];
        return false;
    }
};

__global__ __launch_bounds__(BOOT_THREADS) void k_split_iota(uint32_t *idx, uint32_t n) {
    const uint32_t i = blockIdx.x * BOOT_THREADS + threadIdx.x;
    if (i < n) idx[i] = i;
}

// a wave per replicate row: the binary search over the sorted main rows; counts[the main row equal to it] += 1
__global__ __launch_bounds__(BOOT_THREADS) void k_split_count(const uint64_t *main_rows, const uint32_t *order, uint32_t n_main, const uint64_t *rep, uint64_t n_rep,
                                                              uint32_t W, uint32_t *counts) {
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t row = (uint64_t)blockIdx.x * (BOOT_THREADS / 64) + (threadIdx.x >> 6); row < n_rep; row += (uint64_t)gridDim.x * (BOOT_THREADS / 64)) {
        const uint64_t *x = rep + row * W;
        uint32_t lo = 0, hi = n_main;
        while (lo < hi) {                                            // (lo, hi and cmp are the same for the whole wave)
            const uint32_t mid = lo + ((hi - lo) >> 1), at = order[mid];
            const uint64_t *m = main_rows + (size_t)at * W;
            int cmp = 0;
            for (uint32_t w0 = 0; w0 < W && cmp == 0; w0 += 64) {
                const bool have = w0 + lane < W;
                const uint64_t xv = have ? x[w0 + lane] : 0ull, mv = have ? m[w0 + lane] : 0ull;
                const uint64_t differ = __ballot(xv != mv), less = __ballot(xv < mv);
                if (differ) cmp = (less >> (__ffsll((unsigned long long)differ) - 1)) & 1ull ? -1 : 1;
            }
            if (cmp == 0) {
                if (lane == 0) atomicAdd(counts + at, 1u);
                break;
            }
            if (cmp < 0) hi = mid; else lo = mid + 1;
        }
    }
}

inline uint32_t packed_words(uint32_t n_sites) { return padded_words(n_sites); }
inline uint32_t split_words(uint32_t n) { return (n + 63) / 64; }

void columns_run(snpgpu_ctx *ctx, uint64_t seed, uint32_t replicate, uint32_t s, uint32_t *d_cols) {
    if (s == 0) return;
    const uint64_t base = boot_mix(seed + BOOT_G * ((uint64_t)replicate + 1));
    const uint32_t blocks = (s + BOOT_THREADS - 1) / BOOT_THREADS, cap = (uint32_t)ctx->n_cu * 32;
    k_boot_columns<<<blocks < cap ? blocks : cap, BOOT_THREADS, 0, ctx->stream>>>(base, s, d_cols);
}

// c(replicate, .) ascending; d_ws: 3 s words and one for the sort's flag.  Returns where in d_ws they end up.
const uint32_t *sorted_columns_run(snpgpu_ctx *ctx, uint64_t seed, uint32_t replicate, uint32_t s, uint32_t *d_ws) {
    columns_run(ctx, seed, replicate, s, d_ws);
    return prim_sort(ctx->stream, d_ws, d_ws + s, d_ws + 2 * (size_t)s, s, d_ws + 3 * (size_t)s, U32Less{});
}

// columns all below n_sites (the caller knows); n_rows, n_cols >= 1
void resample_run(snpgpu_ctx *ctx, const void *d_packed, uint32_t n_rows, uint32_t n_sites, const uint32_t *d_cols, uint32_t n_cols, void *d_out) {
    const uint32_t dst_words = packed_words(n_cols), gx = (dst_words / 2 + BOOT_THREADS / 64 - 1) / (BOOT_THREADS / 64);
    const uint32_t steps = (n_rows + BOOT_ROWS - 1) / BOOT_ROWS, fill = ((uint32_t)ctx->n_cu * 8 + gx - 1) / gx;
    const uint32_t gy = fill < steps ? fill : steps;
    k_boot_resample<<<dim3(gx, gy < 65535u ? gy : 65535u), BOOT_THREADS, 0, ctx->stream>>>((const uint4 *)d_packed, n_rows, packed_words(n_sites), d_cols, n_cols, (uint4 *)d_out,
                                                                                      dst_words);
}

size_t splits_workspace_bytes(uint32_t n, uint32_t n_trees) { return (size_t)n_trees * n * split_words(n) * 8; }

// n >= 4, n_trees >= 1; d_sets: splits_workspace_bytes
void splits_run(snpgpu_ctx *ctx, const uint32_t *d_a, const uint32_t *d_b, uint32_t n, uint32_t n_trees, uint64_t *d_sets, uint64_t *d_out) {
    const uint32_t W = split_words(n);
    k_nj_splits<<<n_trees, W <= 64 ? 64 : BOOT_THREADS, 0, ctx->stream>>>(d_a, d_b, n, W, d_sets, d_out);
}

// the main rows' indices in their order; d_idx: 3 * n_main words and one for the flag.  Returns where the order ends up.
const uint32_t *support_sort(snpgpu_ctx *ctx, const uint64_t *d_main, uint32_t n_main, uint32_t W, uint32_t *d_idx) {
    k_split_iota<<<(n_main + BOOT_THREADS - 1) / BOOT_THREADS, BOOT_THREADS, 0, ctx->stream>>>(d_idx, n_main);
    return prim_sort(ctx->stream, d_idx, d_idx + n_main, d_idx + 2 * (size_t)n_main, n_main, d_idx + 3 * (size_t)n_main, SplitLess{d_main, W});
}

void support_count(snpgpu_ctx *ctx, const uint64_t *d_main, const uint32_t *d_order, uint32_t n_main, const uint64_t *d_rep, uint64_t n_rep, uint32_t W,
                   uint32_t *d_counts) {
    if (n_main == 0 || n_rep == 0) return;
    const uint64_t blocks = (n_rep + BOOT_THREADS / 64 - 1) / (BOOT_THREADS / 64), cap = (uint64_t)ctx->n_cu * 32;
    k_split_count<<<(unsigned)(blocks < cap ? blocks : cap), BOOT_THREADS, 0, ctx->stream>>>(d_main, d_order, n_main, d_rep, n_rep, W, d_counts);
}

// device memory that waits for the stream before it goes
struct DevBlock {
    snpgpu_ctx *ctx = nullptr;
    void *p = nullptr;
    int get(snpgpu_ctx *c, size_t bytes) {
        ctx = c;
        const hipError_t he = hipMalloc(&p, bytes ? bytes : 1);
        if (he != hipSuccess) { p = nullptr; return snpgpu_set_error(ctx, SNPGPU_E_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(he)); }
        return SNPGPU_OK;
    }
    ~DevBlock() {
        if (!p) return;
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(p);
    }
};

void boot_no_star(uint32_t *star, int64_t *star_len) {
    for (int s = 0; s < 3; ++s) { star[s] = NJ_NONE; star_len[s] = 0; }
}

inline size_t up256(size_t x) { return (x + 255) / 256 * 256; }

// n >= 4: the main tree of dev's matrix to the host, the replicates, the counts
int bootstrap_run(snpgpu_ctx *ctx, const DevSymbols &dev, uint32_t n, uint32_t s, uint32_t replicates, uint64_t seed, uint32_t *out_a, uint32_t *out_b,
                  int64_t *out_len_a, int64_t *out_len_b, uint32_t *out_star, int64_t *out_star_len, uint32_t *out_support) {
    hipStream_t st = ctx->stream;
    const size_t k = n - 3, W = split_words(n), row_bytes = snpgpu_packed_row_bytes(s);
    // 8-byte arrays first: the main lengths, the replicates' lengths (read by nobody), the main bipartitions; then the 4-byte ones
    const size_t o_len = 0, o_tmp = o_len + up256(k * 16), o_main = o_tmp + up256(k * 16), o_ab = o_main + up256(k * W * 8), o_rep = o_ab + up256(k * 8);
    const size_t o_cols = o_rep + up256((size_t)replicates * k * 8), o_counts = o_cols + up256(((size_t)s * 3 + 1) * 4), o_idx = o_counts + up256(k * 4);
    const size_t o_pack = o_idx + up256((k * 3 + 1) * 4), o_mat = o_pack + up256(row_bytes * n + 256), total = o_mat + up256((size_t)n * n * 4);
    DevBlock blk;
    int rc = blk.get(ctx, total);
    if (rc != SNPGPU_OK) return rc;
    char *d = (char *)blk.p;
    int64_t *d_la = (int64_t *)(d + o_len), *d_lb = d_la + k, *d_tla = (int64_t *)(d + o_tmp), *d_tlb = d_tla + k;
    uint64_t *d_main = (uint64_t *)(d + o_main);
    uint32_t *d_a = (uint32_t *)(d + o_ab), *d_b = d_a + k, *d_ra = (uint32_t *)(d + o_rep), *d_rb = d_ra + (size_t)replicates * k;
    uint32_t *d_cols = (uint32_t *)(d + o_cols), *d_counts = (uint32_t *)(d + o_counts), *d_idx = (uint32_t *)(d + o_idx);
    void *d_pack = d + o_pack;
    int32_t *d_mat = (int32_t *)(d + o_mat);

    rc = nj_run(ctx, dev.matrix(), n, n, d_a, d_b, d_la, d_lb, out_star, out_star_len);
    if (rc != SNPGPU_OK) return rc;
    for (uint32_t rep = 0; rep < replicates; ++rep) {
        if (s) {
            const uint32_t *sorted = sorted_columns_run(ctx, seed, rep, s, d_cols);
            resample_run(ctx, dev.packed(), n, s, sorted, s, d_pack);
            HIP_TRY(ctx, hipGetLastError());
        }
        rc = snpgpu_distance_packed_dev(ctx, d_pack, n, s, 0, 1, d_mat);
        uint32_t star[3];
        int64_t star_len[3];
        if (rc == SNPGPU_OK) rc = nj_run(ctx, d_mat, n, n, d_ra + (size_t)rep * k, d_rb + (size_t)rep * k, d_tla, d_tlb, star, star_len);
        if (rc != SNPGPU_OK) return rc;
    }
    // the bands: as many trees at once as a quarter of the free memory holds (a tree: its sets and its bipartitions)
    size_t free_b = 0, total_b = 0;
    HIP_TRY(ctx, hipMemGetInfo(&free_b, &total_b));
    const size_t per_tree = splits_workspace_bytes(n, 1) + k * W * 8;
    const uint64_t fit = (uint64_t)(free_b / 4) / per_tree;
    const uint32_t band = (uint32_t)(fit < 1 ? 1 : fit < replicates ? fit : replicates);
    DevBlock ws;
    rc = ws.get(ctx, per_tree * band);
    if (rc != SNPGPU_OK) return rc;
    uint64_t *d_sets = (uint64_t *)ws.p, *d_rows = d_sets + (size_t)band * n * W;
    HIP_TRY(ctx, hipMemsetAsync(d_counts, 0, k * 4, st));
    splits_run(ctx, d_a, d_b, n, 1, d_sets, d_main);
    const uint32_t *d_order = support_sort(ctx, d_main, (uint32_t)k, (uint32_t)W, d_idx);
    for (uint32_t t0 = 0; t0 < replicates; t0 += band) {
        const uint32_t trees = replicates - t0 < band ? replicates - t0 : band;
        splits_run(ctx, d_ra + (size_t)t0 * k, d_rb + (size_t)t0 * k, n, trees, d_sets, d_rows);
        support_count(ctx, d_main, d_order, (uint32_t)k, d_rows, (uint64_t)trees * k, (uint32_t)W, d_counts);
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(out_len_a, d_la, k * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(out_len_b, d_lb, k * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(out_a, d_a, k * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(out_b, d_b, k * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(out_support, d_counts, k * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return SNPGPU_OK;
}

}  // namespace

extern "C" {

int snpgpu_bootstrap_columns_dev(snpgpu_ctx *ctx, uint64_t seed, uint32_t replicate, uint32_t n_sites, uint32_t *d_cols) {
    if (!ctx) return SNPGPU_E_ARG;
    if (n_sites == 0) return SNPGPU_OK;
    if (!d_cols || ((uintptr_t)d_cols & 3)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "the column array is null or not 4-byte aligned");
    HIP_TRY(ctx, snpgpu_enter(ctx));
    columns_run(ctx, seed, replicate, n_sites, d_cols);
    HIP_TRY(ctx, hipGetLastError());
    return SNPGPU_OK;
}

int snpgpu_bootstrap_columns_sorted_dev(snpgpu_ctx *ctx, uint64_t seed, uint32_t replicate, uint32_t n_sites, uint32_t *d_cols) {
    if (!ctx) return SNPGPU_E_ARG;
    if (n_sites == 0) return SNPGPU_OK;
    if (!d_cols || ((uintptr_t)d_cols & 3)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "the column array is null or not 4-byte aligned");
    HIP_TRY(ctx, snpgpu_enter(ctx));
    DevBlock ws;
    const int rc = ws.get(ctx, ((size_t)n_sites * 3 + 1) * 4);
    if (rc != SNPGPU_OK) return rc;
    const uint32_t *sorted = sorted_columns_run(ctx, seed, replicate, n_sites, (uint32_t *)ws.p);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(d_cols, sorted, (size_t)n_sites * 4, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return SNPGPU_OK;
}

int snpgpu_resample_packed_dev(snpgpu_ctx *ctx, const void *d_packed, uint32_t n_rows, uint32_t n_sites, const uint32_t *d_cols, uint32_t n_cols, void *d_out) {
    if (!ctx) return SNPGPU_E_ARG;
    if (n_rows == 0 || n_cols == 0) return SNPGPU_OK;
    if (!d_packed || !d_cols || !d_out || ((uintptr_t)d_packed & 15) || ((uintptr_t)d_out & 15) || ((uintptr_t)d_cols & 3))
        return snpgpu_set_error(ctx, SNPGPU_E_ARG, "bad resample arguments");
    if (n_sites == 0) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "a column list of a matrix without a column");
    HIP_TRY(ctx, snpgpu_enter(ctx));
    void *flag = nullptr;                                            // the largest index of the list, before anything is written
    const int rc = snpgpu_scratch(ctx, 4, &flag);
    if (rc != SNPGPU_OK) return rc;
    uint32_t most = 0;
    HIP_TRY(ctx, hipMemsetAsync(flag, 0, 4, ctx->stream));
    const uint32_t blocks = (n_cols + BOOT_THREADS - 1) / BOOT_THREADS, cap = (uint32_t)ctx->n_cu * 32;
    k_boot_max<<<blocks < cap ? blocks : cap, BOOT_THREADS, 0, ctx->stream>>>(d_cols, n_cols, (uint32_t *)flag);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(&most, flag, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (most >= n_sites) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "column %u of the list is not one of the %u columns", most, n_sites);
    resample_run(ctx, d_packed, n_rows, n_sites, d_cols, n_cols, d_out);
    HIP_TRY(ctx, hipGetLastError());
    return SNPGPU_OK;
}

int snpgpu_nj_splits_dev(snpgpu_ctx *ctx, const uint32_t *d_a, const uint32_t *d_b, uint32_t n, uint32_t n_trees, uint64_t *d_out) {
    if (!ctx) return SNPGPU_E_ARG;
    if (n <= 3 || n_trees == 0) return SNPGPU_OK;
    if (!d_a || !d_b || !d_out || ((uintptr_t)d_a & 3) || ((uintptr_t)d_b & 3) || ((uintptr_t)d_out & 7)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "bad bipartition arguments");
    HIP_TRY(ctx, snpgpu_enter(ctx));
    DevBlock ws;
    const int rc = ws.get(ctx, splits_workspace_bytes(n, n_trees));
    if (rc != SNPGPU_OK) return rc;
    splits_run(ctx, d_a, d_b, n, n_trees, (uint64_t *)ws.p, d_out);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return SNPGPU_OK;
}

int snpgpu_split_support_dev(snpgpu_ctx *ctx, const uint64_t *d_main, uint32_t n_main, const uint64_t *d_rep, uint64_t n_rep, uint32_t n_words, uint32_t *d_counts) {
    if (!ctx) return SNPGPU_E_ARG;
    if (n_main == 0) return SNPGPU_OK;
    if (!d_main || !d_counts || n_words == 0 || (n_rep && !d_rep) || ((uintptr_t)d_main & 7) || ((uintptr_t)d_rep & 7) || ((uintptr_t)d_counts & 3))
        return snpgpu_set_error(ctx, SNPGPU_E_ARG, "bad support arguments");
    HIP_TRY(ctx, snpgpu_enter(ctx));
    DevBlock idx;
    const int rc = idx.get(ctx, ((size_t)n_main * 3 + 1) * 4);
    if (rc != SNPGPU_OK) return rc;
    HIP_TRY(ctx, hipMemsetAsync(d_counts, 0, (size_t)n_main * 4, ctx->stream));
    const uint32_t *d_order = support_sort(ctx, d_main, n_main, n_words, (uint32_t *)idx.p);
    support_count(ctx, d_main, d_order, n_main, d_rep, n_rep, n_words, d_counts);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return SNPGPU_OK;
}

int snpgpu_nj_bootstrap(snpgpu_ctx *ctx, const uint8_t *symbols, uint32_t n_rows, uint32_t n_sites, uint32_t replicates, uint64_t seed, uint32_t *out_a, uint32_t *out_b,
                        int64_t *out_len_a, int64_t *out_len_b, int32_t *out_matrix, uint32_t *out_star, int64_t *out_star_len, uint32_t *out_n_merges,
                        uint32_t *out_support) {
    if (!ctx) return SNPGPU_E_ARG;
    if (!out_n_merges || !out_star || !out_star_len || (n_rows && n_sites && !symbols)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "bad bootstrap arguments");
    if (n_rows > 3 && (!out_a || !out_b || !out_len_a || !out_len_b || !out_support)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null bootstrap output");
    if (replicates == 0) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "the bootstrap needs one replicate at least");
    *out_n_merges = 0;
    boot_no_star(out_star, out_star_len);
    if (n_rows == 0) return SNPGPU_OK;
    HIP_TRY(ctx, snpgpu_enter(ctx));
    DevSymbols dev;
    int rc = dev.open(ctx, symbols, n_rows, n_sites, DevSymbols::MATRIX, out_matrix);
    if (rc == SNPGPU_OK && n_rows > 1 && n_rows <= 3)                // a star alone: nothing to count
        rc = nj_run(ctx, dev.matrix(), n_rows, n_rows, nullptr, nullptr, nullptr, nullptr, out_star, out_star_len);
    if (rc == SNPGPU_OK && n_rows > 3)
        rc = bootstrap_run(ctx, dev, n_rows, n_sites, replicates, seed, out_a, out_b, out_len_a, out_len_b, out_star, out_star_len, out_support);
    if (rc != SNPGPU_OK) { boot_no_star(out_star, out_star_len); return rc; }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *out_n_merges = n_rows > 3 ? n_rows - 3 : 0;
    return SNPGPU_OK;
}

}  // extern "C"
