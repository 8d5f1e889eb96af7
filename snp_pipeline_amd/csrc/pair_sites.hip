// The differing sites of sample pairs: which columns of the packed matrix of distance.hip stand behind each distance.
//
// Additive: the reference leaves "by which SNPs do these two isolates differ?" to whoever reads snpma.fasta and snplist.txt
// (snppipeline/distance.py:93-106 prints the count alone).  Column s of pair (a, b) differs iff both bytes, after upper-casing,
// are in {A,C,G,T} and are not equal — the predicate of utils.calculate_sequence_distance (utils.py:1135-1165) and the one
// k_distance counts, so a pair has exactly matrix[a][b] entries.
//
// A wave per pair (grid-stride over the pairs), a 16-byte load of each row per lane and word:
//   a. count: popc(((xh ^ yh) | (xl ^ yl)) & xv & yv) summed over the pair's words;
//   b. an inclusive scan of the counts (prims.h) behind a leading zero: the pairs' offsets;
//   c. emit: in steps of 64 words every lane takes the prefix sum of the popcounts of the lanes below it plus the running base of
//      the pair and walks the set bits of its own mask upwards: site = 32 * word + bit, and one byte of bases out of the code_hi /
//      code_lo / lower planes (low nibble the first sample: bits 0-1 A0 C1 G2 T3, bit 2 lower case; high nibble the second).
// No atomic decides a position: the bytes of the result are a function of the input alone.  The zero words a row is padded with
// never match (valid is 0 there), and no bit at or beyond n_sites is taken whatever the planes hold.  A pair that names a row
// >= n_rows has no entries and raises the status word; a == b has none either.
#include "pair_tiles.h"
#include "prims.h"

#define PAIR_SITES_THREADS 256
#define PAIR_SITES_WAVES (PAIR_SITES_THREADS / 64)
#define PAIR_SITES_GRID_CAP 1024         // workgroups: more pairs than 4 x this go round the grid-stride loop

namespace {

struct AddU64 {
    __device__ uint64_t operator()(const uint64_t &a, const uint64_t &b) const { return a + b; }
};

// bit i = column 32 * w + i counts for the pair
__device__ __forceinline__ uint32_t differing(const uint4 x, const uint4 y, uint32_t w, uint32_t n_sites) {
    const uint32_t first = 32u * w;
    if (first >= n_sites) return 0u;
    const uint32_t left = n_sites - first, m = ((x.y ^ y.y) | (x.z ^ y.z)) & x.x & y.x;
    return left >= 32u ? m : m & ((1u << left) - 1u);
}

__device__ __forceinline__ uint32_t nibble(const uint4 x, uint32_t bit) {
    return ((x.y >> bit) & 1u) << 1 | ((x.z >> bit) & 1u) | ((x.w >> bit) & 1u) << 2;
}

// kEmit = false: pair_cnt[p] = entries of pair p; *status raised by a row index >= n_rows.  kEmit = true: the entries of
// pair p to site / bases from pair_off[p] on.
template <bool kEmit>
__global__ __launch_bounds__(PAIR_SITES_THREADS) void k_pair_sites(const uint4 *packed, uint32_t n_rows, uint32_t n_sites, uint32_t words, const uint32_t *pa,
                                                                   const uint32_t *pb, uint64_t n_pairs, uint64_t *pair_cnt, uint64_t *status,
                                                                   const uint64_t *pair_off, uint32_t *site, uint8_t *bases) {
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t p = (uint64_t)blockIdx.x * PAIR_SITES_WAVES + (threadIdx.x >> 6); p < n_pairs; p += (uint64_t)gridDim.x * PAIR_SITES_WAVES) {
        const uint32_t a = pa[p], b = pb[p];
        if (a >= n_rows || b >= n_rows) {
            if (!kEmit && lane == 0) { pair_cnt[p] = 0; *status = 1; }
            continue;
        }
        if (a == b) {
            if (!kEmit && lane == 0) pair_cnt[p] = 0;
            continue;
        }
        const uint4 *ra = packed + (size_t)a * words, *rb = packed + (size_t)b * words;
        uint64_t run = kEmit ? pair_off[p] : 0;
        uint32_t cnt = 0;
        for (uint32_t w0 = 0; w0 < words; w0 += 64) {                // every lane goes round every step: the wave sums need them all
            const uint32_t w = w0 + lane;
            uint4 x = make_uint4(0, 0, 0, 0), y = x;
            if (w < words) { x = ra[w]; y = rb[w]; }
            uint32_t m = differing(x, y, w, n_sites);
            const uint32_t mine = __popc(m);
            if (!kEmit) { cnt += mine; continue; }
            const uint32_t incl = wave_inclusive_sum(mine);
            uint64_t at = run + (incl - mine);
            while (m) {
                const uint32_t bit = (uint32_t)__ffs((int)m) - 1u;
                m &= m - 1u;
                site[at] = 32u * w + bit;
                bases[at] = (uint8_t)(nibble(x, bit) | nibble(y, bit) << 4);
                ++at;
            }
            run += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        }
        if (!kEmit) {
            const uint32_t total = wave_inclusive_sum(cnt);
            if (lane == 63) pair_cnt[p] = total;
        }
    }
}

inline unsigned grid_for(uint64_t pairs) {
    const uint64_t b = (pairs + PAIR_SITES_WAVES - 1) / PAIR_SITES_WAVES;
    return (unsigned)(b < 1 ? 1 : b < PAIR_SITES_GRID_CAP ? b : PAIR_SITES_GRID_CAP);
}

inline uint32_t words_of(uint32_t n_sites) { return padded_words(n_sites); }

// The count pass and the scan into the context's scratch: *d_off = n_pairs + 1 offsets there, *total on the host (waits for the
// stream).  SNPGPU_E_ARG when a pair names a row >= n_rows or the total reaches 2^32.
int pair_sites_count(snpgpu_ctx *ctx, const void *d_packed, uint32_t n_rows, uint32_t n_sites, const uint32_t *d_a, const uint32_t *d_b, uint64_t n_pairs,
                     uint64_t **d_off, uint64_t *total) {
    void *ws = nullptr;
    const int rc = snpgpu_scratch(ctx, ((size_t)n_pairs + 2 + prim_gscan_blocks(n_pairs) + 2) * 8, &ws);
    if (rc != SNPGPU_OK) return rc;
    uint64_t *off = (uint64_t *)ws, *status = off + n_pairs + 1, *aggr = status + 1;   // the total, off[n_pairs], lies next to the status word
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipMemsetAsync(off, 0, 8, st));
    HIP_TRY(ctx, hipMemsetAsync(status, 0, 8, st));
    if (n_pairs) {
        k_pair_sites<false><<<grid_for(n_pairs), PAIR_SITES_THREADS, 0, st>>>((const uint4 *)d_packed, n_rows, n_sites, words_of(n_sites), d_a, d_b, n_pairs, off + 1,
                                                                             status, nullptr, nullptr, nullptr);
        prim_inclusive_scan(st, off + 1, off + 1, n_pairs, aggr, AddU64());
        HIP_TRY(ctx, hipGetLastError());
    }
    uint64_t back[2] = {0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(back, off + n_pairs, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    *d_off = off;
    *total = back[0];
    if (back[1]) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "a pair names a row outside the %u rows of the matrix", n_rows);
    if (back[0] >> 32) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "the pairs differ at %llu sites: a call holds fewer than 2^32", (unsigned long long)back[0]);
    return SNPGPU_OK;
}

int pair_sites_emit(snpgpu_ctx *ctx, const void *d_packed, uint32_t n_rows, uint32_t n_sites, const uint32_t *d_a, const uint32_t *d_b, uint64_t n_pairs,
                    const uint64_t *d_off, uint32_t *d_site, uint8_t *d_bases) {
    if (!n_pairs) return SNPGPU_OK;
    k_pair_sites<true><<<grid_for(n_pairs), PAIR_SITES_THREADS, 0, ctx->stream>>>((const uint4 *)d_packed, n_rows, n_sites, words_of(n_sites), d_a, d_b, n_pairs, nullptr,
                                                                                 nullptr, d_off, d_site, d_bases);
    HIP_TRY(ctx, hipGetLastError());
    return SNPGPU_OK;
}

// Host pair lists against a packed matrix on the device: upload the lists, count, and — when the entries fit — emit and copy back.
int pair_sites_of_lists(snpgpu_ctx *ctx, const void *d_packed, uint32_t n_rows, uint32_t n_sites, const uint32_t *a, const uint32_t *b, uint64_t n_pairs,
                        uint64_t capacity, uint64_t *out_pair_off, uint32_t *out_site, uint8_t *out_bases, uint64_t *out_n) {
    *out_n = 0;
    for (uint64_t p = 0; p < n_pairs; ++p)
        if (a[p] >= n_rows || b[p] >= n_rows)
            return snpgpu_set_error(ctx, SNPGPU_E_ARG, "pair %llu names row %u of %u", (unsigned long long)p, a[p] >= n_rows ? a[p] : b[p], n_rows);
    if (n_pairs == 0) {
        if (capacity && out_pair_off) out_pair_off[0] = 0;
        return SNPGPU_OK;
    }
    hipStream_t st = ctx->stream;
    void *d_lists = nullptr, *d_out = nullptr;
    hipError_t he = hipMalloc(&d_lists, (size_t)n_pairs * 8);
    if (he != hipSuccess) return snpgpu_set_error(ctx, SNPGPU_E_NOMEM, "hipMalloc failed: %s", hipGetErrorString(he));
    uint32_t *d_a = (uint32_t *)d_lists, *d_b = d_a + n_pairs;
    int rc = SNPGPU_OK;
    uint64_t *d_off = nullptr, total = 0;
    he = hipMemcpyAsync(d_a, a, (size_t)n_pairs * 4, hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipMemcpyAsync(d_b, b, (size_t)n_pairs * 4, hipMemcpyHostToDevice, st);
    if (he == hipSuccess) rc = pair_sites_count(ctx, d_packed, n_rows, n_sites, d_a, d_b, n_pairs, &d_off, &total);
    if (he == hipSuccess && rc == SNPGPU_OK) {
        *out_n = total;
        if (capacity && total <= capacity) {
            if (!out_pair_off || (total && (!out_site || !out_bases))) rc = snpgpu_set_error(ctx, SNPGPU_E_ARG, "null pair-sites output");
            if (rc == SNPGPU_OK && total) {
                const hipError_t hm = hipMalloc(&d_out, total * 5);
                if (hm != hipSuccess) rc = snpgpu_set_error(ctx, SNPGPU_E_NOMEM, "hipMalloc failed: %s", hipGetErrorString(hm));
            }
            uint32_t *d_site = (uint32_t *)d_out;
            uint8_t *d_bases = (uint8_t *)d_out + total * 4;
            if (rc == SNPGPU_OK && total) rc = pair_sites_emit(ctx, d_packed, n_rows, n_sites, d_a, d_b, n_pairs, d_off, d_site, d_bases);
            if (rc == SNPGPU_OK) he = hipMemcpyAsync(out_pair_off, d_off, ((size_t)n_pairs + 1) * 8, hipMemcpyDeviceToHost, st);
            if (rc == SNPGPU_OK && he == hipSuccess && total) he = hipMemcpyAsync(out_site, d_site, total * 4, hipMemcpyDeviceToHost, st);
            if (rc == SNPGPU_OK && he == hipSuccess && total) he = hipMemcpyAsync(out_bases, d_bases, total, hipMemcpyDeviceToHost, st);
        }
    }
    const hipError_t hs = hipStreamSynchronize(st);
    if (he == hipSuccess) he = hs;
    (void)hipFree(d_out);
    (void)hipFree(d_lists);
    if (he != hipSuccess) return snpgpu_set_error(ctx, SNPGPU_E_HIP, "pair sites failed: %s", hipGetErrorString(he));
    return rc;
}

}  // namespace

extern "C" {

int snpgpu_pair_sites_dev(snpgpu_ctx *ctx, const void *d_packed, uint32_t n_rows, uint32_t n_sites, const uint32_t *d_a, const uint32_t *d_b, uint64_t n_pairs,
                          uint64_t capacity, uint64_t *d_pair_off, uint32_t *d_site, uint8_t *d_bases, uint64_t *out_n) {
    if (!ctx) return SNPGPU_E_ARG;
    if (!out_n) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "bad pair-sites arguments");
    *out_n = 0;
    if (n_pairs && (!d_a || !d_b || ((uintptr_t)d_a & 3) || ((uintptr_t)d_b & 3))) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "the pair lists are null or not 4-byte aligned");
    if (((uintptr_t)d_packed & 15) || (n_pairs && n_rows && n_sites && !d_packed)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "the packed matrix is null or not 16-byte aligned");
    HIP_TRY(ctx, snpgpu_enter(ctx));
    uint64_t *d_off = nullptr, total = 0;
    const int rc = pair_sites_count(ctx, d_packed, n_rows, n_sites, d_a, d_b, n_pairs, &d_off, &total);
    if (rc != SNPGPU_OK) return rc;
    *out_n = total;
    if (capacity == 0 || total > capacity) return SNPGPU_OK;
    if (!d_pair_off || (total && (!d_site || !d_bases))) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null pair-sites output");
    HIP_TRY(ctx, hipMemcpyAsync(d_pair_off, d_off, ((size_t)n_pairs + 1) * 8, hipMemcpyDeviceToDevice, ctx->stream));
    if (!total) return SNPGPU_OK;
    return pair_sites_emit(ctx, d_packed, n_rows, n_sites, d_a, d_b, n_pairs, d_off, d_site, d_bases);
}

int snpgpu_pair_sites(snpgpu_ctx *ctx, const uint8_t *symbols, uint32_t n_rows, uint32_t n_sites, const uint32_t *a, const uint32_t *b, uint64_t n_pairs,
                      uint64_t capacity, uint64_t *out_pair_off, uint32_t *out_site, uint8_t *out_bases, uint64_t *out_n) {
    if (!ctx) return SNPGPU_E_ARG;
    if (!out_n || (n_rows && n_sites && !symbols) || (n_pairs && (!a || !b))) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null pair-sites argument");
    HIP_TRY(ctx, snpgpu_enter(ctx));
    DevSymbols dev;
    int rc = dev.open(ctx, symbols, n_rows, n_sites);
    if (rc == SNPGPU_OK) rc = pair_sites_of_lists(ctx, dev.packed(), n_rows, n_sites, a, b, n_pairs, capacity, out_pair_off, out_site, out_bases, out_n);
    if (rc != SNPGPU_OK) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return SNPGPU_OK;
}

int snpgpu_pair_sites_kept(snpgpu_ctx *ctx, const uint32_t *a, const uint32_t *b, uint64_t n_pairs, uint64_t capacity, uint64_t *out_pair_off, uint32_t *out_site,
                           uint8_t *out_bases, uint64_t *out_n) {
    if (!ctx) return SNPGPU_E_ARG;
    if (!out_n || (n_pairs && (!a || !b))) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null pair-sites argument");
    if (!ctx->kept_packed) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "the context keeps no packed matrix");
    HIP_TRY(ctx, snpgpu_enter(ctx));
    return pair_sites_of_lists(ctx, ctx->kept_packed, ctx->kept_rows, ctx->kept_sites, a, b, n_pairs, capacity, out_pair_off, out_site, out_bases, out_n);
}

int snpgpu_packed_drop(snpgpu_ctx *ctx) {
    if (!ctx) return SNPGPU_E_ARG;
    if (!ctx->kept_packed) return SNPGPU_OK;
    HIP_TRY(ctx, snpgpu_enter(ctx));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    (void)hipFree(ctx->kept_packed);
    ctx->kept_packed = nullptr;
    ctx->kept_rows = ctx->kept_sites = 0;
    return SNPGPU_OK;
}

}  // extern "C"
