// Per-site allele counts and cluster-defining SNPs: what a column of the packed matrix of distance.hip looks like, and at which
// columns the members of a cluster share a base that no sample outside the cluster holds.
//
// Additive: nothing in the reference prints the A / C / G / T counts of a column of snpma.fasta, and "which SNPs define this
// cluster" is left to whoever reads the matrix.  A byte is a base iff, after upper-casing, it is one of ACGT — the predicate of
// utils.calculate_sequence_distance (utils.py:1135-1165) and of k_pack_matrix.
//
//   Site counts.    count[s][b] = the rows that hold base b (A0 C1 G2 T3, either case) at column s.
//   Cluster SNPs.   Given labels 1 ... C, (cluster c, column s, base b) is an entry iff some member of c holds b at s, no member
//                   holds another base there, and no sample outside c holds b at s.  Its Members, the members of c that hold b,
//                   then equal count[s][b]: every holder of b is a member.
//
// A lane owns a word (32 sites); a wave reads 64 consecutive uint4 {valid, code_hi, code_lo, lower} of a row, 1 KB coalesced.
//   a. k_sweep: the ONE pass over the packed matrix.  The grid is word tiles (CS_TILE_WORDS) x row chunks (CS_ROW_CHUNK); a
//      wave walks the rows of its chunk, CS_LOADS loads in flight.  The masks of the four bases are three bit operations each.
//      Counts: bit-sliced vertical counters, CS_PLANES planes per base, fed eight rows at a time through a carry-save tree
//      (planes_add8); at the end of the chunk the planes are read out column by column and added (integer atomicAdd: the sum does not
//      depend on the order) to count[s][b].  Presence: the rows are visited in cluster order — a stable sort of (label, row) by
//      prim_sort —, the masks are OR-ed per cluster, and at a change of label P[c][word] = {A, C, G, T} is stored; a cluster
//      that straddles a chunk edge is OR-ed in with atomicOr (zeroed first, with the empty clusters, by k_presence_zero).
//   b. k_unique_part / k_unique: "held by exactly one cluster" per word and base from the associative, commutative pair
//      twice |= once & P; once |= P — over chunks of CS_CLUSTER_CHUNK clusters in parallel, then over the chunks.
//   c. k_rows<false>: a wave per (cluster, word tile) counts popc(rows) where rows_b = P_b & ~(the other three) & unique_b; an
//      inclusive scan (prims.h) behind a leading zero gives every (cluster, tile) its offset — and the clusters theirs;
//      k_rows<true> places the entries by wave prefix sums and walks its set bits upwards: site, base, Members = count[s][b].
// No atomic decides a position or an order-dependent value: the bytes of the result are a function of the input alone.  No bit
// at or beyond n_sites is taken whatever the planes hold.  Traffic: one sweep of the packed matrix (16 B per 32 sites and row)
// for the counts, one for the cluster SNPs of a labelling (counts and presence together); P is C / n_rows of the matrix, written
// once and read twice.
#include "pair_tiles.h"
#include "prims.h"

#define CS_THREADS 256
#define CS_WAVES (CS_THREADS / 64)
#define CS_TILE_WORDS 64         // words (of 32 sites) per wave: a lane owns one
#define CS_ROW_CHUNK 256         // rows a wave walks
#define CS_PLANES 9              // counter planes per base: a chunk counts up to CS_ROW_CHUNK = 2^8
#define CS_LOADS 8               // rows in flight per wave, and the rows one carry-save tree takes
#define CS_CLUSTER_CHUNK 64      // clusters per wave of the first unique pass
#define CS_GRID_CAP_PER_CU 16    // workgroups: more waves than 4 x this x CUs go round the grid-stride loop

static_assert((1u << (CS_PLANES - 1)) >= CS_ROW_CHUNK && CS_PLANES > 3, "the planes hold a chunk's count");
static_assert(CS_LOADS == 8 && CS_ROW_CHUNK % CS_LOADS == 0, "planes_add8 takes eight rows");

namespace {

struct AddU64 {
    __device__ uint64_t operator()(const uint64_t &a, const uint64_t &b) const { return a + b; }
};
struct LessU64 {
    __device__ bool operator()(const uint64_t &a, const uint64_t &b) const { return a < b; }
};

// the wave's number in the launch, as a scalar
__device__ __forceinline__ uint64_t wave_id() { return (uint64_t)blockIdx.x * CS_WAVES + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }
__device__ __forceinline__ uint64_t wave_count() { return (uint64_t)gridDim.x * CS_WAVES; }

// bit i = column 32 * w + i exists
__device__ __forceinline__ uint32_t site_mask(uint32_t w, uint32_t n_sites) {
    const uint64_t first = 32ull * w;
    if (first >= n_sites) return 0u;
    const uint32_t left = n_sites - (uint32_t)first;
    return left >= 32u ? 0xFFFFFFFFu : (1u << left) - 1u;
}

// keys[i] = (label << 32) | i: ascending keys are the stable order by label.  *status raised by a label outside 1 ... n_clusters.
__global__ __launch_bounds__(CS_THREADS) void k_label_keys(const uint32_t *labels, uint32_t n_rows, uint32_t n_clusters, uint64_t *keys, uint32_t *status) {
    for (uint64_t i = (uint64_t)blockIdx.x * CS_THREADS + threadIdx.x; i < n_rows; i += (uint64_t)gridDim.x * CS_THREADS) {
        const uint32_t l = labels[i];
        if (l == 0 || l > n_clusters) *status = 1u;
        keys[i] = (uint64_t)l << 32 | i;
    }
}

// start[c] = the first position of the sorted keys whose label is above c (labels are 1-based: the rows of cluster c, 0-based,
// are [start[c], start[c + 1])); start[n_clusters] = n_rows
__global__ __launch_bounds__(CS_THREADS) void k_cluster_starts(const uint64_t *sorted, uint32_t n_rows, uint32_t n_clusters, uint32_t *start) {
    for (uint64_t c = (uint64_t)blockIdx.x * CS_THREADS + threadIdx.x; c <= n_clusters; c += (uint64_t)gridDim.x * CS_THREADS) {
        uint32_t lo = 0, hi = n_rows;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if ((uint32_t)(sorted[mid] >> 32) <= (uint32_t)c) lo = mid + 1; else hi = mid;
        }
        start[c] = lo;
    }
}

struct SweepArgs {
    const uint4 *packed;
    uint32_t n_rows, n_sites, words;        // words: uint4 per packed row
    uint32_t n_tiles, n_chunks;
    const uint64_t *sorted;                 // presence: the sorted keys of k_label_keys
    const uint32_t *start;                  // presence: k_cluster_starts
    uint4 *presence;                        // [n_clusters][n_tiles * CS_TILE_WORDS] {A, C, G, T}
    int32_t *counts;                        // [n_sites][4], zeroed
};

// a + b + c = 2 high + low, bit by bit
__device__ __forceinline__ void carry_save(uint32_t &high, uint32_t &low, uint32_t a, uint32_t b, uint32_t c) {
    const uint32_t u = a ^ b;
    high = (a & b) | (u & c);
    low = u ^ c;
}

// Eight more sets of 32 one-bit numbers onto the bit-sliced counters: a carry-save tree folds them into the planes of weight 1, 2
// and 4 (seven adders), and what it carries out has weight 8 and ripples through the planes above — 53 operations for eight
// rows, no branch.  (A ripple add per row that stops when the carry is zero across the wave seldom stops early: the 2 048
// counters of a wave differ and one of them carries far.  It measured 0.49 ms for the counts of 10 000 x 200 000, this 0.47.)
__device__ __forceinline__ void planes_add8(uint32_t (&pl)[CS_PLANES], const uint32_t (&d)[CS_LOADS]) {
    uint32_t ta, tb, fa, fb, e;
    carry_save(ta, pl[0], pl[0], d[0], d[1]);
    carry_save(tb, pl[0], pl[0], d[2], d[3]);
    carry_save(fa, pl[1], pl[1], ta, tb);
    carry_save(ta, pl[0], pl[0], d[4], d[5]);
    carry_save(tb, pl[0], pl[0], d[6], d[7]);
    carry_save(fb, pl[1], pl[1], ta, tb);
    carry_save(e, pl[2], pl[2], fa, fb);
#pragma unroll
    for (int p = 3; p < CS_PLANES; ++p) {
        const uint32_t t = pl[p] & e;
        pl[p] ^= e;
        e = t;
    }
}

template <bool kCounts, bool kPresence>
__global__ __launch_bounds__(CS_THREADS) void k_sweep(SweepArgs a) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t total = (uint64_t)a.n_tiles * a.n_chunks;
    const size_t pitch = (size_t)a.n_tiles * CS_TILE_WORDS;
    for (uint64_t wid = wave_id(); wid < total; wid += wave_count()) {
        const uint32_t tile = (uint32_t)(wid % a.n_tiles), chunk = (uint32_t)(wid / a.n_tiles);
        const uint32_t w = tile * CS_TILE_WORDS + lane;
        const bool in_row = w < a.words;
        const uint32_t sm = site_mask(w, a.n_sites);
        const uint32_t r0 = chunk * CS_ROW_CHUNK, r1 = a.n_rows - r0 < CS_ROW_CHUNK ? a.n_rows : r0 + CS_ROW_CHUNK;
        uint32_t pl[4][CS_PLANES];
        if (kCounts) {
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
                for (int p = 0; p < CS_PLANES; ++p) pl[b][p] = 0u;
        }
        uint32_t held[4] = {0u, 0u, 0u, 0u};
        uint32_t cur = kPresence ? (uint32_t)(a.sorted[r0] >> 32) : 0u;          // the label being gathered
        auto flush = [&]() {
            const uint32_t c = cur - 1u;
            uint4 *dst = a.presence + (size_t)c * pitch + w;
            if (a.start[c] >= r0 && a.start[c + 1] <= r1) {                      // all of the cluster lies in this chunk: its only writer
                *dst = make_uint4(held[0], held[1], held[2], held[3]);
            } else {
                uint32_t *d = (uint32_t *)dst;
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (held[b]) atomicOr(d + b, held[b]);
            }
        };
        const uint32_t w_read = in_row ? w : a.words - 1;                        // (a lane past the row reads its last word and masks it away: sm is 0 there)
        for (uint32_t r = r0; r < r1; r += CS_LOADS) {
            // every load is issued before the first is waited for: no branch between them, a row past the chunk reads the chunk's last
            uint4 x[CS_LOADS];
            uint32_t lab[CS_LOADS];
#pragma unroll
            for (int k = 0; k < CS_LOADS; ++k) {
                const uint32_t at = r + k < r1 ? r + k : r1 - 1;
                uint32_t row = at;
                lab[k] = 0u;
                if (kPresence) {
                    const uint64_t key = a.sorted[at];
                    row = (uint32_t)key;
                    lab[k] = (uint32_t)(key >> 32);
                }
                x[k] = a.packed[(size_t)row * a.words + w_read];
            }
            uint32_t m[4][CS_LOADS];                                             // (a row past the chunk holds no base)
#pragma unroll
            for (int k = 0; k < CS_LOADS; ++k) {
                const uint32_t v = r + k < r1 ? x[k].x & sm : 0u, hi = x[k].y, lo = x[k].z;
                m[0][k] = v & ~hi & ~lo;
                m[1][k] = v & ~hi & lo;
                m[2][k] = v & hi & ~lo;
                m[3][k] = v & hi & lo;
                if (kPresence && r + k < r1) {
                    if (lab[k] != cur) {
                        flush();
                        cur = lab[k];
                        held[0] = held[1] = held[2] = held[3] = 0u;
                    }
#pragma unroll
                    for (int b = 0; b < 4; ++b) held[b] |= m[b][k];
                }
            }
            if (kCounts) {
#pragma unroll
                for (int b = 0; b < 4; ++b) planes_add8(pl[b], m[b]);
            }
        }
        if (kPresence) flush();
        if (kCounts && sm) {
            int32_t *dst = a.counts + (size_t)w * 128;                          // [32 sites][4 bases] of this word
            for (uint32_t i = 0; i < 32u && ((sm >> i) & 1u); ++i) {
                uint32_t cnt[4];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    cnt[b] = 0;
#pragma unroll
                    for (int p = 0; p < CS_PLANES; ++p) cnt[b] |= ((pl[b][p] >> i) & 1u) << p;
                }
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (cnt[b]) atomicAdd(dst + i * 4 + b, (int32_t)cnt[b]);
            }
        }
    }
}

// the presence words that k_sweep does not store outright: those of empty clusters and of clusters that straddle a chunk edge
__global__ __launch_bounds__(CS_THREADS) void k_presence_zero(const uint32_t *start, uint32_t n_clusters, uint32_t n_tiles, uint4 *presence) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t total = (uint64_t)n_clusters * n_tiles;
    for (uint64_t wid = wave_id(); wid < total; wid += wave_count()) {
        const uint32_t c = (uint32_t)(wid / n_tiles), tile = (uint32_t)(wid % n_tiles);
        const uint32_t s0 = start[c], s1 = start[c + 1];
        if (s0 == s1 || s0 / CS_ROW_CHUNK != (s1 - 1) / CS_ROW_CHUNK)
            presence[((size_t)c * n_tiles + tile) * CS_TILE_WORDS + lane] = make_uint4(0u, 0u, 0u, 0u);
    }
}

struct OnceTwice { uint4 once, twice; };

__device__ __forceinline__ void hold(OnceTwice &s, const uint4 p) {
    s.twice.x |= s.once.x & p.x; s.twice.y |= s.once.y & p.y; s.twice.z |= s.once.z & p.z; s.twice.w |= s.once.w & p.w;
    s.once.x |= p.x; s.once.y |= p.y; s.once.z |= p.z; s.once.w |= p.w;
}

// part[k][word]: once / twice over the clusters of chunk k
__global__ __launch_bounds__(CS_THREADS) void k_unique_part(const uint4 *presence, uint32_t n_clusters, uint32_t n_tiles, uint32_t n_parts, OnceTwice *part) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t total = (uint64_t)n_parts * n_tiles;
    const size_t pitch = (size_t)n_tiles * CS_TILE_WORDS;
    for (uint64_t wid = wave_id(); wid < total; wid += wave_count()) {
        const uint32_t k = (uint32_t)(wid / n_tiles), w = (uint32_t)(wid % n_tiles) * CS_TILE_WORDS + lane;
        const uint32_t c0 = k * CS_CLUSTER_CHUNK, c1 = n_clusters - c0 < CS_CLUSTER_CHUNK ? n_clusters : c0 + CS_CLUSTER_CHUNK;
        OnceTwice s = {make_uint4(0u, 0u, 0u, 0u), make_uint4(0u, 0u, 0u, 0u)};
        for (uint32_t c = c0; c < c1; ++c) hold(s, presence[(size_t)c * pitch + w]);
        part[(size_t)k * pitch + w] = s;
    }
}

// unique[word] = the bases held by exactly one cluster
__global__ __launch_bounds__(CS_THREADS) void k_unique(const OnceTwice *part, uint32_t n_tiles, uint32_t n_parts, uint4 *unique) {
    const uint32_t lane = threadIdx.x & 63;
    const size_t pitch = (size_t)n_tiles * CS_TILE_WORDS;
    for (uint64_t wid = wave_id(); wid < n_tiles; wid += wave_count()) {
        const uint32_t w = (uint32_t)wid * CS_TILE_WORDS + lane;
        OnceTwice s = {make_uint4(0u, 0u, 0u, 0u), make_uint4(0u, 0u, 0u, 0u)};
        for (uint32_t k = 0; k < n_parts; ++k) {
            const OnceTwice o = part[(size_t)k * pitch + w];
            hold(s, o.once);                                                     // (once, twice) x (once', twice'): twice | twice' | once & once'
            s.twice.x |= o.twice.x; s.twice.y |= o.twice.y; s.twice.z |= o.twice.z; s.twice.w |= o.twice.w;
        }
        unique[w] = make_uint4(s.once.x & ~s.twice.x, s.once.y & ~s.twice.y, s.once.z & ~s.twice.z, s.once.w & ~s.twice.w);
    }
}

// kEmit = false: cnt[c * n_tiles + tile] = entries of cluster c in the tile.  kEmit = true: those entries from off[c * n_tiles + tile] on.
template <bool kEmit>
__global__ __launch_bounds__(CS_THREADS) void k_rows(const uint4 *presence, const uint4 *unique, uint32_t n_clusters, uint32_t n_tiles, uint64_t *cnt, const uint64_t *off,
                                                     const int32_t *counts, uint32_t *site, uint8_t *base, uint32_t *members) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t total = (uint64_t)n_clusters * n_tiles;
    for (uint64_t wid = wave_id(); wid < total; wid += wave_count()) {
        const uint32_t w = (uint32_t)(wid % n_tiles) * CS_TILE_WORDS + lane;
        const uint4 p = presence[wid * CS_TILE_WORDS + lane], u = unique[w];
        const uint32_t ra = p.x & ~(p.y | p.z | p.w) & u.x, rc = p.y & ~(p.x | p.z | p.w) & u.y, rg = p.z & ~(p.x | p.y | p.w) & u.z, rt = p.w & ~(p.x | p.y | p.z) & u.w;
        uint32_t m = ra | rc | rg | rt;
        const uint32_t mine = __popc(m);
        const uint32_t incl = wave_inclusive_sum(mine);
        if (!kEmit) {
            if (lane == 63) cnt[wid] = incl;
            continue;
        }
        uint64_t at = off[wid] + (incl - mine);
        while (m) {
            const uint32_t bit = (uint32_t)__ffs((int)m) - 1u;
            m &= m - 1u;
            const uint32_t b = ((rc >> bit) & 1u) | ((rg >> bit) & 1u) << 1 | ((rt >> bit) & 1u) * 3u;
            const uint32_t s = 32u * w + bit;
            site[at] = s;
            base[at] = (uint8_t)b;
            members[at] = (uint32_t)counts[(size_t)s * 4 + b];
            ++at;
        }
    }
}

// the offsets of the clusters: every n_tiles-th of the cells'
__global__ __launch_bounds__(CS_THREADS) void k_cluster_offsets(const uint64_t *off, uint32_t n_clusters, uint32_t n_tiles, uint64_t *cluster_off) {
    for (uint64_t c = (uint64_t)blockIdx.x * CS_THREADS + threadIdx.x; c <= n_clusters; c += (uint64_t)gridDim.x * CS_THREADS) cluster_off[c] = off[c * n_tiles];
}

inline uint32_t words_of(uint32_t n_sites) { return padded_words(n_sites); }
inline uint32_t tiles_of(uint32_t n_sites) { return (uint32_t)(((uint64_t)n_sites + 32 * CS_TILE_WORDS - 1) / (32 * CS_TILE_WORDS)); }
inline unsigned grid_for(const snpgpu_ctx *ctx, uint64_t waves) {
    const uint64_t b = (waves + CS_WAVES - 1) / CS_WAVES, cap = (uint64_t)ctx->n_cu * CS_GRID_CAP_PER_CU;
    return (unsigned)(b < 1 ? 1 : b < cap ? b : cap);
}
inline unsigned grid_threads(const snpgpu_ctx *ctx, uint64_t items) { return grid_for(ctx, (items + 63) / 64); }
inline size_t up256(size_t x) { return (x + 255) / 256 * 256; }

// count[s][b] over all the rows, enqueued on the context's stream (n_rows and n_sites not 0)
int enqueue_site_counts(snpgpu_ctx *ctx, const void *d_packed, uint32_t n_rows, uint32_t n_sites, int32_t *d_counts) {
    SweepArgs a{};
    a.packed = (const uint4 *)d_packed;
    a.n_rows = n_rows;
    a.n_sites = n_sites;
    a.words = words_of(n_sites);
    a.n_tiles = tiles_of(n_sites);
    a.n_chunks = (n_rows + CS_ROW_CHUNK - 1) / CS_ROW_CHUNK;
    a.counts = d_counts;
    HIP_TRY(ctx, hipMemsetAsync(d_counts, 0, (size_t)n_sites * 16, ctx->stream));
    k_sweep<true, false><<<grid_for(ctx, (uint64_t)a.n_tiles * a.n_chunks), CS_THREADS, 0, ctx->stream>>>(a);
    HIP_TRY(ctx, hipGetLastError());
    return SNPGPU_OK;
}

// One labelling against a packed matrix on the device.  d_counts: the site counts when the caller has them, else null (they are
// then counted in the sweep).  *total comes back on the host; the arrays are written only when 0 < capacity and it fits.  Waits
// for the stream: for the check of the labels, for the count, and before the workspace goes.
int cluster_snps_of_labels(snpgpu_ctx *ctx, const void *d_packed, uint32_t n_rows, uint32_t n_sites, const uint32_t *d_labels, uint32_t n_clusters, const int32_t *d_counts,
                           uint64_t capacity, uint64_t *d_cluster_off, uint32_t *d_site, uint8_t *d_base, uint32_t *d_members, uint64_t *total) {
    *total = 0;
    hipStream_t st = ctx->stream;
    const uint32_t n_tiles = tiles_of(n_sites), n_parts = (n_clusters + CS_CLUSTER_CHUNK - 1) / CS_CLUSTER_CHUNK;
    const size_t pitch = (size_t)n_tiles * CS_TILE_WORDS;
    const uint64_t n_cells = (uint64_t)n_clusters * n_tiles;
    // the workspace, one allocation
    const size_t b_keys = up256((size_t)n_rows * 8), b_start = up256(((size_t)n_clusters + 1) * 4), b_presence = up256((size_t)n_clusters * pitch * 16);
    const size_t b_part = up256((size_t)n_parts * pitch * sizeof(OnceTwice)), b_unique = up256(pitch * 16), b_off = up256((n_cells + 2) * 8);
    const size_t b_aggr = up256(((size_t)prim_gscan_blocks(n_cells) + 2) * 8), b_counts = d_counts ? 0 : up256((size_t)n_sites * 16);
    void *ws = nullptr;
    const hipError_t hm = hipMalloc(&ws, 256 + 3 * b_keys + b_start + b_presence + b_part + b_unique + b_off + b_aggr + b_counts);
    if (hm != hipSuccess) return snpgpu_set_error(ctx, SNPGPU_E_NOMEM, "hipMalloc failed: %s", hipGetErrorString(hm));
    char *b = (char *)ws;
    uint32_t *status = (uint32_t *)b, *flag = status + 1;
    b += 256;
    uint64_t *keys = (uint64_t *)b, *buf_a = (uint64_t *)(b + b_keys), *buf_b = (uint64_t *)(b + 2 * b_keys);
    b += 3 * b_keys;
    uint32_t *start = (uint32_t *)b;
    b += b_start;
    uint4 *presence = (uint4 *)b;
    b += b_presence;
    OnceTwice *part = (OnceTwice *)b;
    b += b_part;
    uint4 *unique = (uint4 *)b;
    b += b_unique;
    uint64_t *off = (uint64_t *)b;
    b += b_off;
    uint64_t *aggr = (uint64_t *)b;
    b += b_aggr;
    int32_t *counts = d_counts ? const_cast<int32_t *>(d_counts) : (int32_t *)b;

    int rc = SNPGPU_OK;
    hipError_t he = hipMemsetAsync(status, 0, 8, st);
    uint32_t bad = 0;
    if (he == hipSuccess && n_rows) {
        k_label_keys<<<grid_threads(ctx, n_rows), CS_THREADS, 0, st>>>(d_labels, n_rows, n_clusters, keys, status);
        he = hipGetLastError();
    }
    if (he == hipSuccess) he = hipMemcpyAsync(&bad, status, 4, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    if (he == hipSuccess && bad) rc = snpgpu_set_error(ctx, SNPGPU_E_ARG, "a label lies outside 1 ... %u", n_clusters);
    uint64_t n_entries = 0;
    if (he == hipSuccess && rc == SNPGPU_OK && n_rows && n_sites && n_clusters) {
        const uint64_t *sorted = prim_sort(st, keys, buf_a, buf_b, n_rows, flag, LessU64());
        k_cluster_starts<<<grid_threads(ctx, (uint64_t)n_clusters + 1), CS_THREADS, 0, st>>>(sorted, n_rows, n_clusters, start);
        k_presence_zero<<<grid_for(ctx, n_cells), CS_THREADS, 0, st>>>(start, n_clusters, n_tiles, presence);
        SweepArgs a{};
        a.packed = (const uint4 *)d_packed;
        a.n_rows = n_rows;
        a.n_sites = n_sites;
        a.words = words_of(n_sites);
        a.n_tiles = n_tiles;
        a.n_chunks = (n_rows + CS_ROW_CHUNK - 1) / CS_ROW_CHUNK;
        a.sorted = sorted;
        a.start = start;
        a.presence = presence;
        a.counts = counts;
        const unsigned grid = grid_for(ctx, (uint64_t)a.n_tiles * a.n_chunks);
        if (d_counts) {
            k_sweep<false, true><<<grid, CS_THREADS, 0, st>>>(a);
        } else {
            he = hipMemsetAsync(counts, 0, (size_t)n_sites * 16, st);
            k_sweep<true, true><<<grid, CS_THREADS, 0, st>>>(a);
        }
        k_unique_part<<<grid_for(ctx, (uint64_t)n_parts * n_tiles), CS_THREADS, 0, st>>>(presence, n_clusters, n_tiles, n_parts, part);
        k_unique<<<grid_for(ctx, n_tiles), CS_THREADS, 0, st>>>(part, n_tiles, n_parts, unique);
        if (he == hipSuccess) he = hipMemsetAsync(off, 0, 8, st);
        k_rows<false><<<grid_for(ctx, n_cells), CS_THREADS, 0, st>>>(presence, unique, n_clusters, n_tiles, off + 1, nullptr, nullptr, nullptr, nullptr, nullptr);
        prim_inclusive_scan(st, off + 1, off + 1, n_cells, aggr, AddU64());
        if (he == hipSuccess) he = hipGetLastError();
        if (he == hipSuccess) he = hipMemcpyAsync(&n_entries, off + n_cells, 8, hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipStreamSynchronize(st);
        if (he == hipSuccess && capacity && n_entries <= capacity) {
            if (!d_cluster_off || (n_entries && (!d_site || !d_base || !d_members))) rc = snpgpu_set_error(ctx, SNPGPU_E_ARG, "null cluster-SNPs output");
            if (rc == SNPGPU_OK) {
                k_cluster_offsets<<<grid_threads(ctx, (uint64_t)n_clusters + 1), CS_THREADS, 0, st>>>(off, n_clusters, n_tiles, d_cluster_off);
                he = hipGetLastError();
            }
            if (rc == SNPGPU_OK && he == hipSuccess && n_entries) {
                k_rows<true><<<grid_for(ctx, n_cells), CS_THREADS, 0, st>>>(presence, unique, n_clusters, n_tiles, nullptr, off, counts, d_site, d_base, d_members);
                he = hipGetLastError();
            }
        }
    } else if (he == hipSuccess && rc == SNPGPU_OK && capacity) {                 // no row, no site or no cluster: no entry
        if (!d_cluster_off) rc = snpgpu_set_error(ctx, SNPGPU_E_ARG, "null cluster-SNPs output");
        else he = hipMemsetAsync(d_cluster_off, 0, ((size_t)n_clusters + 1) * 8, st);
    }
    const hipError_t hs = hipStreamSynchronize(st);                              // the workspace is read until here
    if (he == hipSuccess) he = hs;
    (void)hipFree(ws);
    if (rc != SNPGPU_OK) return rc;
    if (he != hipSuccess) return snpgpu_set_error(ctx, SNPGPU_E_HIP, "cluster SNPs failed: %s", hipGetErrorString(he));
    *total = n_entries;
    return SNPGPU_OK;
}

}  // namespace

extern "C" {

int snpgpu_site_counts_dev(snpgpu_ctx *ctx, const void *d_packed, uint32_t n_rows, uint32_t n_sites, int32_t *d_counts) {
    if (!ctx) return SNPGPU_E_ARG;
    if (n_sites == 0) return SNPGPU_OK;
    if (!d_counts || ((uintptr_t)d_counts & 3)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "the counts are null or not 4-byte aligned");
    if (n_rows && (!d_packed || ((uintptr_t)d_packed & 15))) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "the packed matrix is null or not 16-byte aligned");
    HIP_TRY(ctx, snpgpu_enter(ctx));
    if (n_rows == 0) {
        HIP_TRY(ctx, hipMemsetAsync(d_counts, 0, (size_t)n_sites * 16, ctx->stream));
        return SNPGPU_OK;
    }
    return enqueue_site_counts(ctx, d_packed, n_rows, n_sites, d_counts);
}

int snpgpu_site_counts_host(snpgpu_ctx *ctx, const uint8_t *symbols, uint32_t n_rows, uint32_t n_sites, int32_t *out_counts) {
    if (!ctx) return SNPGPU_E_ARG;
    if (n_sites == 0) return SNPGPU_OK;
    if (!out_counts || (n_rows && !symbols)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null site-counts argument");
    if (n_rows == 0) {
        for (size_t k = 0; k < (size_t)n_sites * 4; ++k) out_counts[k] = 0;
        return SNPGPU_OK;
    }
    HIP_TRY(ctx, snpgpu_enter(ctx));
    DevSymbols dev;                                             // the counts behind the symbols
    int rc = dev.open(ctx, symbols, n_rows, n_sites, 0, nullptr, (size_t)n_sites * 16);
    if (rc == SNPGPU_OK) rc = enqueue_site_counts(ctx, dev.packed(), n_rows, n_sites, (int32_t *)dev.extra());
    if (rc != SNPGPU_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(out_counts, dev.extra(), (size_t)n_sites * 16, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return SNPGPU_OK;
}

int snpgpu_cluster_snps_dev(snpgpu_ctx *ctx, const void *d_packed, uint32_t n_rows, uint32_t n_sites, const uint32_t *d_labels, uint32_t n_clusters, uint64_t capacity,
                            uint64_t *d_cluster_off, uint32_t *d_site, uint8_t *d_base, uint32_t *d_members, uint64_t *out_n) {
    if (!ctx) return SNPGPU_E_ARG;
    if (!out_n) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "bad cluster-SNPs arguments");
    *out_n = 0;
    if (n_rows && (!d_labels || ((uintptr_t)d_labels & 3))) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "the labels are null or not 4-byte aligned");
    if (((uintptr_t)d_packed & 15) || (n_rows && n_sites && !d_packed)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "the packed matrix is null or not 16-byte aligned");
    if (((uintptr_t)d_cluster_off & 7) || (((uintptr_t)d_site | (uintptr_t)d_members) & 3)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "a cluster-SNPs output is not aligned");
    HIP_TRY(ctx, snpgpu_enter(ctx));
    return cluster_snps_of_labels(ctx, d_packed, n_rows, n_sites, d_labels, n_clusters, nullptr, capacity, d_cluster_off, d_site, d_base, d_members, out_n);
}

int snpgpu_cluster_snps(snpgpu_ctx *ctx, const uint8_t *symbols, uint32_t n_rows, uint32_t n_sites, const uint32_t *labels, const uint32_t *n_clusters,
                        uint32_t n_labellings, uint64_t capacity, uint64_t *out_cluster_off, uint32_t *out_site, uint8_t *out_base, uint32_t *out_members,
                        uint64_t *out_n) {
    if (!ctx) return SNPGPU_E_ARG;
    if (!out_n || (n_rows && n_sites && !symbols) || (n_labellings && (!n_clusters || (n_rows && !labels)))) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null cluster-SNPs argument");
    *out_n = 0;
    size_t n_offsets = 0;
    for (uint32_t t = 0; t < n_labellings; ++t) {
        n_offsets += (size_t)n_clusters[t] + 1;
        for (uint32_t i = 0; i < n_rows; ++i) {
            const uint32_t l = labels[(size_t)t * n_rows + i];
            if (l == 0 || l > n_clusters[t]) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "label %u of row %u of labelling %u lies outside 1 ... %u", l, i, t, n_clusters[t]);
        }
    }
    if (n_labellings == 0) return SNPGPU_OK;
    if (capacity && (!out_cluster_off || !out_site || !out_base || !out_members)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null cluster-SNPs output");
    HIP_TRY(ctx, snpgpu_enter(ctx));
    hipStream_t st = ctx->stream;
    DevSymbols dev;
    void *d_lists = nullptr, *d_out = nullptr;
    // labels of one labelling, the site counts (counted once), the offsets of every labelling; the entries when there is room
    const size_t b_labels = up256((size_t)n_rows * 4), b_counts = up256((size_t)n_sites * 16), b_coff = up256(n_offsets * 8);
    const size_t b_site = up256((size_t)capacity * 4);
    hipError_t he = hipMalloc(&d_lists, b_labels + b_counts + b_coff + 256);
    if (he == hipSuccess && capacity) he = hipMalloc(&d_out, 2 * b_site + up256((size_t)capacity) + 256);
    if (he != hipSuccess) {
        (void)hipFree(d_lists);
        return snpgpu_set_error(ctx, SNPGPU_E_NOMEM, "hipMalloc failed: %s", hipGetErrorString(he));
    }
    uint32_t *d_labels = (uint32_t *)d_lists;
    int32_t *d_counts = (int32_t *)((char *)d_lists + b_labels);
    uint64_t *d_coff = (uint64_t *)((char *)d_lists + b_labels + b_counts);
    uint32_t *d_site = (uint32_t *)d_out, *d_members = (uint32_t *)((char *)d_out + b_site);
    uint8_t *d_base = (uint8_t *)d_out + 2 * b_site;
    int rc = dev.open(ctx, symbols, n_rows, n_sites);
    const void *d_packed = dev.packed();
    if (rc == SNPGPU_OK) he = hipMemsetAsync(d_coff, 0, n_offsets * 8, st);      // a labelling without room for an entry has none: its offsets stay 0
    const bool cells = n_rows && n_sites;
    if (rc == SNPGPU_OK && cells) rc = enqueue_site_counts(ctx, d_packed, n_rows, n_sites, d_counts);
    std::vector<uint64_t> first(n_labellings + 1, 0);                            // entries before each labelling
    bool fits = capacity != 0;
    size_t o = 0;
    for (uint32_t t = 0; t < n_labellings && rc == SNPGPU_OK && he == hipSuccess; ++t) {
        if (n_rows) he = hipMemcpyAsync(d_labels, labels + (size_t)t * n_rows, (size_t)n_rows * 4, hipMemcpyHostToDevice, st);
        if (he != hipSuccess) break;
        const uint64_t room = fits ? capacity - first[t] : 0;
        uint64_t got = 0;
        rc = cluster_snps_of_labels(ctx, d_packed, n_rows, n_sites, d_labels, n_clusters[t], cells ? d_counts : nullptr, room, d_coff + o, fits ? d_site + first[t] : nullptr,
                                    fits ? d_base + first[t] : nullptr, fits ? d_members + first[t] : nullptr, &got);
        first[t + 1] = first[t] + got;
        if (got > room) fits = false;
        o += (size_t)n_clusters[t] + 1;
    }
    const uint64_t total = first[n_labellings];
    if (rc == SNPGPU_OK && he == hipSuccess && fits) {
        he = hipMemcpyAsync(out_cluster_off, d_coff, n_offsets * 8, hipMemcpyDeviceToHost, st);
        if (he == hipSuccess && total) he = hipMemcpyAsync(out_site, d_site, total * 4, hipMemcpyDeviceToHost, st);
        if (he == hipSuccess && total) he = hipMemcpyAsync(out_members, d_members, total * 4, hipMemcpyDeviceToHost, st);
        if (he == hipSuccess && total) he = hipMemcpyAsync(out_base, d_base, total, hipMemcpyDeviceToHost, st);
    }
    const hipError_t hs = hipStreamSynchronize(st);
    if (he == hipSuccess) he = hs;
    (void)hipFree(d_lists);
    (void)hipFree(d_out);
    if (rc != SNPGPU_OK) return rc;
    if (he != hipSuccess) return snpgpu_set_error(ctx, SNPGPU_E_HIP, "cluster SNPs failed: %s", hipGetErrorString(he));
    *out_n = total;
    if (fits) {                                                                  // a labelling's offsets count from its own first entry on the device
        o = 0;
        for (uint32_t t = 0; t < n_labellings; ++t)
            for (uint32_t c = 0; c <= n_clusters[t]; ++c) out_cluster_off[o++] += first[t];
    }
    return SNPGPU_OK;
}

}  // extern "C"
