// Minimum spanning tree of the distance step: the N x N matrix of distance.hip as the tree that links the samples.
//
// Additive: extends what distance.calculate_snp_distances (snppipeline/distance.py:93-106) hands the user.  The reference writes
// every ordered pair and leaves "who is linked to whom, and through which pair" (the minimum spanning tree) and "at which distance
// does each group fall together" (the single-linkage dendrogram, which is the tree's edges read in ascending order) to whoever
// reads the file.  Nothing the reference writes changes.
//
// The statement: edge {i, j}, i < j, weighs d = matrix[i][j]; the edges are totally ordered by (d, i, j); the tree is the one
// Kruskal builds in that order, hence unique.  Boruvka rounds under the same order arrive at it:
//   1. k_mst_rows: a workgroup per row i of [row_lo, row_hi) (grid-stride over the rows) reads the row in steps of 256 x 4
//      columns — one 16-byte load per lane where the row's alignment allows, up to three scalar columns before and after, as
//      k_close_rows — and keeps the least (d, j) among the columns j < n, j != i, whose component differs from i's.  Least (d, j)
//      is least (d, min(i,j), max(i,j)): at equal d a column below i beats every column above it, and among either kind the
//      smallest wins.  Shuffle-xor minimum inside the wave, four words of LDS across the waves, then ONE 64-bit vector atomic
//      min per row into best1[component of i] with the key (d, min(i,j)), and the row's own candidate into cand[i].
//   2. k_mst_cols (only when the range is not every row): a thread per column j outside the band walks 64 band rows (the
//      loads of a wave are 256 consecutive bytes of one row) and gives sample j its candidate the same way (an atomic min into
//      cand[j] per chunk of rows, then k_mst_cols_best: one into best1 per sample): an outside sample sees its edges only in
//      the band's columns, and without it a component would pick an edge that is not its minimum.
//   3. three 32-bit fields do not fit a 64-bit key, so the choice has two stages: best1 = least (d, min) of the component
//      (above), then k_mst_max: best2 = least max among the samples whose candidate carries exactly that (d, min).  A sample's
//      candidate is its least full key, so a tie on (d, min) inside a sample is already settled for the smaller max.
//   4. k_mst_pick: every component root reads its edge and the root across it.  Two components that picked the same edge are the
//      only cycle a total order allows; the smaller root of the two stays a root and the larger one keeps the edge, so the edge is
//      counted once.  Every other root hangs itself under the root across.  An exclusive scan (prims.h) of the keep flags places the
//      round's edges in root order behind those of the rounds before: no atomic chooses a position, the bytes are a function of
//      the matrix.  k_mst_jump halves the pointer chains in place (pointers only ever move to an ancestor, so a stale read delays
//      and never misleads) ceil(log2(components)) + 1 times, the last launch walks what is left to the root.
//   The rounds end with the first that picks nothing (or when n - 1 edges are there); with the candidates of both ends every
//   component merges with at least one other per round, so there are at most ceil(log2 n) of them.  The host waits for the
//   stream once per round (the count).  Last, the at most n - 1 edges are sorted by (d, i, j) with prim_sort.
// The empty slot is all ones: d = 2^31 - 1 maps to 0xFFFFFFFF in the high word, but the low word of a real key is an index < n.
// Distances are signed: the high word is d with its sign bit flipped.  Only vector atomics (global_atomic_umin_x2 / umin) and
// plain stores.
//
// k_mst_rows, gfx950, hipcc -O3 (-Rpass-analysis=kernel-resource-usage): 29 VGPRs, 48 SGPRs, no spill, no scratch, 64 bytes of LDS;
// k_mst_cols: 16 VGPRs, 47 SGPRs, no spill; every other kernel of the file at most 18 VGPRs, no spill.
//
// snpgpu_mst_of_edges (host code): Kruskal in the same order over an edge list — the merge of the forests of several ranks.
#include <algorithm>
#include <numeric>

#include "internal.h"
#include "prims.h"

#define MST_THREADS 256
#define MST_ROW_GRID_CAP 1024            // workgroups of the row kernel: more rows than this go round its grid-stride loop
#define MST_NODE_GRID_CAP 2048           // workgroups of the per-sample kernels
#define MST_COL_ROWS 64                  // band rows a thread of the column kernel walks
#define MST_COL_CHUNK_CAP 1024           // row chunks of the column kernel's grid (more go round a loop)
#define MST_EMPTY 0xFFFFFFFFFFFFFFFFull
#define MST_MAX_ROUNDS 40                // far above ceil(log2 n) for any 32-bit n: only a broken matrix pointer gets here

namespace {

struct MstEdge {
    uint32_t d, u, v;                    // d with the sign bit flipped: unsigned order = signed order
};
struct MstEdgeLess {
    __host__ __device__ bool operator()(const MstEdge &a, const MstEdge &b) const {
        if (a.d != b.d) return a.d < b.d;
        if (a.u != b.u) return a.u < b.u;
        return a.v < b.v;
    }
};

__device__ __forceinline__ uint32_t mst_du(int32_t d) { return (uint32_t)d ^ 0x80000000u; }
__device__ __forceinline__ uint64_t mst_min(uint64_t a, uint64_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint32_t node_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m);
        v = mst_min(v, (uint64_t)hi << 32 | lo);
    }
    return v;
}

__global__ __launch_bounds__(MST_THREADS) void k_mst_init(uint32_t *comp, uint32_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) comp[i] = (uint32_t)i;
}

// cand[i] = least (d, j) of row i over the columns of other components; best1[comp[i]] lowered to (d, min(i, j))
__global__ __launch_bounds__(MST_THREADS) void k_mst_rows(const int32_t *mat, uint64_t stride, uint32_t n, uint32_t row_lo, uint32_t rows,
                                                          const uint32_t *comp, uint64_t *cand, unsigned long long *best1) {
    __shared__ uint64_t wave_best[2][MST_THREADS / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t parity = 0;
    for (uint32_t r = blockIdx.x; r < rows; r += gridDim.x, parity ^= 1) {
        const uint32_t i = row_lo + r, ci = comp[i];
        const int32_t *row = mat + (uint64_t)i * stride;
        uint32_t head = (uint32_t)(((16u - (uint32_t)((uintptr_t)row & 15u)) & 15u) >> 2);      // scalar columns up to the 16-byte boundary
        if (head > n) head = n;
        const uint32_t n_vec = (n - head) >> 2, tail = head + n_vec * 4;                         // 16-byte groups, first column behind them
        const int4 *body = (const int4 *)(row + head);
        uint64_t best = MST_EMPTY;
        auto take = [&](int32_t d, uint32_t j) {
            if (j != i && comp[j] != ci) best = mst_min(best, (uint64_t)mst_du(d) << 32 | j);
        };
        if (tid < head) take(row[tid], tid);
        for (uint32_t g = tid; g < n_vec; g += MST_THREADS) {
            const int4 x = body[g];
            const uint32_t j = head + 4 * g;
            take(x.x, j); take(x.y, j + 1); take(x.z, j + 2); take(x.w, j + 3);
        }
        if (tail + tid < n) take(row[tail + tid], tail + tid);                                   // (at most three columns)
        best = wave_min_u64(best);
        if (lane == 0) wave_best[parity][wave] = best;
        __syncthreads();                                             // (the other half of wave_best is written next: one barrier per row)
        if (tid == 0) {
#pragma unroll
            for (uint32_t w = 1; w < MST_THREADS / 64; ++w) best = mst_min(best, wave_best[parity][w]);
            cand[i] = best;
            if (best != MST_EMPTY) {
                const uint32_t j = (uint32_t)best;
                atomicMin(best1 + ci, (unsigned long long)((best & 0xFFFFFFFF00000000ull) | (j < i ? j : i)));
            }
        }
    }
}

// the samples outside the band: cand[j] lowered by what the band's rows hold in column j (a chunk of rows per workgroup row)
__global__ __launch_bounds__(MST_THREADS) void k_mst_cols(const int32_t *mat, uint64_t stride, uint32_t n, uint32_t row_lo, uint32_t row_hi,
                                                          const uint32_t *comp, unsigned long long *cand) {
    const uint32_t chunks = (row_hi - row_lo + MST_COL_ROWS - 1) / MST_COL_ROWS;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x) {
        if (j >= row_lo && j < row_hi) continue;                     // its own row has seen every column
        const uint32_t cj = comp[j];
        for (uint32_t c = blockIdx.y; c < chunks; c += gridDim.y) {
            const uint32_t i0 = row_lo + c * MST_COL_ROWS, i1 = row_hi - i0 < MST_COL_ROWS ? row_hi : i0 + MST_COL_ROWS;
            uint64_t best = MST_EMPTY;
            for (uint32_t i = i0; i < i1; ++i)
                if (comp[i] != cj) best = mst_min(best, (uint64_t)mst_du(mat[(uint64_t)i * stride + j]) << 32 | i);
            if (best != MST_EMPTY) atomicMin(cand + j, (unsigned long long)best);
        }
    }
}

// ... and, once the chunks are through, best1[comp[j]] lowered to the (d, min) of cand[j]: one atomic per outside sample, as the
// row pass has one per row (the chunks themselves would send rows / 64 times as many to the few slots of the large components)
__global__ __launch_bounds__(MST_THREADS) void k_mst_cols_best(const uint64_t *cand, const uint32_t *comp, uint32_t n, uint32_t row_lo, uint32_t row_hi,
                                                               unsigned long long *best1) {
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x) {
        if (j >= row_lo && j < row_hi) continue;
        const uint64_t best = cand[j];
        if (best == MST_EMPTY) continue;
        const uint32_t i = (uint32_t)best;
        atomicMin(best1 + comp[j], (unsigned long long)((best & 0xFFFFFFFF00000000ull) | (i < (uint32_t)j ? i : (uint32_t)j)));
    }
}

// best2[c] = least max(s, j) among the samples s of c whose candidate carries the component's (d, min)
__global__ __launch_bounds__(MST_THREADS) void k_mst_max(const uint64_t *cand, const uint64_t *best1, const uint32_t *comp, uint32_t n, uint32_t *best2) {
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t k = cand[s];
        if (k == MST_EMPTY) continue;
        const uint32_t j = (uint32_t)k, lo = j < (uint32_t)s ? j : (uint32_t)s, hi = j < (uint32_t)s ? (uint32_t)s : j, c = comp[s];
        if (((k & 0xFFFFFFFF00000000ull) | lo) == best1[c]) atomicMin(best2 + c, hi);
    }
}

// next[s] = where s points after this round (a root: itself, or the root across its edge; any other sample: its root);
// keep[s] = 1 for the roots whose edge enters the forest through them
__global__ __launch_bounds__(MST_THREADS) void k_mst_pick(const uint64_t *best1, const uint32_t *best2, const uint32_t *comp, uint32_t n, uint32_t *next, uint32_t *keep) {
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t c = comp[s];
        uint32_t to = c, k = 0;
        if (c == (uint32_t)s && best1[c] != MST_EMPTY) {
            const uint32_t lo = (uint32_t)best1[c], hi = best2[c];
            if (lo < n && hi < n) {                                  // (always: the key of a real edge)
                const uint32_t clo = comp[lo], other = clo == c ? comp[hi] : clo;
                const bool same_edge = best1[other] == best1[c] && best2[other] == hi;
                if (!(same_edge && c < other)) { to = other; k = 1; }
            }
        }
        next[s] = to;
        keep[s] = k;
    }
}

__global__ __launch_bounds__(MST_THREADS) void k_mst_emit(const uint64_t *best1, const uint32_t *best2, const uint32_t *keep, const uint32_t *rank, uint32_t n,
                                                          uint32_t base, uint32_t capacity, MstEdge *edges) {
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (uint64_t)gridDim.x * blockDim.x) {
        if (!keep[s]) continue;
        const uint64_t at = (uint64_t)base + rank[s];
        if (at >= capacity) continue;                                // (never: a forest over n samples has at most n - 1 edges)
        MstEdge e;
        e.d = (uint32_t)(best1[s] >> 32);
        e.u = (uint32_t)best1[s];
        e.v = best2[s];
        edges[at] = e;
    }
}

// kLast = false: one halving of every pointer chain, in place; kLast = true: walk what is left of the chain, comp[s] = its root
template <bool kLast>
__global__ __launch_bounds__(MST_THREADS) void k_mst_jump(uint32_t *next, uint32_t n, uint32_t *comp) {
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t l = node_load(next + s);
        if (!kLast) {
            const uint32_t up = node_load(next + l);
            if (up != l) __hip_atomic_store(next + s, up, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            continue;
        }
        for (uint32_t step = 0; step < n; ++step) {                  // a pointer leads to an ancestor: the walk ends at the root
            const uint32_t up = node_load(next + l);
            if (up == l) break;
            l = up;
        }
        comp[s] = l;
    }
}

__global__ __launch_bounds__(MST_THREADS) void k_mst_split(const MstEdge *edges, uint32_t n_edges, uint32_t *u, uint32_t *v, int32_t *dist) {
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += (uint64_t)gridDim.x * blockDim.x) {
        const MstEdge x = edges[e];
        u[e] = x.u;
        v[e] = x.v;
        dist[e] = (int32_t)(x.d ^ 0x80000000u);
    }
}

inline unsigned grid_for(uint64_t items, unsigned cap) {
    const uint64_t b = (items + MST_THREADS - 1) / MST_THREADS;
    return (unsigned)(b < 1 ? 1 : b < cap ? b : cap);
}

inline uint32_t ceil_log2(uint64_t x) {
    uint32_t k = 0;
    while (((uint64_t)1 << k) < x) ++k;
    return k;
}

}  // namespace

extern "C" {

int snpgpu_mst_dev(snpgpu_ctx *ctx, const int32_t *d_matrix, uint32_t n, uint64_t row_stride, uint32_t row_lo, uint32_t row_hi, uint32_t *d_u, uint32_t *d_v,
                   int32_t *d_dist, uint32_t *out_n_edges, uint32_t *out_rounds) {
    if (!ctx) return SNPGPU_E_ARG;
    if (!out_n_edges || !out_rounds || row_lo > row_hi || row_hi > n || row_stride < n) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "bad mst arguments");
    if (((uintptr_t)d_matrix & 3) || (row_hi > row_lo && !d_matrix)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "the matrix is null or not 4-byte aligned");
    *out_n_edges = 0;
    *out_rounds = 0;
    if (n <= 1 || row_lo == row_hi) return SNPGPU_OK;
    if (!d_u || !d_v || !d_dist) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null mst output");
    HIP_TRY(ctx, snpgpu_enter(ctx));
    hipStream_t st = ctx->stream;
    const uint32_t rows = row_hi - row_lo, capacity = n - 1;
    const bool whole = rows == n;
    // 8-byte arrays first: cand, best1 | best2 (the three are reset together), then comp, next, keep, rank, the scan's and the sort's room
    const size_t w_scan = prim_scan_workspace_words(n), w_edges = (size_t)capacity * 3;
    const size_t words = (size_t)n * 4 + (size_t)n * 5 + w_scan + 3 * w_edges + 8;
    void *d = nullptr;
    hipError_t he = hipMalloc(&d, words * 4);
    if (he != hipSuccess) return snpgpu_set_error(ctx, SNPGPU_E_NOMEM, "hipMalloc failed: %s", hipGetErrorString(he));
    uint64_t *cand = (uint64_t *)d, *best1 = cand + n;
    uint32_t *best2 = (uint32_t *)(best1 + n), *comp = best2 + n, *next = comp + n, *keep = next + n, *rank = keep + n, *scan_ws = rank + n;
    uint32_t *flag = scan_ws + w_scan;
    MstEdge *edges = (MstEdge *)(flag + 8), *buf_a = edges + capacity, *buf_b = buf_a + capacity;
    uint32_t n_edges = 0, rounds = 0;
    auto run = [&]() -> hipError_t {
        hipError_t e;
        k_mst_init<<<grid_for(n, MST_NODE_GRID_CAP), MST_THREADS, 0, st>>>(comp, n);
        while (n_edges < capacity) {
            if (rounds >= MST_MAX_ROUNDS) return hipErrorUnknown;
            if ((e = hipMemsetAsync(cand, 0xFF, (size_t)n * 20, st)) != hipSuccess) return e;
            k_mst_rows<<<rows < MST_ROW_GRID_CAP ? rows : MST_ROW_GRID_CAP, MST_THREADS, 0, st>>>(d_matrix, row_stride, n, row_lo, rows, comp, cand,
                                                                                                 (unsigned long long *)best1);
            if (!whole) {
                const uint32_t chunks = (rows + MST_COL_ROWS - 1) / MST_COL_ROWS;
                k_mst_cols<<<dim3(grid_for(n, MST_NODE_GRID_CAP), chunks < MST_COL_CHUNK_CAP ? chunks : MST_COL_CHUNK_CAP), MST_THREADS, 0, st>>>(
                    d_matrix, row_stride, n, row_lo, row_hi, comp, (unsigned long long *)cand);
                k_mst_cols_best<<<grid_for(n, MST_NODE_GRID_CAP), MST_THREADS, 0, st>>>(cand, comp, n, row_lo, row_hi, (unsigned long long *)best1);
            }
            k_mst_max<<<grid_for(n, MST_NODE_GRID_CAP), MST_THREADS, 0, st>>>(cand, best1, comp, n, best2);
            k_mst_pick<<<grid_for(n, MST_NODE_GRID_CAP), MST_THREADS, 0, st>>>(best1, best2, comp, n, next, keep);
            uint32_t *d_total = nullptr, picked = 0;
            prim_exclusive_scan_u32(st, keep, rank, n, scan_ws, &d_total);
            if ((e = hipGetLastError()) != hipSuccess) return e;
            if ((e = hipMemcpyAsync(&picked, d_total, 4, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
            if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
            if (picked == 0) break;                                  // no component has a candidate: what is there is the forest
            if (picked > capacity - n_edges) return hipErrorUnknown;
            k_mst_emit<<<grid_for(n, MST_NODE_GRID_CAP), MST_THREADS, 0, st>>>(best1, best2, keep, rank, n, n_edges, capacity, edges);
            const uint32_t halvings = ceil_log2((uint64_t)n - n_edges) + 1;     // a chain is no longer than the components of this round, plus the step onto a root
            for (uint32_t h = 0; h < halvings; ++h) k_mst_jump<false><<<grid_for(n, MST_NODE_GRID_CAP), MST_THREADS, 0, st>>>(next, n, comp);
            k_mst_jump<true><<<grid_for(n, MST_NODE_GRID_CAP), MST_THREADS, 0, st>>>(next, n, comp);
            n_edges += picked;
            ++rounds;
        }
        if (n_edges) {
            MstEdge *sorted = prim_sort(st, edges, buf_a, buf_b, (uint64_t)n_edges, flag, MstEdgeLess());
            k_mst_split<<<grid_for(n_edges, MST_NODE_GRID_CAP), MST_THREADS, 0, st>>>(sorted, n_edges, d_u, d_v, d_dist);
        }
        if ((e = hipGetLastError()) != hipSuccess) return e;
        return hipStreamSynchronize(st);
    };
    he = run();
    if (he != hipSuccess) (void)hipStreamSynchronize(st);
    (void)hipFree(d);
    if (he != hipSuccess) return snpgpu_set_error(ctx, SNPGPU_E_HIP, "mst failed: %s", hipGetErrorString(he));
    *out_n_edges = n_edges;
    *out_rounds = rounds;
    return SNPGPU_OK;
}

// One upload, pack and k_distance for everything the distance step hands out: the tree (want_tree), the close pairs (want_pairs),
// the matrix (out_matrix) — and, with keep_packed, the packed matrix stays in the context for snpgpu_pair_sites_kept.
int snpgpu_distance_outputs(snpgpu_ctx *ctx, const uint8_t *symbols, uint32_t n_rows, uint32_t n_sites, int want_tree, uint32_t *out_u, uint32_t *out_v,
                            int32_t *out_dist, int32_t *out_matrix, int want_pairs, int32_t threshold, uint64_t capacity, uint64_t *out_row_off,
                            uint32_t *out_col, int32_t *out_pair_dist, uint64_t *out_n, int keep_packed) {
    if (!ctx) return SNPGPU_E_ARG;
    if ((n_rows && n_sites && !symbols) || (want_pairs && !out_n)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null mst argument");
    if (want_tree && n_rows > 1 && (!out_u || !out_v || !out_dist)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null mst output");
    HIP_TRY(ctx, snpgpu_enter(ctx));
    if (keep_packed) {
        const int rc_drop = snpgpu_packed_drop(ctx);
        if (rc_drop != SNPGPU_OK) return rc_drop;
    }
    if (want_pairs) *out_n = 0;
    if (n_rows == 0) {
        if (want_pairs && capacity && out_row_off) out_row_off[0] = 0;
        return SNPGPU_OK;
    }
    DevSymbols dev;                                             // the tree's edges behind the matrix
    int rc = dev.open(ctx, symbols, n_rows, n_sites, DevSymbols::MATRIX, out_matrix, (size_t)n_rows * 12);
    if (rc != SNPGPU_OK) return rc;
    hipStream_t st = ctx->stream;
    if (want_tree) {
        uint32_t *d_u = (uint32_t *)dev.extra(), *d_v = d_u + n_rows, n_edges = 0, rounds = 0;
        int32_t *d_dist = (int32_t *)(d_v + n_rows);
        rc = snpgpu_mst_dev(ctx, dev.matrix(), n_rows, n_rows, 0, n_rows, d_u, d_v, d_dist, &n_edges, &rounds);
        if (rc != SNPGPU_OK) return rc;
        if (n_edges != n_rows - 1) return snpgpu_set_error(ctx, SNPGPU_E_HIP, "the tree of %u samples has %u edges", n_rows, n_edges);
        if (n_edges) {                                          // only the tree crosses the host link, never the matrix
            HIP_TRY(ctx, hipMemcpyAsync(out_u, d_u, (size_t)n_edges * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(ctx, hipMemcpyAsync(out_v, d_v, (size_t)n_edges * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(ctx, hipMemcpyAsync(out_dist, d_dist, (size_t)n_edges * 4, hipMemcpyDeviceToHost, st));
        }
    }
    if (want_pairs) {                                           // the close pairs of the same matrix
        rc = snpgpu_close_pairs_to_host(ctx, dev.matrix(), n_rows, threshold, capacity, out_row_off, out_col, out_pair_dist, out_n);
        if (rc != SNPGPU_OK) return rc;
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (keep_packed) {
        ctx->kept_packed = dev.release_packed();
        ctx->kept_rows = n_rows;
        ctx->kept_sites = n_sites;
    }
    return SNPGPU_OK;
}

int snpgpu_mst_close_pairs(snpgpu_ctx *ctx, const uint8_t *symbols, uint32_t n_rows, uint32_t n_sites, uint32_t *out_u, uint32_t *out_v, int32_t *out_dist,
                           int32_t *out_matrix, int want_pairs, int32_t threshold, uint64_t capacity, uint64_t *out_row_off, uint32_t *out_col,
                           int32_t *out_pair_dist, uint64_t *out_n) {
    return snpgpu_distance_outputs(ctx, symbols, n_rows, n_sites, 1, out_u, out_v, out_dist, out_matrix, want_pairs, threshold, capacity, out_row_off, out_col,
                                   out_pair_dist, out_n, 0);
}

int snpgpu_mst(snpgpu_ctx *ctx, const uint8_t *symbols, uint32_t n_rows, uint32_t n_sites, uint32_t *out_u, uint32_t *out_v, int32_t *out_dist,
               int32_t *out_matrix) {
    return snpgpu_mst_close_pairs(ctx, symbols, n_rows, n_sites, out_u, out_v, out_dist, out_matrix, 0, 0, 0, nullptr, nullptr, nullptr, nullptr);
}

int snpgpu_mst_of_edges(uint32_t n, const uint32_t *u, const uint32_t *v, const int32_t *dist, uint64_t n_edges, uint32_t *out_u, uint32_t *out_v,
                        int32_t *out_dist, uint32_t *out_n) {
    if (!out_n || (n_edges && (!u || !v || !dist))) return SNPGPU_E_ARG;
    *out_n = 0;
    for (uint64_t e = 0; e < n_edges; ++e)
        if (u[e] >= n || v[e] >= n || u[e] == v[e]) return SNPGPU_E_ARG;
    std::vector<uint64_t> order(n_edges);
    std::iota(order.begin(), order.end(), (uint64_t)0);
    auto lo = [&](uint64_t e) { return u[e] < v[e] ? u[e] : v[e]; };
    auto hi = [&](uint64_t e) { return u[e] < v[e] ? v[e] : u[e]; };
    std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) {
        if (dist[a] != dist[b]) return dist[a] < dist[b];
        if (lo(a) != lo(b)) return lo(a) < lo(b);
        return hi(a) < hi(b);
    });
    std::vector<uint32_t> parent(n);
    std::iota(parent.begin(), parent.end(), 0u);
    auto find = [&](uint32_t x) {
        while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
        return x;
    };
    uint32_t kept = 0;
    for (uint64_t k = 0; k < n_edges && kept + 1 < n; ++k) {
        const uint64_t e = order[k];
        const uint32_t a = find(u[e]), b = find(v[e]);
        if (a == b) continue;
        if (!out_u || !out_v || !out_dist) return SNPGPU_E_ARG;
        parent[a < b ? b : a] = a < b ? a : b;
        out_u[kept] = lo(e);
        out_v[kept] = hi(e);
        out_dist[kept] = dist[e];
        ++kept;
    }
    *out_n = kept;
    return SNPGPU_OK;
}

}  // extern "C"
