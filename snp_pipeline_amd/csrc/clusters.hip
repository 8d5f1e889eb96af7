// Close pairs and SNP-threshold clusters of the distance step: the N x N matrix of distance.hip thresholded on the device.
//
// Additive: extends what distance.calculate_snp_distances (snppipeline/distance.py:93-106) hands the user — the reference writes
// every ordered pair (distance.py:100-106, itertools.product(ids, ids)) and leaves the filter "Distance <= T" and the grouping of
// samples within so many SNPs of each other to whoever reads the 10^8-row file.  Nothing the reference writes changes.
//
//   a. k_close_rows: the rows [row_lo, row_hi) of the matrix as a CSR of their entries <= T, columns ascending, the diagonal
//      included.  A workgroup per row (grid-stride over the rows): a count pass, an inclusive scan of the row counts (prims.h),
//      then an emit pass that reads the row in steps of 256 x 4 columns — one 16-byte load per lane where the row's alignment
//      allows, up to three scalar columns before and after — and places every match by four wave ballots plus the running sum
//      of the wave totals of the workgroup.  No atomics: the bytes of the result are a function of the matrix alone.  Columns
//      at or beyond n are never read, whatever the row pitch holds there.
//   b. connected components of such a CSR at k thresholds at once: label[t][i] starts as i; a hook kernel (a thread per edge)
//      lowers the larger of the two labels of every edge with d <= t by atomicMin, a jump kernel replaces every label by the
//      root of its chain; both report into a flag word, and the rounds end with the first one that changed nothing.  Labels only
//      ever decrease and stay inside their component, so the fixed point — every label the smallest index of its component —
//      is unique and independent of scheduling (a stale read only delays it).  A last pass numbers the roots in index order.
#include "internal.h"
#include "prims.h"

#define CLUSTERS_THREADS 256
#define CLUSTERS_ROW_GRID_CAP 1024       // workgroups of the row kernels: more rows than this go round their grid-stride loop
#define CLUSTERS_EDGE_GRID_CAP 2048      // workgroups of the edge and label kernels

namespace {

struct AddU64 {
    __device__ uint64_t operator()(const uint64_t &a, const uint64_t &b) const { return a + b; }
};

// kEmit = false: row_cnt[r] = matches of row row_lo + r.  kEmit = true: the matches to col / dist from row_off[r] on.
template <bool kEmit>
__global__ __launch_bounds__(CLUSTERS_THREADS) void k_close_rows(const int32_t *mat, uint64_t stride, uint32_t n, uint32_t row_lo, uint32_t rows,
                                                                 int32_t thr, uint64_t *row_cnt, const uint64_t *row_off, uint32_t *col, int32_t *dist) {
    __shared__ uint32_t wave_sum[2][CLUSTERS_THREADS / 64];
    __shared__ uint32_t red[17];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t below = (1ull << lane) - 1;
    uint32_t parity = 0;
    for (uint32_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const int32_t *row = mat + (uint64_t)(row_lo + r) * stride;
        uint32_t head = (uint32_t)(((16u - (uint32_t)((uintptr_t)row & 15u)) & 15u) >> 2);      // scalar columns up to the 16-byte boundary
        if (head > n) head = n;
        const uint32_t n_vec = (n - head) >> 2, tail = head + n_vec * 4;                         // 16-byte groups, first column behind them
        const uint32_t n_tiles = (n_vec + CLUSTERS_THREADS - 1) / CLUSTERS_THREADS;
        const int4 *body = (const int4 *)(row + head);
        uint64_t run = kEmit ? row_off[r] : 0;
        uint32_t cnt = 0;
        for (uint32_t s = 0; s < n_tiles + 2; ++s) {                // step 0: the head, steps 1 .. n_tiles: the body, the last: the tail
            int32_t v[4] = {0, 0, 0, 0};
            uint32_t c0 = 0, m = 0;                                  // first column of this lane, bit k = column c0 + k matches
            if (s == 0) {
                if (head == 0) continue;
                c0 = tid;
                if (tid < head) { v[0] = row[tid]; m = v[0] <= thr; }
            } else if (s == n_tiles + 1) {
                if (tail == n) continue;
                c0 = tail + tid;
                if (c0 < n) { v[0] = row[c0]; m = v[0] <= thr; }
            } else {
                const uint32_t g = (s - 1) * CLUSTERS_THREADS + tid;
                c0 = head + 4 * g;
                if (g < n_vec) {
                    const int4 x = body[g];
                    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
                    m = (uint32_t)(x.x <= thr) | (uint32_t)(x.y <= thr) << 1 | (uint32_t)(x.z <= thr) << 2 | (uint32_t)(x.w <= thr) << 3;
                }
            }
            if (!kEmit) { cnt += __popc(m); continue; }
            uint32_t before = 0, in_wave = 0;                        // matches of lower lanes, of the whole wave
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint64_t b = __ballot((m >> k) & 1u);
                before += __popcll(b & below);
                in_wave += __popcll(b);
            }
            if (lane == 0) wave_sum[parity][wave] = in_wave;
            __syncthreads();                                         // (the other half of wave_sum is written next: one barrier per step)
            uint32_t lower_waves = 0, all = 0;
#pragma unroll
            for (uint32_t w = 0; w < CLUSTERS_THREADS / 64; ++w) {
                const uint32_t x = wave_sum[parity][w];
                lower_waves += w < wave ? x : 0u;
                all += x;
            }
            parity ^= 1;
            uint64_t p = run + lower_waves + before;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if ((m >> k) & 1u) { col[p] = c0 + k; dist[p] = v[k]; ++p; }
            run += all;
        }
        if (!kEmit) {
            uint32_t total;
            (void)block_exclusive_sum(cnt, red, total);
            if (tid == 0) row_cnt[r] = total;
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(CLUSTERS_THREADS) void k_cc_init(uint32_t *label, uint32_t n, uint32_t k) {
    const uint64_t total = (uint64_t)n * k;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) label[i] = (uint32_t)(i % n);
}

// row_of[e] = the row whose slice of the CSR holds entry e (a wave per row); entries no row owns keep 0xFFFFFFFF
__global__ __launch_bounds__(CLUSTERS_THREADS) void k_cc_rows(const uint64_t *row_off, uint32_t n, uint64_t n_edges, uint32_t *row_of) {
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t r = (uint64_t)blockIdx.x * (CLUSTERS_THREADS / 64) + (threadIdx.x >> 6); r < n; r += (uint64_t)gridDim.x * (CLUSTERS_THREADS / 64)) {
        const uint64_t e0 = row_off[r], e1 = row_off[r + 1] < n_edges ? row_off[r + 1] : n_edges;
        for (uint64_t e = e0 + lane; e < e1; e += 64) row_of[e] = (uint32_t)r;
    }
}

__device__ __forceinline__ uint32_t label_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(CLUSTERS_THREADS) void k_cc_hook(const uint32_t *row_of, const uint32_t *col, const int32_t *dist, uint64_t n_edges,
                                                              const int32_t *thr, uint32_t k, uint32_t *label, uint32_t n, uint32_t *changed) {
    bool any = false;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t u = row_of[e], v = col[e];
        if (u >= n || v >= n || u == v) continue;
        const int32_t d = dist[e];
        for (uint32_t t = 0; t < k; ++t) {
            if (d > thr[t]) continue;
            uint32_t *L = label + (uint64_t)t * n;
            const uint32_t lu = label_load(L + u), lv = label_load(L + v);
            if (lu == lv) continue;
            const uint32_t lo = lu < lv ? lu : lv, hi = lu < lv ? lv : lu;
            atomicMin(L + hi, lo);                                  // the larger label's own node ...
            atomicMin(L + (lu < lv ? v : u), lo);                   // ... and the end of the edge that carried it
            any = true;
        }
    }
    if (__ballot(any) && (threadIdx.x & 63) == 0) *changed = 1u;
}

__global__ __launch_bounds__(CLUSTERS_THREADS) void k_cc_jump(uint32_t *label, uint32_t n, uint32_t k, uint32_t *changed) {
    bool any = false;
    const uint64_t total = (uint64_t)n * k;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t *L = label + i / n * n;
        const uint32_t first = label_load(label + i);
        uint32_t l = first;
        for (;;) {                                                   // labels fall strictly along a chain: it ends at a root
            const uint32_t up = label_load(L + l);
            if (up >= l) break;
            l = up;
        }
        if (l != first) { atomicMin(label + i, l); any = true; }
    }
    if (__ballot(any) && (threadIdx.x & 63) == 0) *changed = 1u;
}

__global__ __launch_bounds__(CLUSTERS_THREADS) void k_cc_roots(const uint32_t *label, uint32_t n, uint32_t *is_root) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) is_root[i] = label[i] == (uint32_t)i;
}

__global__ __launch_bounds__(CLUSTERS_THREADS) void k_cc_number(const uint32_t *label, const uint32_t *rank, uint32_t n, uint32_t *number) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) number[i] = rank[label[i]] + 1;
}

inline unsigned grid_for(uint64_t items, unsigned cap) {
    const uint64_t b = (items + CLUSTERS_THREADS - 1) / CLUSTERS_THREADS;
    return (unsigned)(b < 1 ? 1 : b < cap ? b : cap);
}

// The count pass and the scan into the context's scratch: *d_off = rows + 1 offsets there, *total on the host (waits for the stream).
int close_pairs_count(snpgpu_ctx *ctx, const int32_t *d_matrix, uint32_t n, uint64_t row_stride, uint32_t row_lo, uint32_t row_hi, int32_t threshold,
                      uint64_t **d_off, uint64_t *total) {
    const uint32_t rows = row_hi - row_lo;
    void *ws = nullptr;
    const int rc = snpgpu_scratch(ctx, ((size_t)rows + 1 + prim_gscan_blocks(rows) + 2) * 8, &ws);
    if (rc != SNPGPU_OK) return rc;
    uint64_t *off = (uint64_t *)ws, *aggr = off + rows + 1;
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipMemsetAsync(off, 0, 8, st));
    if (rows) {
        k_close_rows<false><<<rows < CLUSTERS_ROW_GRID_CAP ? rows : CLUSTERS_ROW_GRID_CAP, CLUSTERS_THREADS, 0, st>>>(d_matrix, row_stride, n, row_lo, rows, threshold,
                                                                                                                  off + 1, nullptr, nullptr, nullptr);
        prim_inclusive_scan(st, off + 1, off + 1, (uint64_t)rows, aggr, AddU64());
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipMemcpyAsync(total, off + rows, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    *d_off = off;
    return SNPGPU_OK;
}

int close_pairs_emit(snpgpu_ctx *ctx, const int32_t *d_matrix, uint32_t n, uint64_t row_stride, uint32_t row_lo, uint32_t row_hi, int32_t threshold,
                     const uint64_t *d_off, uint32_t *d_col, int32_t *d_dist) {
    const uint32_t rows = row_hi - row_lo;
    if (!rows) return SNPGPU_OK;
    k_close_rows<true><<<rows < CLUSTERS_ROW_GRID_CAP ? rows : CLUSTERS_ROW_GRID_CAP, CLUSTERS_THREADS, 0, ctx->stream>>>(d_matrix, row_stride, n, row_lo, rows, threshold,
                                                                                                                       nullptr, d_off, d_col, d_dist);
    HIP_TRY(ctx, hipGetLastError());
    return SNPGPU_OK;
}

}  // namespace

int snpgpu_close_pairs_to_host(snpgpu_ctx *ctx, const int32_t *d_matrix, uint32_t n, int32_t threshold, uint64_t capacity, uint64_t *out_row_off, uint32_t *out_col,
                               int32_t *out_dist, uint64_t *out_n) {
    uint64_t *d_off = nullptr, total = 0;
    int rc = close_pairs_count(ctx, d_matrix, n, n, 0, n, threshold, &d_off, &total);
    if (rc != SNPGPU_OK) return rc;
    *out_n = total;
    if (capacity == 0 || total > capacity) return SNPGPU_OK;
    if (!out_row_off || (total && (!out_col || !out_dist))) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null close-pairs output");
    void *d_csr = nullptr;                                          // only the CSR crosses the host link, never the matrix
    if (total) {
        const hipError_t hm = hipMalloc(&d_csr, total * 8);
        if (hm != hipSuccess) return snpgpu_set_error(ctx, SNPGPU_E_NOMEM, "hipMalloc failed: %s", hipGetErrorString(hm));
    }
    uint32_t *d_col = (uint32_t *)d_csr;
    int32_t *d_dist = (int32_t *)d_csr + total;
    hipStream_t st = ctx->stream;
    hipError_t he = hipSuccess;
    rc = close_pairs_emit(ctx, d_matrix, n, n, 0, n, threshold, d_off, d_col, d_dist);
    if (rc == SNPGPU_OK) he = hipMemcpyAsync(out_row_off, d_off, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, st);
    if (rc == SNPGPU_OK && he == hipSuccess && total) he = hipMemcpyAsync(out_col, d_col, total * 4, hipMemcpyDeviceToHost, st);
    if (rc == SNPGPU_OK && he == hipSuccess && total) he = hipMemcpyAsync(out_dist, d_dist, total * 4, hipMemcpyDeviceToHost, st);
    const hipError_t hs = hipStreamSynchronize(st);
    if (he == hipSuccess) he = hs;
    (void)hipFree(d_csr);
    if (he != hipSuccess) return snpgpu_set_error(ctx, SNPGPU_E_HIP, "close pairs failed: %s", hipGetErrorString(he));
    return rc;
}

extern "C" {

int snpgpu_close_pairs_dev(snpgpu_ctx *ctx, const int32_t *d_matrix, uint32_t n, uint64_t row_stride, uint32_t row_lo, uint32_t row_hi, int32_t threshold,
                           uint64_t capacity, uint64_t *d_row_off, uint32_t *d_col, int32_t *d_dist, uint64_t *out_n) {
    if (!ctx) return SNPGPU_E_ARG;
    if (!out_n || row_lo > row_hi || row_hi > n || row_stride < n) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "bad close-pairs arguments");
    if (((uintptr_t)d_matrix & 3) || (row_hi > row_lo && !d_matrix)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "the matrix is null or not 4-byte aligned");
    HIP_TRY(ctx, snpgpu_enter(ctx));
    uint64_t *d_off = nullptr, total = 0;
    const int rc = close_pairs_count(ctx, d_matrix, n, row_stride, row_lo, row_hi, threshold, &d_off, &total);
    if (rc != SNPGPU_OK) return rc;
    *out_n = total;
    if (capacity == 0 || total > capacity) return SNPGPU_OK;
    if (!d_row_off || (total && (!d_col || !d_dist))) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null close-pairs output");
    HIP_TRY(ctx, hipMemcpyAsync(d_row_off, d_off, ((size_t)(row_hi - row_lo) + 1) * 8, hipMemcpyDeviceToDevice, ctx->stream));
    return close_pairs_emit(ctx, d_matrix, n, row_stride, row_lo, row_hi, threshold, d_off, d_col, d_dist);
}

int snpgpu_close_pairs(snpgpu_ctx *ctx, const uint8_t *symbols, uint32_t n_rows, uint32_t n_sites, int32_t threshold, uint64_t capacity,
                       uint64_t *out_row_off, uint32_t *out_col, int32_t *out_dist, uint64_t *out_n, int32_t *out_matrix) {
    if (ctx && !out_n) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null close-pairs argument");
    return snpgpu_distance_outputs(ctx, symbols, n_rows, n_sites, 0, nullptr, nullptr, nullptr, out_matrix, 1, threshold, capacity, out_row_off, out_col, out_dist,
                                   out_n, 0);
}

int snpgpu_clusters_dev(snpgpu_ctx *ctx, uint32_t n, const uint64_t *d_row_off, const uint32_t *d_col, const int32_t *d_dist, uint64_t n_edges,
                        const int32_t *thresholds, uint32_t n_thresholds, uint32_t *d_out_numbers, uint32_t *out_n_clusters) {
    if (!ctx) return SNPGPU_E_ARG;
    const uint32_t k = n_thresholds;
    if (k && (!thresholds || !out_n_clusters)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null clusters argument");
    for (uint32_t t = 0; t < k; ++t) out_n_clusters[t] = 0;
    if (n == 0 || k == 0) return SNPGPU_OK;
    if (!d_row_off || !d_out_numbers || (n_edges && (!d_col || !d_dist))) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null clusters argument");
    HIP_TRY(ctx, snpgpu_enter(ctx));
    hipStream_t st = ctx->stream;
    const size_t w_row_of = (size_t)n_edges, w_label = (size_t)n * k, w_scan = prim_scan_workspace_words(n);
    const size_t words = w_row_of + w_label + 2 * (size_t)n + w_scan + 2 * (size_t)k + 4;
    void *d = nullptr;
    hipError_t he = hipMalloc(&d, words * 4);
    if (he != hipSuccess) return snpgpu_set_error(ctx, SNPGPU_E_NOMEM, "hipMalloc failed: %s", hipGetErrorString(he));
    uint32_t *row_of = (uint32_t *)d, *label = row_of + w_row_of, *is_root = label + w_label, *rank = is_root + n, *scan_ws = rank + n;
    uint32_t *counts = scan_ws + w_scan, *flag = counts + k;
    int32_t *d_thr = (int32_t *)(flag + 4);
    std::vector<uint32_t> h_counts(k, 0);
    uint32_t h_flag = 0;
    auto run = [&]() -> hipError_t {
        hipError_t e = hipMemcpyAsync(d_thr, thresholds, (size_t)k * 4, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return e;
        if (n_edges) {
            if ((e = hipMemsetAsync(row_of, 0xFF, (size_t)n_edges * 4, st)) != hipSuccess) return e;
            k_cc_rows<<<grid_for((uint64_t)n * 64, CLUSTERS_EDGE_GRID_CAP), CLUSTERS_THREADS, 0, st>>>(d_row_off, n, n_edges, row_of);
        }
        k_cc_init<<<grid_for((uint64_t)n * k, CLUSTERS_EDGE_GRID_CAP), CLUSTERS_THREADS, 0, st>>>(label, n, k);
        for (uint64_t round = 0; n_edges; ++round) {                // every round but the last lowers a label: at most n * k rounds, in practice a few
            if ((e = hipMemsetAsync(flag, 0, 16, st)) != hipSuccess) return e;
            k_cc_hook<<<grid_for(n_edges, CLUSTERS_EDGE_GRID_CAP), CLUSTERS_THREADS, 0, st>>>(row_of, d_col, d_dist, n_edges, d_thr, k, label, n, flag);
            k_cc_jump<<<grid_for((uint64_t)n * k, CLUSTERS_EDGE_GRID_CAP), CLUSTERS_THREADS, 0, st>>>(label, n, k, flag);
            if ((e = hipGetLastError()) != hipSuccess) return e;
            if ((e = hipMemcpyAsync(&h_flag, flag, 4, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
            if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
            if (!h_flag) break;
            if (round > (uint64_t)n * k + 1) return hipErrorUnknown;
        }
        for (uint32_t t = 0; t < k; ++t) {
            uint32_t *d_total = nullptr;
            k_cc_roots<<<grid_for(n, CLUSTERS_EDGE_GRID_CAP), CLUSTERS_THREADS, 0, st>>>(label + (size_t)t * n, n, is_root);
            prim_exclusive_scan_u32(st, is_root, rank, n, scan_ws, &d_total);
            k_cc_number<<<grid_for(n, CLUSTERS_EDGE_GRID_CAP), CLUSTERS_THREADS, 0, st>>>(label + (size_t)t * n, rank, n, d_out_numbers + (size_t)t * n);
            if ((e = hipMemcpyAsync(counts + t, d_total, 4, hipMemcpyDeviceToDevice, st)) != hipSuccess) return e;
        }
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(h_counts.data(), counts, (size_t)k * 4, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
        return hipStreamSynchronize(st);
    };
    he = run();
    if (he != hipSuccess) (void)hipStreamSynchronize(st);
    (void)hipFree(d);
    if (he != hipSuccess) return snpgpu_set_error(ctx, SNPGPU_E_HIP, "clusters failed: %s", hipGetErrorString(he));
    for (uint32_t t = 0; t < k; ++t) out_n_clusters[t] = h_counts[t];
    return SNPGPU_OK;
}

int snpgpu_clusters(snpgpu_ctx *ctx, uint32_t n, const uint64_t *row_off, const uint32_t *col, const int32_t *dist, uint64_t n_edges,
                    const int32_t *thresholds, uint32_t n_thresholds, uint32_t *out_numbers, uint32_t *out_n_clusters) {
    if (!ctx) return SNPGPU_E_ARG;
    if (n == 0 || n_thresholds == 0) return snpgpu_clusters_dev(ctx, n, nullptr, nullptr, nullptr, 0, thresholds, n_thresholds, nullptr, out_n_clusters);
    if (!row_off || !out_numbers || (n_edges && (!col || !dist))) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null clusters argument");
    if (row_off[0] != 0 || row_off[n] != n_edges) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "the row offsets do not span the %llu edges", (unsigned long long)n_edges);
    for (uint32_t i = 0; i < n; ++i)
        if (row_off[i] > row_off[i + 1]) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "the row offsets fall at row %u", i);
    HIP_TRY(ctx, snpgpu_enter(ctx));
    hipStream_t st = ctx->stream;
    const size_t b_off = ((size_t)n + 1) * 8, b_edges = (size_t)n_edges * 4, b_out = (size_t)n * n_thresholds * 4;
    void *d = nullptr;
    hipError_t he = hipMalloc(&d, b_off + 2 * b_edges + b_out + 64);
    if (he != hipSuccess) return snpgpu_set_error(ctx, SNPGPU_E_NOMEM, "hipMalloc failed: %s", hipGetErrorString(he));
    char *b = (char *)d;
    uint64_t *d_off = (uint64_t *)b;
    uint32_t *d_col = (uint32_t *)(b + b_off);
    int32_t *d_dist = (int32_t *)(b + b_off + b_edges);
    uint32_t *d_out = (uint32_t *)(b + b_off + 2 * b_edges);
    int rc = SNPGPU_OK;
    he = hipMemcpyAsync(d_off, row_off, b_off, hipMemcpyHostToDevice, st);
    if (he == hipSuccess && n_edges) he = hipMemcpyAsync(d_col, col, b_edges, hipMemcpyHostToDevice, st);
    if (he == hipSuccess && n_edges) he = hipMemcpyAsync(d_dist, dist, b_edges, hipMemcpyHostToDevice, st);
    if (he == hipSuccess) rc = snpgpu_clusters_dev(ctx, n, d_off, d_col, d_dist, n_edges, thresholds, n_thresholds, d_out, out_n_clusters);
    if (he == hipSuccess && rc == SNPGPU_OK) he = hipMemcpyAsync(out_numbers, d_out, b_out, hipMemcpyDeviceToHost, st);
    const hipError_t hs = hipStreamSynchronize(st);
    if (he == hipSuccess) he = hs;
    (void)hipFree(d);
    if (he != hipSuccess) return snpgpu_set_error(ctx, SNPGPU_E_HIP, "clusters failed: %s", hipGetErrorString(he));
    return rc;
}

}  // extern "C"
