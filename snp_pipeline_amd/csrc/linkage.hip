// Complete- and average-linkage trees of the distance step: the N x N matrix of distance.hip as the tree the greedy
// agglomeration builds.
//
// Additive, like mst.hip: the reference stops at the two tables (snppipeline/distance.py:93-115); single linkage (clusters.hip,
// mst.hip) chains, these two do not.  Nothing the reference writes changes.
//
// The statement: a cluster is a set of samples, its id its smallest sample.  complete: d(A,B) = max d(a,b); average: d(A,B) =
// S(A,B) / (|A| |B|), S the sum of d(a,b) — held as the integer S and the two sizes, never as a float.  Pairs of live clusters
// are totally ordered by (d(A,B), min id, max id); THE tree merges the least pair n - 1 times.  Both linkages are reducible and
// the merged cluster keeps the smaller id, so a reciprocal-nearest-neighbour pair stays one when any other such pair merges:
// merging ALL reciprocal pairs of a round builds the same tree, and that is what the rounds here do.
//
// The working matrix W is n x n uint64, symmetric, slot i = the cluster whose id is i; size[i] = 0 marks a retired slot.
//   k_lnk_init      W[i][k] = matrix[i][k] (the caller's matrix is symmetric, as the distance step's is), size = 1, every row to be
//                   scanned; the largest entry and "a negative entry" go to two flags (vector atomics), read before any round.
//   per round:
//   k_lnk_rows      a workgroup per live row that has to be rescanned (grid-stride): lane loads of 8 consecutive bytes, four
//                   steps in flight, the least (W[i][k] / size[k], k) over the live columns k != i.  |i| cancels within a row,
//                   so two columns compare as W[i][k] size[j] against W[i][j] size[k], in 128 bits (W < 2^64, size < 2^32); at
//                   equal value the smaller k is the smaller (min id, max id).  (value, weight, index) go together through six
//                   shuffle-xor steps, sixteen bytes of LDS per wave across the four waves (two such sets, used in turn: one
//                   barrier per row).  Columns >= n do not exist in W, the diagonal and retired slots are never taken.
//   k_lnk_pairs     partner[i] = j where nn[i] = j and nn[j] = i, flag[i] for i < j.  An exclusive scan (prims.h) of the flags
//                   places the round's merges in slot order behind those of the rounds before: no atomic chooses a position.
//                   The host waits for the stream here, once per round, for the count.
//   k_lnk_emit      the records (a, b, sizeA, sizeB, W[a][b]) and the list of the round's surviving slots.
//   k_lnk_contract  a workgroup per live row, in place.  The row of a surviving slot i (partner j > i) becomes the union: against
//                   a live k it combines W[i][k], W[j][k] and, when k merges in the same round and survives, W[i][k'], W[j][k']
//                   too (sum or max); it reads rows i and j only and writes row i only, and column k of row i is read by the
//                   thread that writes it and by the thread of k', which retires and writes nothing.  The row of a slot r that
//                   does not merge takes, for every merge (i, j) of the round's list, W[r][i] = combine(W[r][i], W[r][j]): its own
//                   row only.  Retiring rows are left alone.  So no workgroup reads what another writes, and afterwards row and
//                   column of every surviving slot hold the union.
//   k_lnk_update    size[i] += size[j], size[j] = 0; a row is rescanned next round iff it merged or its nearest neighbour did
//                   (reducibility: nothing else can change a row's minimum; the result does not depend on this saving).
// The rounds end after n - 1 merges; every round has at least one (the least pair of all is reciprocal), so there are at most
// n - 1 — exactly that many for n identical samples, where the ids break every tie.  Last, the n - 1 records are ordered by
// key on the host (lnk_sort_merges, 128-bit cross-multiplication).
//
// Exactness: every comparison is in integers and 128 bits wide where two 64-bit numbers are multiplied.  S itself must fit 64
// bits: S <= (largest entry) floor(n/2) ceil(n/2); a matrix for which that bound reaches 2^64 is refused with SNPGPU_E_ARG before
// the first round (n beyond 185 000 at entries of 2^31 - 1: such a W would not fit the device either).  So is a negative entry.
// Only vector atomics (global_atomic_umax / or in k_lnk_init) and plain stores.
//
// The row loops of k_lnk_rows and k_lnk_contract issue the loads of four steps before the first compare (LNK_UNROLL): at 10 000
// samples that took the call from 15.6 to 12.8 ms (average) and from 15.2 to 13.3 ms (complete; profiles/r20/linkage.md); eight steps
// gave nothing more.
//
// k_lnk_rows, gfx950, hipcc -O3 (-Rpass-analysis=kernel-resource-usage): 48 VGPRs, 45 SGPRs (average; complete: 30 / 51), no spill,
// no scratch, 128 bytes of LDS (complete: 96, the weights are constant); k_lnk_contract: 37 VGPRs, 66 SGPRs; every other kernel of
// the file at most 18 VGPRs, no spill.
#include <algorithm>
#include <vector>

#include "internal.h"
#include "linkage_host.h"
#include "prims.h"

#define LNK_THREADS 256
#define LNK_ROW_GRID_CAP 2048            // workgroups of the per-row kernels: more rows than this go round their grid-stride loops
#define LNK_NODE_GRID_CAP 2048           // workgroups of the per-slot kernels
#define LNK_UNROLL 4                     // steps of a row loop whose loads are in flight together
#define LNK_NONE 0xFFFFFFFFu

namespace {

struct LnkBest {
    uint64_t s;
    uint32_t w, k;                       // weight (size of column k, 1 for complete linkage) and column; k = LNK_NONE: empty
};

// does x come before y in the order of one row: (s / w, k)
template <int kKind>
__device__ __forceinline__ bool lnk_before(const LnkBest &x, const LnkBest &y) {
    if (y.k == LNK_NONE) return x.k != LNK_NONE;
    if (x.k == LNK_NONE) return false;
    if (kKind == SNPGPU_LINKAGE_AVERAGE) {
        const lnk_u128 l = (lnk_u128)x.s * y.w, r = (lnk_u128)y.s * x.w;
        if (l != r) return l < r;
    } else if (x.s != y.s) {
        return x.s < y.s;
    }
    return x.k < y.k;
}

template <int kKind>
__device__ __forceinline__ uint64_t lnk_combine(uint64_t x, uint64_t y) {
    return kKind == SNPGPU_LINKAGE_AVERAGE ? x + y : (x < y ? y : x);
}

__device__ __forceinline__ LnkBest lnk_shfl_xor(const LnkBest &x, int m) {
    LnkBest o;
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x.s, m), hi = (uint32_t)__shfl_xor((int)(uint32_t)(x.s >> 32), m);
    o.s = (uint64_t)hi << 32 | lo;
    o.w = (uint32_t)__shfl_xor((int)x.w, m);
    o.k = (uint32_t)__shfl_xor((int)x.k, m);
    return o;
}

// flags[0]: the largest entry off the diagonal, flags[1]: not 0 when one of them is negative
__global__ __launch_bounds__(LNK_THREADS) void k_lnk_init(const int32_t *mat, uint64_t stride, uint32_t n, uint64_t *W, uint32_t *size, uint32_t *dirty,
                                                          uint32_t *flags) {
    uint32_t most = 0, negative = 0;
    for (uint32_t r = blockIdx.x; r < n; r += gridDim.x) {
        const int32_t *row = mat + (uint64_t)r * stride;
        uint64_t *out = W + (uint64_t)r * n;
        for (uint32_t k = threadIdx.x; k < n; k += LNK_THREADS) {
            const int32_t v = k == r ? 0 : row[k];                   // (the diagonal is never a distance, whatever it holds)
            if (v < 0) negative = 1;
            else if ((uint32_t)v > most) most = (uint32_t)v;
            out[k] = v < 0 ? 0 : (uint64_t)(uint32_t)v;
        }
        if (threadIdx.x == 0) { size[r] = 1; dirty[r] = 1; }
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)most, m);
        most = o > most ? o : most;
        negative |= (uint32_t)__shfl_xor((int)negative, m);
    }
    if ((threadIdx.x & 63) == 0) {
        if (most) atomicMax(flags, most);
        if (negative) atomicOr(flags + 1, 1u);
    }
}

// nn[i] = the live column k != i with the least (W[i][k] / size[k], k), for the live rows marked dirty
template <int kKind>
__global__ __launch_bounds__(LNK_THREADS) void k_lnk_rows(const uint64_t *W, uint32_t n, const uint32_t *size, const uint32_t *dirty, uint32_t *nn) {
    __shared__ uint64_t wave_s[2][LNK_THREADS / 64];
    __shared__ uint32_t wave_w[2][LNK_THREADS / 64], wave_k[2][LNK_THREADS / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t parity = 0;
    for (uint32_t r = blockIdx.x; r < n; r += gridDim.x) {
        if (size[r] == 0 || !dirty[r]) continue;                     // (the same for the whole workgroup)
        const uint64_t *row = W + (uint64_t)r * n;
        LnkBest best = {0, 0, LNK_NONE};
        for (uint32_t k0 = tid; k0 < n; k0 += LNK_UNROLL * LNK_THREADS) {      // the loads of LNK_UNROLL steps are issued before the first compare
            uint32_t w[LNK_UNROLL];
            uint64_t s[LNK_UNROLL];
#pragma unroll
            for (uint32_t u = 0; u < LNK_UNROLL; ++u) {
                const uint32_t k = k0 + u * LNK_THREADS;
                w[u] = k < n ? size[k] : 0u;
                s[u] = k < n ? row[k] : 0u;
            }
#pragma unroll
            for (uint32_t u = 0; u < LNK_UNROLL; ++u) {
                const uint32_t k = k0 + u * LNK_THREADS;
                if (w[u] == 0 || k == r) continue;
                const LnkBest x = {s[u], kKind == SNPGPU_LINKAGE_AVERAGE ? w[u] : 1u, k};
                if (lnk_before<kKind>(x, best)) best = x;
            }
        }
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) {
            const LnkBest o = lnk_shfl_xor(best, m);
            if (lnk_before<kKind>(o, best)) best = o;
        }
        if (lane == 0) { wave_s[parity][wave] = best.s; wave_w[parity][wave] = best.w; wave_k[parity][wave] = best.k; }
        __syncthreads();                                             // (the other half of the LDS is written next: one barrier per row)
        if (tid == 0) {
#pragma unroll
            for (uint32_t v = 1; v < LNK_THREADS / 64; ++v) {
                const LnkBest o = {wave_s[parity][v], wave_w[parity][v], wave_k[parity][v]};
                if (lnk_before<kKind>(o, best)) best = o;
            }
            nn[r] = best.k;
        }
        parity ^= 1;
    }
}

__global__ __launch_bounds__(LNK_THREADS) void k_lnk_pairs(const uint32_t *nn, const uint32_t *size, uint32_t n, uint32_t *partner, uint32_t *flag) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t p = LNK_NONE;
        if (size[i]) {
            const uint32_t j = nn[i];
            if (j < n && j != (uint32_t)i && size[j] && nn[j] == (uint32_t)i) p = j;
        }
        partner[i] = p;
        flag[i] = p != LNK_NONE && (uint32_t)i < p;
    }
}

__global__ __launch_bounds__(LNK_THREADS) void k_lnk_emit(const uint64_t *W, uint32_t n, const uint32_t *size, const uint32_t *partner, const uint32_t *flag,
                                                          const uint32_t *rank, uint32_t base, uint32_t capacity, LnkMerge *merges, uint32_t *list) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        if (!flag[i]) continue;
        const uint32_t at = rank[i], j = partner[i];
        if (at >= n || (uint64_t)base + at >= capacity || j >= n) continue;     // (never: a tree over n samples has n - 1 joins)
        LnkMerge m;
        m.num = W[i * n + j];
        m.a = (uint32_t)i;
        m.b = j;
        m.sa = size[i];
        m.sb = size[j];
        merges[base + at] = m;
        list[at] = (uint32_t)i;
    }
}

template <int kKind>
__global__ __launch_bounds__(LNK_THREADS) void k_lnk_contract(uint64_t *W, uint32_t n, const uint32_t *size, const uint32_t *partner, const uint32_t *list,
                                                              uint32_t picked) {
    for (uint32_t r = blockIdx.x; r < n; r += gridDim.x) {
        if (size[r] == 0) continue;
        const uint32_t p = partner[r];
        uint64_t *row = W + (uint64_t)r * n;
        if (p == LNK_NONE) {                                         // r stays as it is: its entries against the round's unions
            for (uint32_t m = threadIdx.x; m < picked; m += LNK_THREADS) {
                const uint32_t i = list[m], j = partner[i];
                if (i < n && j < n) row[i] = lnk_combine<kKind>(row[i], row[j]);
            }
        } else if (r < p && p < n) {                                 // r becomes the union with p
            const uint64_t *other = W + (uint64_t)p * n;
            for (uint32_t k0 = threadIdx.x; k0 < n; k0 += LNK_UNROLL * LNK_THREADS) {
                uint32_t w[LNK_UNROLL], q[LNK_UNROLL];
                uint64_t mine[LNK_UNROLL], its[LNK_UNROLL];
#pragma unroll
                for (uint32_t u = 0; u < LNK_UNROLL; ++u) {
                    const uint32_t k = k0 + u * LNK_THREADS;
                    const bool in = k < n;
                    w[u] = in ? size[k] : 0u;
                    q[u] = in ? partner[k] : LNK_NONE;
                    mine[u] = in ? row[k] : 0u;
                    its[u] = in ? other[k] : 0u;
                }
#pragma unroll
                for (uint32_t u = 0; u < LNK_UNROLL; ++u) {
                    const uint32_t k = k0 + u * LNK_THREADS;
                    if (k == r || k == p || w[u] == 0) continue;
                    const uint64_t v = lnk_combine<kKind>(mine[u], its[u]);
                    if (q[u] == LNK_NONE) row[k] = v;
                    else if (k < q[u] && q[u] < n) row[k] = lnk_combine<kKind>(v, lnk_combine<kKind>(row[q[u]], other[q[u]]));
                }
            }
        }
    }
}

__global__ __launch_bounds__(LNK_THREADS) void k_lnk_update(const uint32_t *nn, const uint32_t *partner, uint32_t n, uint32_t *size, uint32_t *dirty) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t p = partner[i];
        if (p == LNK_NONE) {                                         // (nobody writes this slot's size in this launch)
            const uint32_t k = nn[i];
            dirty[i] = size[i] && k < n && partner[k] != LNK_NONE;
            continue;
        }
        dirty[i] = 1;
        if ((uint32_t)i < p && p < n) {                              // the survivor moves both sizes; the retiring slot's thread reads neither
            size[i] += size[p];
            size[p] = 0;
        }
    }
}

inline unsigned grid_for(uint64_t items, unsigned cap) {
    const uint64_t b = (items + LNK_THREADS - 1) / LNK_THREADS;
    return (unsigned)(b < 1 ? 1 : b < cap ? b : cap);
}

// The tree of a device matrix as host records in ascending key order.  n >= 2.
int linkage_run(snpgpu_ctx *ctx, const int32_t *d_matrix, uint32_t n, uint64_t row_stride, int kind, std::vector<LnkMerge> &out, uint32_t *out_rounds) {
    hipStream_t st = ctx->stream;
    const uint32_t capacity = n - 1;
    // 8-byte arrays first: W, the records; then size, dirty, nn, partner, flag, rank, list, the scan's room, the two flags
    const size_t w_scan = prim_scan_workspace_words(n);
    const size_t bytes = (size_t)n * n * 8 + (size_t)capacity * sizeof(LnkMerge) + ((size_t)n * 7 + w_scan + 2) * 4;
    void *d = nullptr;
    hipError_t he = hipMalloc(&d, bytes);
    if (he != hipSuccess) return snpgpu_set_error(ctx, SNPGPU_E_NOMEM, "hipMalloc failed: %s", hipGetErrorString(he));
    uint64_t *W = (uint64_t *)d;
    LnkMerge *merges = (LnkMerge *)(W + (size_t)n * n);
    uint32_t *size = (uint32_t *)(merges + capacity), *dirty = size + n, *nn = dirty + n, *partner = nn + n, *flag = partner + n, *rank = flag + n;
    uint32_t *list = rank + n, *scan_ws = list + n, *flags = scan_ws + w_scan;
    uint32_t n_merges = 0, rounds = 0, seen[2] = {0, 0};
    const unsigned row_grid = n < LNK_ROW_GRID_CAP ? n : LNK_ROW_GRID_CAP, node_grid = grid_for(n, LNK_NODE_GRID_CAP);
    out.assign(capacity, LnkMerge());
    int refused = 0;
    auto run = [&]() -> hipError_t {
        hipError_t e;
        if ((e = hipMemsetAsync(nn, 0xFF, (size_t)n * 4, st)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(flags, 0, 8, st)) != hipSuccess) return e;
        k_lnk_init<<<row_grid, LNK_THREADS, 0, st>>>(d_matrix, row_stride, n, W, size, dirty, flags);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(seen, flags, 8, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
        const lnk_u128 most_sum = (lnk_u128)seen[0] * ((uint64_t)(n / 2) * (n - n / 2));
        if (seen[1]) { refused = 1; return hipSuccess; }
        if (kind == SNPGPU_LINKAGE_AVERAGE && most_sum >> 64) { refused = 2; return hipSuccess; }
        while (n_merges < capacity) {
            if (rounds >= capacity) return hipErrorUnknown;
            if (kind == SNPGPU_LINKAGE_AVERAGE) k_lnk_rows<SNPGPU_LINKAGE_AVERAGE><<<row_grid, LNK_THREADS, 0, st>>>(W, n, size, dirty, nn);
            else k_lnk_rows<SNPGPU_LINKAGE_COMPLETE><<<row_grid, LNK_THREADS, 0, st>>>(W, n, size, dirty, nn);
            k_lnk_pairs<<<node_grid, LNK_THREADS, 0, st>>>(nn, size, n, partner, flag);
            uint32_t *d_total = nullptr, picked = 0;
            prim_exclusive_scan_u32(st, flag, rank, n, scan_ws, &d_total);
            if ((e = hipGetLastError()) != hipSuccess) return e;
            if ((e = hipMemcpyAsync(&picked, d_total, 4, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
            if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
            if (picked == 0 || picked > capacity - n_merges) return hipErrorUnknown;     // (never: the least pair of all is reciprocal)
            k_lnk_emit<<<node_grid, LNK_THREADS, 0, st>>>(W, n, size, partner, flag, rank, n_merges, capacity, merges, list);
            n_merges += picked;
            ++rounds;
            if (n_merges == capacity) break;                          // the root: nothing is left to contract for
            if (kind == SNPGPU_LINKAGE_AVERAGE) k_lnk_contract<SNPGPU_LINKAGE_AVERAGE><<<row_grid, LNK_THREADS, 0, st>>>(W, n, size, partner, list, picked);
            else k_lnk_contract<SNPGPU_LINKAGE_COMPLETE><<<row_grid, LNK_THREADS, 0, st>>>(W, n, size, partner, list, picked);
            k_lnk_update<<<node_grid, LNK_THREADS, 0, st>>>(nn, partner, n, size, dirty);
        }
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(out.data(), merges, (size_t)capacity * sizeof(LnkMerge), hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
        return hipStreamSynchronize(st);
    };
    he = run();
    if (he != hipSuccess) (void)hipStreamSynchronize(st);
    (void)hipFree(d);
    if (he != hipSuccess) return snpgpu_set_error(ctx, SNPGPU_E_HIP, "linkage failed: %s", hipGetErrorString(he));
    if (refused == 1) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "the matrix holds a negative entry");
    if (refused == 2) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "a sum of distances could reach 2^64 (largest entry %u, %u samples)", seen[0], n);
    lnk_sort_merges(kind, out);
    *out_rounds = rounds;
    return SNPGPU_OK;
}

void split_merges(const std::vector<LnkMerge> &m, uint32_t *a, uint32_t *b, uint32_t *sa, uint32_t *sb, uint64_t *num) {
    for (size_t e = 0; e < m.size(); ++e) {
        a[e] = m[e].a;
        b[e] = m[e].b;
        sa[e] = m[e].sa;
        sb[e] = m[e].sb;
        num[e] = m[e].num;
    }
}

bool bad_kind(int kind) { return kind != SNPGPU_LINKAGE_COMPLETE && kind != SNPGPU_LINKAGE_AVERAGE; }

}  // namespace

extern "C" {

int snpgpu_linkage_dev(snpgpu_ctx *ctx, const int32_t *d_matrix, uint32_t n, uint64_t row_stride, int kind, uint32_t *d_a, uint32_t *d_b, uint32_t *d_size_a,
                       uint32_t *d_size_b, uint64_t *d_num, uint32_t *out_n_merges, uint32_t *out_rounds) {
    if (!ctx) return SNPGPU_E_ARG;
    if (!out_n_merges || !out_rounds || row_stride < n || bad_kind(kind)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "bad linkage arguments");
    if (((uintptr_t)d_matrix & 3) || (n > 1 && !d_matrix)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "the matrix is null or not 4-byte aligned");
    *out_n_merges = 0;
    *out_rounds = 0;
    if (n <= 1) return SNPGPU_OK;
    if (!d_a || !d_b || !d_size_a || !d_size_b || !d_num) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null linkage output");
    HIP_TRY(ctx, snpgpu_enter(ctx));
    std::vector<LnkMerge> merges;
    uint32_t rounds = 0;
    const int rc = linkage_run(ctx, d_matrix, n, row_stride, kind, merges, &rounds);
    if (rc != SNPGPU_OK) return rc;
    const size_t m = merges.size();
    std::vector<uint32_t> words(m * 4);
    std::vector<uint64_t> num(m);
    split_merges(merges, words.data(), words.data() + m, words.data() + 2 * m, words.data() + 3 * m, num.data());
    hipStream_t st = ctx->stream;
    uint32_t *const to[4] = {d_a, d_b, d_size_a, d_size_b};
    for (int k = 0; k < 4; ++k) HIP_TRY(ctx, hipMemcpyAsync(to[k], words.data() + k * m, m * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_num, num.data(), m * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    *out_n_merges = (uint32_t)m;
    *out_rounds = rounds;
    return SNPGPU_OK;
}

int snpgpu_linkage_of_matrix(snpgpu_ctx *ctx, const int32_t *matrix, uint32_t n, uint64_t row_stride, int kind, uint32_t *out_a, uint32_t *out_b,
                             uint32_t *out_size_a, uint32_t *out_size_b, uint64_t *out_num, uint32_t *out_n_merges, uint32_t *out_rounds) {
    if (!ctx) return SNPGPU_E_ARG;
    if (!out_n_merges || !out_rounds || row_stride < n || bad_kind(kind) || (n > 1 && !matrix)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "bad linkage arguments");
    *out_n_merges = 0;
    *out_rounds = 0;
    if (n <= 1) return SNPGPU_OK;
    if (!out_a || !out_b || !out_size_a || !out_size_b || !out_num) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null linkage output");
    HIP_TRY(ctx, snpgpu_enter(ctx));
    const size_t bytes = ((size_t)(n - 1) * row_stride + n) * 4;      // (the last row ends with its column n - 1)
    void *d = nullptr;
    hipError_t he = hipMalloc(&d, bytes);
    if (he != hipSuccess) return snpgpu_set_error(ctx, SNPGPU_E_NOMEM, "hipMalloc failed: %s", hipGetErrorString(he));
    he = hipMemcpyAsync(d, matrix, bytes, hipMemcpyHostToDevice, ctx->stream);
    std::vector<LnkMerge> merges;
    int rc = SNPGPU_OK;
    if (he == hipSuccess) rc = linkage_run(ctx, (const int32_t *)d, n, row_stride, kind, merges, out_rounds);
    else (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(d);
    if (he != hipSuccess) return snpgpu_set_error(ctx, SNPGPU_E_HIP, "linkage failed: %s", hipGetErrorString(he));
    if (rc != SNPGPU_OK) return rc;
    split_merges(merges, out_a, out_b, out_size_a, out_size_b, out_num);
    *out_n_merges = (uint32_t)merges.size();
    return SNPGPU_OK;
}

int snpgpu_linkage(snpgpu_ctx *ctx, const uint8_t *symbols, uint32_t n_rows, uint32_t n_sites, int kind, uint32_t *out_a, uint32_t *out_b, uint32_t *out_size_a,
                   uint32_t *out_size_b, uint64_t *out_num, int32_t *out_matrix, uint32_t *out_n_merges, uint32_t *out_rounds) {
    if (!ctx) return SNPGPU_E_ARG;
    if (!out_n_merges || !out_rounds || bad_kind(kind) || (n_rows && n_sites && !symbols)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "bad linkage arguments");
    if (n_rows > 1 && (!out_a || !out_b || !out_size_a || !out_size_b || !out_num)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null linkage output");
    *out_n_merges = 0;
    *out_rounds = 0;
    if (n_rows == 0) return SNPGPU_OK;
    HIP_TRY(ctx, snpgpu_enter(ctx));
    DevSymbols dev;
    int rc = dev.open(ctx, symbols, n_rows, n_sites, DevSymbols::MATRIX, out_matrix);
    std::vector<LnkMerge> merges;
    if (rc == SNPGPU_OK && n_rows > 1) rc = linkage_run(ctx, dev.matrix(), n_rows, n_rows, kind, merges, out_rounds);   // only the tree crosses the host link
    if (rc != SNPGPU_OK) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    split_merges(merges, out_a, out_b, out_size_a, out_size_b, out_num);
    *out_n_merges = (uint32_t)merges.size();
    return SNPGPU_OK;
}

int snpgpu_linkage_cut(int kind, uint32_t n, const uint32_t *a, const uint32_t *b, const uint32_t *size_a, const uint32_t *size_b, const uint64_t *num,
                       uint32_t n_merges, const int32_t *thresholds, uint32_t n_thresholds, uint32_t *out_numbers, uint32_t *out_n_clusters) {
    if ((n_thresholds && !thresholds) || (n && n_thresholds && !out_numbers)) return SNPGPU_E_ARG;
    if (!lnk_merges_ok(n, kind, a, b, size_a, size_b, num, n_merges, false, false)) return SNPGPU_E_ARG;
    lnk_cut(kind, n, a, b, size_a, size_b, num, n_merges, thresholds, n_thresholds, out_numbers, out_n_clusters);
    return SNPGPU_OK;
}

}  // extern "C"
