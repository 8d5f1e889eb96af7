// The neighbour-joining tree of the distance step: the N x N matrix of distance.hip as the phylogeny Saitou & Nei's method builds
// with the Studier-Keppler criterion, in fixed point.
//
// Additive, like mst.hip and linkage.hip: the reference stops at the two tables (snppipeline/distance.py:93-115).  Those files give
// clusterings and ultrametric trees; this one assumes no molecular clock.  Nothing the reference writes changes.
//
// The statement (include/snpgpu.h has it in full; tests/nj_cases.py restates it in Python).  F = 20; w(i,k) = matrix[i][k] << F,
// signed 64 bits; a node lives in the slot of its smallest sample; r live slots.  While r > 3: R(i) = the sum of w(i,k) over live
// k != i; Q(i,j) = (r-2) w(i,j) - R(i) - R(j); the least (Q, i, j), i < j, is joined: (a, b).  La = floor(((r-2) w(a,b) + R(a) - R(b))
// / (2 (r-2))), Lb = w(a,b) - La; the new node takes slot a, w(a,k) = w(k,a) = floor((w(a,k) + w(b,k) - w(a,b)) / 2), b retires.
// The last three slots are a star.  Every sum is an integer sum: any reduction order gives the same value and the tree is unique.
// Values go negative and are kept as they are.  The floors cost at most 2^-20 SNP per level of the tree.
//
// Not a variant of linkage.hip: the criterion depends on every row sum, so cached row minima are worthless and every live row is
// scanned every round; reciprocal pairs cannot be merged together, so a round is one join and there are n - 3 of them.
//
// The working matrix W is n rows of an even pitch, int64, symmetric.  The row of a slot never moves: it is the row of the slot's
// smallest sample.  The COLUMNS are positions: position p is the p-th stored slot in ascending slot order (slot[p]), live[p] = 0 for
// a retired one, R[p] its row sum, m the stored extent (n at first).  So w(p, q) lies at W[slot[p]][q].
//   k_nj_init     W[i][k] = matrix[i][k] << F (the diagonal 0, whatever the caller's holds), R[i] by a block sum; the largest entry
//                 and "a negative entry" go to two flags (vector atomics).  The host waits for the stream here, once, and refuses.
//   per round, r and m known on the host, nothing waits:
//   k_nj_rows     a workgroup per live row i (grid-stride under NJ_ROW_GRID_CAP) over the columns k > i: a lane loads two columns
//                 at once, 16 bytes of the row and of R and 8 of live[] (rows and R are 16-byte aligned: the pitch is even), the
//                 loads of NJ_UNROLL steps in flight; the least ((r-2) W[i][k] - R[k], k) over the live ones; R[i] is the same for
//                 the whole row and is subtracted once.  (value, k) go together through six shuffle-xor steps and twelve bytes of
//                 LDS per wave across the four waves (two such sets, used in turn: one barrier per row).  Only the upper triangle
//                 is read.  4.3 TB/s over all rounds at 10 000 samples; with 8-byte loads it was 3.3 (profiles/r26/nj.md).  Between
//                 one and eight steps in flight nothing moved by more than 3 %.
//   k_nj_pick     one workgroup of 1024: the least (Q, i, k) over the rows, the three going through shuffles and LDS together; the
//                 record (slot[a], slot[b], La, Lb) straight into the caller's arrays; (a, b, W[a][b]) left for the next kernel,
//                 R[a] = 0, live[b] = 0.
//   k_nj_update   a thread per other live k, ceil(m / 256) workgroups: the new W[a][k] = W[k][a], R[k] += new - W[a][k] - W[b][k];
//                 R[a] += the workgroup's block sum of the new values (a 64-bit vector atomic add: an integer sum, any order gives
//                 the same number); the range flag when a new |w| exceeds L.  It reads rows a and b and writes row and column a: a
//                 thread reads only what it writes itself or what nobody writes.  As the tail of k_nj_pick's one workgroup this
//                 took 18 us a round at 10 000 samples against 5 us here.
//   k_nj_compact  whenever r has fallen to 7/8 of m (the host knows when): an exclusive scan (prims.h) of live[] numbers the live
//                 positions in their order, and a workgroup per live row moves that row's live columns together IN PLACE: a step
//                 reads, waits at a barrier, and writes at or before where it read.  No row moves and no workgroup touches
//                 another's row, so there is no second matrix.  slot, live and R go to their other copies.  The order of the
//                 positions stays the order of the smallest samples, so the tie-break is untouched, and all the rounds together
//                 read 1.07 times the live upper triangles (the sum of r^2 / 2 entries) at 10 000 samples; never moving them
//                 reads 1.5 times, at a half 1.29, at 15/16 1.03 times (profiles/r26/nj.md).
//   k_nj_star     the two or three slots left and their lengths.
// Three launches per round, no cooperative launch, no kernel waits for another workgroup.  One more wait at the end, for the star
// and the range flag.  Memory: the matrix, 8 n^2 bytes, and 48 bytes per sample.
//
// Range: with L = floor(2^61 / n), |w| <= L everywhere keeps every |Q| and every numerator of La below 2^63.  A matrix with a negative
// entry or with (largest entry) << F above L is refused with SNPGPU_E_ARG before the first round.  k_nj_update raises a sticky flag when
// a new |w| exceeds L; it is read once after the last round and makes the call return SNPGPU_E_ARG.  In the Python statement no
// random, tied, planted or additive matrix ever grew beyond its initial largest value (the update is half of a sum of two entries
// less a third), so this flag is a guard that no test reaches on the device.
// Only vector atomics (global_atomic_umax / or in k_nj_init, global_atomic_add_x2 in k_nj_update) and plain stores.
//
// gfx950, hipcc -O3 (-Rpass-analysis=kernel-resource-usage): k_nj_rows 57 VGPRs, 49 SGPRs, 96 bytes of LDS; k_nj_init 42 VGPRs, 50 SGPRs,
// 32 bytes of LDS; k_nj_pick 22 VGPRs, 40 SGPRs, 256 bytes of LDS; k_nj_update 20 VGPRs, 32 bytes of LDS; k_nj_compact 22 VGPRs;
// k_nj_star 10; no spill and no scratch in any of them.
#include <vector>

#include "internal.h"
#include "nj_host.h"
#include "prims.h"

#define NJ_THREADS 256
#define NJ_PICK_THREADS 1024
#define NJ_ROW_GRID_CAP 2048             // workgroups of the per-row kernels: more rows than this go round their grid-stride loops
#ifndef NJ_UNROLL
#define NJ_UNROLL 4                      // steps of a row loop whose loads are in flight together
#endif
#ifndef NJ_COMPACT_NUM                   // the live slots move together when r <= m * NUM / DEN (tools/nj_time.py measures other
#define NJ_COMPACT_NUM 7                 // schedules in libraries built with -DNJ_COMPACT_NUM=..., 0 for never)
#define NJ_COMPACT_DEN 8
#endif

namespace {

typedef long long nj_i64x2 __attribute__((ext_vector_type(2)));
typedef unsigned int nj_u32x2 __attribute__((ext_vector_type(2)));

struct NjResult {                        // what the host reads at the end, and what k_nj_pick leaves for k_nj_update
    int64_t star_len[3];
    int64_t wab;                         // w(a, b) of the round's join
    uint32_t star[3];
    uint32_t out_of_range;
    uint32_t a, b;                       // the positions of the round's join; a = NJ_NONE: none
};

__device__ __forceinline__ int64_t nj_shfl_xor(int64_t v, int m) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)(uint64_t)v, m), hi = (uint32_t)__shfl_xor((int)(uint32_t)((uint64_t)v >> 32), m);
    return (int64_t)((uint64_t)hi << 32 | lo);
}

// the sum of one value per thread over the workgroup, to every thread; lds holds a word per wave; two barriers, so lds can be used
// again right away
__device__ __forceinline__ int64_t nj_block_sum(int64_t v, int64_t *lds) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += nj_shfl_xor(v, m);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    int64_t s = 0;
    for (uint32_t w = 0; w < (blockDim.x >> 6); ++w) s += lds[w];
    __syncthreads();
    return s;
}

__device__ __forceinline__ int64_t nj_floor_div(int64_t x, int64_t d) {          // d > 0
    const int64_t q = x / d;
    return (x % d != 0 && x < 0) ? q - 1 : q;
}

// flags[0]: the largest entry off the diagonal, flags[1]: not 0 when one of them is negative
__global__ __launch_bounds__(NJ_THREADS) void k_nj_init(const int32_t *mat, uint64_t stride, uint32_t n, uint32_t pitch, int64_t *W, int64_t *R, uint32_t *slot,
                                                        uint32_t *live, uint32_t *flags) {
    __shared__ int64_t lds[NJ_THREADS / 64];
    uint32_t most = 0, negative = 0;
    for (uint32_t r = blockIdx.x; r < n; r += gridDim.x) {
        const int32_t *row = mat + (uint64_t)r * stride;
        int64_t *out = W + (uint64_t)r * pitch;
        int64_t sum = 0;
        for (uint32_t k = threadIdx.x; k < n; k += NJ_THREADS) {
            const int32_t v = k == r ? 0 : row[k];                   // (the diagonal is never a distance, whatever it holds)
            if (v < 0) negative = 1;
            else if ((uint32_t)v > most) most = (uint32_t)v;
            const int64_t w = v < 0 ? 0 : (int64_t)v << NJ_FRACTION_BITS;
            out[k] = w;
            sum += w;
        }
        sum = nj_block_sum(sum, lds);
        if (threadIdx.x == 0) { R[r] = sum; slot[r] = r; live[r] = 1; }
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

// per live row i: rk[i] = the live column k > i with the least (Q(i,k), k), rq[i] that Q; rk[i] = NJ_NONE for the last live row
__global__ __launch_bounds__(NJ_THREADS) void k_nj_rows(const int64_t *W, uint32_t pitch, uint32_t m, uint32_t r, const int64_t *R, const uint32_t *live,
                                                        const uint32_t *slot, int64_t *rq, uint32_t *rk) {
    __shared__ int64_t wave_q[2][NJ_THREADS / 64];
    __shared__ uint32_t wave_k[2][NJ_THREADS / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t factor = (int64_t)r - 2;
    uint32_t parity = 0;
    for (uint32_t i = blockIdx.x; i < m; i += gridDim.x) {
        if (!live[i]) continue;                                      // (the same for the whole workgroup)
        const int64_t *row = W + (uint64_t)slot[i] * pitch;
        int64_t best_q = 0;
        uint32_t best_k = NJ_NONE;
        // a lane takes the columns k, k + 1 of an even k: 16 bytes of the row and of R, 8 of live (the pitch is even, so both exist);
        // the loads of NJ_UNROLL steps are issued before the first compare
        for (uint32_t k0 = ((i + 1) & ~1u) + 2 * tid; k0 < m; k0 += NJ_UNROLL * 2 * NJ_THREADS) {
            nj_u32x2 lv[NJ_UNROLL];
            nj_i64x2 w[NJ_UNROLL], rs[NJ_UNROLL];
#pragma unroll
            for (uint32_t u = 0; u < NJ_UNROLL; ++u) {
                const uint32_t k = k0 + u * 2 * NJ_THREADS;
                const bool in = k < m;
                lv[u] = in ? *(const nj_u32x2 *)(live + k) : nj_u32x2{0u, 0u};
                rs[u] = in ? *(const nj_i64x2 *)(R + k) : nj_i64x2{0, 0};
                w[u] = in ? *(const nj_i64x2 *)(row + k) : nj_i64x2{0, 0};
            }
#pragma unroll
            for (uint32_t u = 0; u < NJ_UNROLL; ++u) {               // (ascending k within a thread: the first of equals stays)
                const uint32_t k = k0 + u * 2 * NJ_THREADS;
                const int64_t q0 = factor * w[u].x - rs[u].x, q1 = factor * w[u].y - rs[u].y;
                if (lv[u].x && k > i && k < m && (best_k == NJ_NONE || q0 < best_q)) { best_q = q0; best_k = k; }
                if (lv[u].y && k + 1 < m && (best_k == NJ_NONE || q1 < best_q)) { best_q = q1; best_k = k + 1; }
            }
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            const int64_t oq = nj_shfl_xor(best_q, s);
            const uint32_t ok = (uint32_t)__shfl_xor((int)best_k, s);
            if (ok != NJ_NONE && (best_k == NJ_NONE || oq < best_q || (oq == best_q && ok < best_k))) { best_q = oq; best_k = ok; }
        }
        if (lane == 0) { wave_q[parity][wave] = best_q; wave_k[parity][wave] = best_k; }
        __syncthreads();                                             // (the other half of the LDS is written next: one barrier per row)
        if (tid == 0) {
#pragma unroll
            for (uint32_t v = 1; v < NJ_THREADS / 64; ++v) {
                const int64_t oq = wave_q[parity][v];
                const uint32_t ok = wave_k[parity][v];
                if (ok != NJ_NONE && (best_k == NJ_NONE || oq < best_q || (oq == best_q && ok < best_k))) { best_q = oq; best_k = ok; }
            }
            rq[i] = best_q - R[i];
            rk[i] = best_k;
        }
        parity ^= 1;
    }
}

// the round's join: the least (Q, i, k) of the rows and its record; R[a] is cleared for the sums of k_nj_update and b retires
__global__ __launch_bounds__(NJ_PICK_THREADS) void k_nj_pick(const int64_t *W, uint32_t pitch, uint32_t m, uint32_t r, int64_t *R, uint32_t *live, const uint32_t *slot,
                                                             const int64_t *rq, const uint32_t *rk, uint32_t round, uint32_t *d_a, uint32_t *d_b,
                                                             int64_t *d_len_a, int64_t *d_len_b, NjResult *res) {
    __shared__ int64_t lds_q[NJ_PICK_THREADS / 64];
    __shared__ uint32_t lds_i[NJ_PICK_THREADS / 64], lds_k[NJ_PICK_THREADS / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t best_q = 0;
    uint32_t best_i = NJ_NONE, best_k = NJ_NONE;
    for (uint32_t i = tid; i < m; i += NJ_PICK_THREADS) {            // (ascending i within a thread: the first of equals stays)
        const uint32_t k = rk[i];
        if (!live[i] || k == NJ_NONE) continue;
        const int64_t q = rq[i];
        if (best_i == NJ_NONE || q < best_q) { best_q = q; best_i = i; best_k = k; }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const int64_t oq = nj_shfl_xor(best_q, s);
        const uint32_t oi = (uint32_t)__shfl_xor((int)best_i, s), ok = (uint32_t)__shfl_xor((int)best_k, s);
        if (oi != NJ_NONE && (best_i == NJ_NONE || oq < best_q || (oq == best_q && oi < best_i))) { best_q = oq; best_i = oi; best_k = ok; }
    }
    if (lane == 0) { lds_q[wave] = best_q; lds_i[wave] = best_i; lds_k[wave] = best_k; }
    __syncthreads();                                                 // (every read of live[] lies before this barrier)
    if (tid != 0) return;
    for (uint32_t v = 1; v < NJ_PICK_THREADS / 64; ++v) {
        const int64_t oq = lds_q[v];
        const uint32_t oi = lds_i[v];
        if (oi != NJ_NONE && (best_i == NJ_NONE || oq < best_q || (oq == best_q && oi < best_i))) { best_q = oq; best_i = oi; best_k = lds_k[v]; }
    }
    const uint32_t a = best_i, b = best_k;
    if (a >= m || b >= m || a >= b) { res->a = NJ_NONE; return; }    // (never: r > 3 live rows)
    const int64_t wab = W[(uint64_t)slot[a] * pitch + b], factor = (int64_t)r - 2;
    const int64_t la = nj_floor_div(factor * wab + R[a] - R[b], 2 * factor);
    d_a[round] = slot[a];
    d_b[round] = slot[b];
    d_len_a[round] = la;
    d_len_b[round] = wab - la;
    res->a = a;
    res->b = b;
    res->wab = wab;
    R[a] = 0;
    live[b] = 0;
}

// the new node: a thread per other live position k writes W[a][k] = W[k][a], moves R[k], and the workgroup adds its new values to R[a]
// (an integer sum: any order gives the same number).  It reads rows a and b and writes row and column a: a thread reads only what it
// writes itself or what nobody writes.
__global__ __launch_bounds__(NJ_THREADS) void k_nj_update(int64_t *W, uint32_t pitch, uint32_t m, int64_t *R, const uint32_t *live, const uint32_t *slot,
                                                          int64_t limit, NjResult *res) {
    __shared__ int64_t lds[NJ_THREADS / 64];
    const uint32_t a = res->a, b = res->b, k = blockIdx.x * NJ_THREADS + threadIdx.x;
    if (a >= m || b >= m) return;                                    // (never; the same for the whole grid)
    int64_t fresh = 0;
    if (k < m && k != a && live[k]) {                                // (b has retired)
        int64_t *row_a = W + (uint64_t)slot[a] * pitch;
        const int64_t wa = row_a[k], wb = W[(uint64_t)slot[b] * pitch + k];
        fresh = (wa + wb - res->wab) >> 1;                           // (an arithmetic shift: the floor)
        row_a[k] = fresh;
        W[(uint64_t)slot[k] * pitch + a] = fresh;
        R[k] += fresh - wa - wb;
        if (fresh > limit || fresh < -limit) res->out_of_range = 1;
    }
    const int64_t sum = nj_block_sum(fresh, lds);
    if (threadIdx.x == 0 && sum) atomicAdd((unsigned long long *)(R + a), (unsigned long long)sum);
}

// the live columns of every live row move together, in their order and in place; at[] is the exclusive scan of live[].  A row belongs
// to one workgroup; a step reads its columns, waits, and writes them at or before where they were: behind what earlier steps read,
// before what later steps read.  The small arrays go to their other copies, which no workgroup reads here.
__global__ __launch_bounds__(NJ_THREADS) void k_nj_compact(int64_t *W, uint32_t pitch, uint32_t m, uint32_t r, const uint32_t *at, const uint32_t *live,
                                                           const uint32_t *slot, const int64_t *R, uint32_t *to_live, uint32_t *to_slot, int64_t *to_R) {
    for (uint32_t i = blockIdx.x; i < m; i += gridDim.x) {
        if (!live[i]) continue;                                      // (the same for the whole workgroup)
        const uint32_t p = at[i];
        if (p >= r) continue;                                        // (never: r slots are live)
        int64_t *row = W + (uint64_t)slot[i] * pitch;
        for (uint32_t k0 = 0; k0 < m; k0 += NJ_UNROLL * NJ_THREADS) {
            uint32_t to[NJ_UNROLL];
            int64_t v[NJ_UNROLL];
#pragma unroll
            for (uint32_t u = 0; u < NJ_UNROLL; ++u) {
                const uint32_t k = k0 + u * NJ_THREADS + threadIdx.x;
                const bool keep = k < m && live[k];
                to[u] = keep ? at[k] : NJ_NONE;
                v[u] = keep ? row[k] : 0;
            }
            __syncthreads();
#pragma unroll
            for (uint32_t u = 0; u < NJ_UNROLL; ++u)
                if (to[u] < r) row[to[u]] = v[u];
        }
        if (threadIdx.x == 0) { to_live[p] = 1; to_slot[p] = slot[i]; to_R[p] = R[i]; }
    }
}

// the star of the `left` (2 or 3) live slots; m is below 2 * left + 2 here, one thread reads it
__global__ void k_nj_star(const int64_t *W, uint32_t pitch, uint32_t m, const uint32_t *live, const uint32_t *slot, uint32_t left, NjResult *res) {
    if (blockIdx.x || threadIdx.x) return;
    uint32_t p[3] = {NJ_NONE, NJ_NONE, NJ_NONE}, found = 0;
    for (uint32_t i = 0; i < m && found < left; ++i)
        if (live[i]) p[found++] = i;
    for (uint32_t s = 0; s < 3; ++s) { res->star[s] = s < found ? slot[p[s]] : NJ_NONE; res->star_len[s] = 0; }
    if (found != left) { res->star[0] = res->star[1] = res->star[2] = NJ_NONE; return; }      // (never)
    const int64_t wab = W[(uint64_t)slot[p[0]] * pitch + p[1]];
    if (left == 2) {
        res->star_len[0] = wab >> 1;
        res->star_len[1] = wab - (wab >> 1);
        return;
    }
    const int64_t wac = W[(uint64_t)slot[p[0]] * pitch + p[2]], wbc = W[(uint64_t)slot[p[1]] * pitch + p[2]];
    const int64_t la = (wab + wac - wbc) >> 1;
    res->star_len[0] = la;
    res->star_len[1] = wab - la;
    res->star_len[2] = wac - la;
}

}  // namespace

// The tree of a device matrix: the merges into the DEVICE arrays d_a ... d_len_b (room for n - 3), the star to the host.  n >= 2.
// (Declared in internal.h: csrc/nj_bootstrap.hip runs it once per replicate.)
int nj_run(snpgpu_ctx *ctx, const int32_t *d_matrix, uint32_t n, uint64_t row_stride, uint32_t *d_a, uint32_t *d_b, int64_t *d_len_a, int64_t *d_len_b,
           uint32_t *out_star, int64_t *out_star_len) {
    hipStream_t st = ctx->stream;
    const size_t pitch = ((size_t)n + 1) & ~(size_t)1, w_scan = prim_scan_workspace_words(n);      // an even pitch: every row and R are 16-byte aligned
    // 8-byte arrays first: the matrix, R twice, rq, the result; then live twice (8-byte aligned), slot twice, rk, at, the scan's room, the two flags
    const size_t bytes = ((size_t)n * pitch + pitch * 3) * 8 + sizeof(NjResult) + (pitch * 2 + (size_t)n * 4 + w_scan + 2) * 4;
    void *d = nullptr;
    hipError_t he = hipMalloc(&d, bytes);
    if (he != hipSuccess) return snpgpu_set_error(ctx, SNPGPU_E_NOMEM, "hipMalloc failed: %s", hipGetErrorString(he));
    int64_t *W = (int64_t *)d;
    int64_t *Rm[2] = {W + (size_t)n * pitch, W + (size_t)n * pitch + pitch};
    int64_t *rq = Rm[1] + pitch;
    NjResult *res = (NjResult *)(rq + pitch);
    static_assert(sizeof(NjResult) % 8 == 0, "live[] behind the result is read in pairs");
    uint32_t *livem[2] = {(uint32_t *)(res + 1), (uint32_t *)(res + 1) + pitch};
    uint32_t *slotm[2] = {livem[1] + pitch, livem[1] + pitch + n};
    uint32_t *rk = slotm[1] + n, *at = rk + n, *scan_ws = at + n, *flags = scan_ws + w_scan;
    const int64_t limit = nj_limit(n);
    uint32_t seen[2] = {0, 0};
    NjResult got;
    int refused = 0;
    auto run = [&]() -> hipError_t {
        hipError_t e;
        if ((e = hipMemsetAsync(flags, 0, 8, st)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(res, 0, sizeof(NjResult), st)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(livem[0], 0, pitch * 2 * 4, st)) != hipSuccess) return e;
        k_nj_init<<<n < NJ_ROW_GRID_CAP ? n : NJ_ROW_GRID_CAP, NJ_THREADS, 0, st>>>(d_matrix, row_stride, n, (uint32_t)pitch, W, Rm[0], slotm[0], livem[0], flags);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(seen, flags, 8, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
        if (seen[1]) { refused = 1; return hipSuccess; }
        if (((int64_t)seen[0] << NJ_FRACTION_BITS) > limit) { refused = 2; return hipSuccess; }
        uint32_t m = n, r = n, cur = 0, round = 0;
        for (; r > 3; --r, ++round) {
            if ((uint64_t)r * NJ_COMPACT_DEN <= (uint64_t)m * NJ_COMPACT_NUM) {   // enough of the stored extent is retired: the live slots move together, in their order
                prim_exclusive_scan_u32(st, livem[cur], at, m, scan_ws, nullptr);
                k_nj_compact<<<m < NJ_ROW_GRID_CAP ? m : NJ_ROW_GRID_CAP, NJ_THREADS, 0, st>>>(W, (uint32_t)pitch, m, r, at, livem[cur], slotm[cur], Rm[cur], livem[cur ^ 1],
                                                                                              slotm[cur ^ 1], Rm[cur ^ 1]);
                cur ^= 1;
                m = r;
            }
            k_nj_rows<<<m < NJ_ROW_GRID_CAP ? m : NJ_ROW_GRID_CAP, NJ_THREADS, 0, st>>>(W, (uint32_t)pitch, m, r, Rm[cur], livem[cur], slotm[cur], rq, rk);
            k_nj_pick<<<1, NJ_PICK_THREADS, 0, st>>>(W, (uint32_t)pitch, m, r, Rm[cur], livem[cur], slotm[cur], rq, rk, round, d_a, d_b, d_len_a, d_len_b, res);
            k_nj_update<<<(m + NJ_THREADS - 1) / NJ_THREADS, NJ_THREADS, 0, st>>>(W, (uint32_t)pitch, m, Rm[cur], livem[cur], slotm[cur], limit, res);
        }
        k_nj_star<<<1, 64, 0, st>>>(W, (uint32_t)pitch, m, livem[cur], slotm[cur], r, res);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(&got, res, sizeof(NjResult), hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
        return hipStreamSynchronize(st);
    };
    he = run();
    if (he != hipSuccess) (void)hipStreamSynchronize(st);
    (void)hipFree(d);
    if (he != hipSuccess) return snpgpu_set_error(ctx, SNPGPU_E_HIP, "neighbour joining failed: %s", hipGetErrorString(he));
    if (refused == 1) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "the matrix holds a negative entry");
    if (refused == 2)
        return snpgpu_set_error(ctx, SNPGPU_E_ARG, "the largest entry %u shifted by %d bits exceeds 2^61 / %u: the criterion could leave 64 bits", seen[0],
                                NJ_FRACTION_BITS, n);
    if (got.out_of_range) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "a distance of the rounds grew beyond 2^61 / %u: the criterion could leave 64 bits", n);
    for (int s = 0; s < 3; ++s) { out_star[s] = got.star[s]; out_star_len[s] = got.star_len[s]; }
    return SNPGPU_OK;
}

namespace {

void no_star(uint32_t *star, int64_t *star_len) {
    for (int s = 0; s < 3; ++s) { star[s] = NJ_NONE; star_len[s] = 0; }
}

// nj_run with the merges brought to HOST arrays
int nj_run_to_host(snpgpu_ctx *ctx, const int32_t *d_matrix, uint32_t n, uint64_t row_stride, uint32_t *out_a, uint32_t *out_b, int64_t *out_len_a,
                   int64_t *out_len_b, uint32_t *out_star, int64_t *out_star_len) {
    const size_t k = n > 3 ? n - 3 : 0;
    void *d = nullptr;
    if (k) {
        const hipError_t he = hipMalloc(&d, k * 24);
        if (he != hipSuccess) return snpgpu_set_error(ctx, SNPGPU_E_NOMEM, "hipMalloc failed: %s", hipGetErrorString(he));
    }
    int64_t *d_la = (int64_t *)d, *d_lb = d_la + k;
    uint32_t *d_a = (uint32_t *)(d_lb + k), *d_b = d_a + k;
    int rc = nj_run(ctx, d_matrix, n, row_stride, d_a, d_b, d_la, d_lb, out_star, out_star_len);
    hipError_t he = hipSuccess;
    if (rc == SNPGPU_OK && k) {
        hipStream_t st = ctx->stream;
        he = hipMemcpyAsync(out_len_a, d_la, k * 8, hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipMemcpyAsync(out_len_b, d_lb, k * 8, hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipMemcpyAsync(out_a, d_a, k * 4, hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipMemcpyAsync(out_b, d_b, k * 4, hipMemcpyDeviceToHost, st);
        const hipError_t hs = hipStreamSynchronize(st);
        if (he == hipSuccess) he = hs;
    }
    (void)hipFree(d);
    if (he != hipSuccess) return snpgpu_set_error(ctx, SNPGPU_E_HIP, "neighbour joining failed: %s", hipGetErrorString(he));
    return rc;
}

}  // namespace

extern "C" {

int snpgpu_nj_dev(snpgpu_ctx *ctx, const int32_t *d_matrix, uint32_t n, uint64_t row_stride, uint32_t *d_a, uint32_t *d_b, int64_t *d_len_a, int64_t *d_len_b,
                  uint32_t *out_star, int64_t *out_star_len, uint32_t *out_n_merges) {
    if (!ctx) return SNPGPU_E_ARG;
    if (!out_n_merges || !out_star || !out_star_len || row_stride < n) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "bad neighbour-joining arguments");
    if (((uintptr_t)d_matrix & 3) || (n > 1 && !d_matrix)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "the matrix is null or not 4-byte aligned");
    *out_n_merges = 0;
    no_star(out_star, out_star_len);
    if (n <= 1) return SNPGPU_OK;
    if (n > 3 && (!d_a || !d_b || !d_len_a || !d_len_b)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null neighbour-joining output");
    HIP_TRY(ctx, snpgpu_enter(ctx));
    const int rc = nj_run(ctx, d_matrix, n, row_stride, d_a, d_b, d_len_a, d_len_b, out_star, out_star_len);
    if (rc != SNPGPU_OK) { no_star(out_star, out_star_len); return rc; }
    *out_n_merges = n > 3 ? n - 3 : 0;
    return SNPGPU_OK;
}

int snpgpu_nj_of_matrix(snpgpu_ctx *ctx, const int32_t *matrix, uint32_t n, uint64_t row_stride, uint32_t *out_a, uint32_t *out_b, int64_t *out_len_a,
                        int64_t *out_len_b, uint32_t *out_star, int64_t *out_star_len, uint32_t *out_n_merges) {
    if (!ctx) return SNPGPU_E_ARG;
    if (!out_n_merges || !out_star || !out_star_len || row_stride < n || (n > 1 && !matrix)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "bad neighbour-joining arguments");
    *out_n_merges = 0;
    no_star(out_star, out_star_len);
    if (n <= 1) return SNPGPU_OK;
    if (n > 3 && (!out_a || !out_b || !out_len_a || !out_len_b)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null neighbour-joining output");
    HIP_TRY(ctx, snpgpu_enter(ctx));
    const size_t bytes = ((size_t)(n - 1) * row_stride + n) * 4;      // (the last row ends with its column n - 1)
    void *d = nullptr;
    hipError_t he = hipMalloc(&d, bytes);
    if (he != hipSuccess) return snpgpu_set_error(ctx, SNPGPU_E_NOMEM, "hipMalloc failed: %s", hipGetErrorString(he));
    he = hipMemcpyAsync(d, matrix, bytes, hipMemcpyHostToDevice, ctx->stream);
    int rc = SNPGPU_OK;
    if (he == hipSuccess) rc = nj_run_to_host(ctx, (const int32_t *)d, n, row_stride, out_a, out_b, out_len_a, out_len_b, out_star, out_star_len);
    else (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(d);
    if (he != hipSuccess) return snpgpu_set_error(ctx, SNPGPU_E_HIP, "neighbour joining failed: %s", hipGetErrorString(he));
    if (rc != SNPGPU_OK) { no_star(out_star, out_star_len); return rc; }
    *out_n_merges = n > 3 ? n - 3 : 0;
    return SNPGPU_OK;
}

int snpgpu_nj(snpgpu_ctx *ctx, const uint8_t *symbols, uint32_t n_rows, uint32_t n_sites, uint32_t *out_a, uint32_t *out_b, int64_t *out_len_a, int64_t *out_len_b,
              int32_t *out_matrix, uint32_t *out_star, int64_t *out_star_len, uint32_t *out_n_merges) {
    if (!ctx) return SNPGPU_E_ARG;
    if (!out_n_merges || !out_star || !out_star_len || (n_rows && n_sites && !symbols)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "bad neighbour-joining arguments");
    if (n_rows > 3 && (!out_a || !out_b || !out_len_a || !out_len_b)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null neighbour-joining output");
    *out_n_merges = 0;
    no_star(out_star, out_star_len);
    if (n_rows == 0) return SNPGPU_OK;
    HIP_TRY(ctx, snpgpu_enter(ctx));
    DevSymbols dev;
    int rc = dev.open(ctx, symbols, n_rows, n_sites, DevSymbols::MATRIX, out_matrix);
    if (rc == SNPGPU_OK && n_rows > 1)                                                                            // only the tree crosses the host link
        rc = nj_run_to_host(ctx, dev.matrix(), n_rows, n_rows, out_a, out_b, out_len_a, out_len_b, out_star, out_star_len);
    if (rc != SNPGPU_OK) { no_star(out_star, out_star_len); return rc; }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *out_n_merges = n_rows > 3 ? n_rows - 3 : 0;
    return SNPGPU_OK;
}

}  // extern "C"
