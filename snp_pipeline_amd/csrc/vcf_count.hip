// The SNP count of a VCF file (collect_metrics.py:61-106 through PyVCF) as a streamed text kernel.
//
// The file arrives in the staging chunks of stream.hip; every chunk is a launch of its own over a device buffer that holds
// the chunk behind the last SNPGPU_VCF_LOOK bytes of the chunk before it.  A line belongs to the block (and to the launch) in
// whose bytes its TERMINATOR lies: the block keeps its SNPGPU_VCF_TILE bytes and the SNPGPU_VCF_LOOK bytes in front of them in
// LDS, every lane looks for line ends in its 64 bytes, and the lane that finds one walks back to the start of the line and
// evaluates the row there.  So a row that straddles a tile or a chunk edge is counted once, by whoever sees its end, and no
// state is carried between blocks or launches.  A line whose start is not inside the window (SNPGPU_VCF_LOOK - 1 bytes or
// more) goes to the unusual list, as does every data line outside the grammar below; the host evaluates those.
//
// The rule per data line (not empty, does not start with '#'; a CR before the terminator is not part of the line):
//   ten TAB-separated columns; FORMAT (9) and the sample (10) split on ':' into the same number of fields, one of them GT;
//   every allele of GT (split on '/' or '|') is '.' or a decimal index into [REF] + ALT.split(',')      -- else: unusual
//   an allele '.'                                  -> not counted
//   every allele 0                                 -> not counted
//   no named allele is one of the letters A C G T N -> not counted   (a spanning deletion '*')
//   an FT field that is not exactly PASS           -> not counted
//   otherwise one SNP.
#include "internal.h"

namespace {

constexpr uint32_t VC_TILE = SNPGPU_VCF_TILE, VC_LOOK = SNPGPU_VCF_LOOK, VC_THREADS = 256, VC_LANE_BYTES = VC_TILE / VC_THREADS;
static_assert(VC_LANE_BYTES == 64 && VC_LOOK % 16 == 0, "a lane scans four 16-byte words");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool is_acgtn(uint32_t c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T' || c == 'N'; }

// The row in lds[s, e): 0 = not counted, 1 = one SNP, 2 = outside the grammar.
__device__ uint32_t vc_row(const uint8_t *lds, uint32_t s, uint32_t e) {
    uint32_t col = 0, col_s = s;
    uint32_t ref_s = 0, ref_e = 0, alt_s = 0, alt_e = 0, fmt_s = 0, fmt_e = 0, smp_s = 0;
    for (uint32_t i = s; i < e; ++i) {
        if (lds[i] != '\t') continue;
        if (col == 3) { ref_s = col_s; ref_e = i; }
        else if (col == 4) { alt_s = col_s; alt_e = i; }
        else if (col == 8) { fmt_s = col_s; fmt_e = i; }
        ++col;
        col_s = i + 1;
    }
    if (col != 9) return 2;
    smp_s = col_s;
    const uint32_t smp_e = e;
    // FORMAT: the places of GT and FT
    int gt_at = -1, ft_at = -1;
    uint32_t n_fmt = 0;
    for (uint32_t i = fmt_s, f_s = fmt_s; i <= fmt_e; ++i) {
        if (i < fmt_e && lds[i] != ':') continue;
        if (i - f_s == 2 && lds[f_s + 1] == 'T') {
            if (lds[f_s] == 'G' && gt_at < 0) gt_at = (int)n_fmt;
            if (lds[f_s] == 'F' && ft_at < 0) ft_at = (int)n_fmt;
        }
        ++n_fmt;
        f_s = i + 1;
    }
    // the sample column: the same number of fields, and where those two are
    uint32_t n_smp = 0, gt_s = 0, gt_e = 0, ft_s = 0, ft_e = 0;
    for (uint32_t i = smp_s, f_s = smp_s; i <= smp_e; ++i) {
        if (i < smp_e && lds[i] != ':') continue;
        if ((int)n_smp == gt_at) { gt_s = f_s; gt_e = i; }
        if ((int)n_smp == ft_at) { ft_s = f_s; ft_e = i; }
        ++n_smp;
        f_s = i + 1;
    }
    if (n_smp != n_fmt || gt_at < 0) return 2;
    uint32_t n_alt = 1;
    for (uint32_t i = alt_s; i < alt_e; ++i) n_alt += lds[i] == ',';
    bool any_dot = false, any_nonzero = false, any_letter = false;
    for (uint32_t i = gt_s, a_s = gt_s; i <= gt_e; ++i) {
        if (i < gt_e && lds[i] != '/' && lds[i] != '|') continue;
        if (i - a_s == 1 && lds[a_s] == '.') any_dot = true;
        else {
            if (i == a_s) return 2;
            uint32_t v = 0;
            for (uint32_t k = a_s; k < i; ++k) {
                if (!is_digit(lds[k])) return 2;
                v = v > 100000u ? v : v * 10 + (lds[k] - 48u);
            }
            if (v > n_alt) return 2;
            any_nonzero |= v != 0;
            uint32_t b_s = ref_s, b_e = ref_e;
            if (v) {                                            // the v-th entry of ALT
                b_s = alt_s;
                for (uint32_t left = v - 1; left; ++b_s) left -= lds[b_s] == ',';
                for (b_e = b_s; b_e < alt_e && lds[b_e] != ','; ++b_e) { }
            }
            any_letter |= b_e - b_s == 1 && is_acgtn(lds[b_s]);
        }
        a_s = i + 1;
    }
    if (any_dot || !any_nonzero || !any_letter) return 0;
    if (ft_at >= 0 && !(ft_e - ft_s == 4 && lds[ft_s] == 'P' && lds[ft_s + 1] == 'A' && lds[ft_s + 2] == 'S' && lds[ft_s + 3] == 'S')) return 0;
    return 1;
}

// buf[0, n): a piece of the file that starts at file offset file_off (a line start when file_off == 0); this launch owns the
// terminators at [own_from, n).  res: [0] SNPs [1] data lines [2] unusual lines, then `capacity` offsets of unusual lines (the
// offset of the line's first byte; of its terminator, with bit 63 set, when the line is longer than the window).
__global__ void __launch_bounds__(VC_THREADS) vcf_count_kernel(const uint8_t *__restrict__ buf, uint32_t n, uint32_t own_from, uint64_t file_off,
                                                                unsigned long long *__restrict__ res, uint32_t capacity) {
    __shared__ u32x4 tile4[(VC_LOOK + VC_TILE) / 16];
    const uint32_t t0 = own_from + blockIdx.x * VC_TILE;         // (the host launches only blocks with t0 < n)
    const uint32_t t1 = n - t0 < VC_TILE ? n : t0 + VC_TILE;
    const uint32_t l0 = t0 >= VC_LOOK ? t0 - VC_LOOK : 0;        // 16-byte aligned: own_from is 0 or VC_LOOK
    for (uint32_t i = threadIdx.x; i < (VC_LOOK + VC_TILE) / 16; i += VC_THREADS)
        if (l0 + i * 16 < t1) tile4[i] = __builtin_nontemporal_load((const u32x4 *)(buf + l0) + i);   // (the buffer is padded to whole words)
    __syncthreads();
    const uint8_t *lds = (const uint8_t *)tile4;                 // lds[i] is buf[l0 + i]
    uint32_t n_snps = 0, n_data = 0;
    const uint32_t lane0 = t0 + threadIdx.x * VC_LANE_BYTES;
    for (uint32_t w = 0; w < VC_LANE_BYTES / 16 && lane0 + w * 16 < t1; ++w) {
        const u32x4 v = tile4[(lane0 + w * 16 - l0) / 16];
        const uint32_t words[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t k = 0; k < 16; ++k) {
            if (((words[k / 4] >> (8 * (k % 4))) & 0xFF) != '\n') continue;
            const uint32_t p = lane0 + w * 16 + k;               // a terminator of this lane
            if (p >= t1) continue;
            const uint32_t lim = p >= VC_LOOK ? p - VC_LOOK + 1 : 0;
            uint32_t s = p;
            while (s > lim && lds[s - 1 - l0] != '\n') --s;
            const bool found = s == 0 ? file_off == 0 : lds[s - 1 - l0] == '\n';
            uint32_t e = p;
            if (e > s && lds[e - 1 - l0] == '\r') --e;
            uint64_t where = file_off + s;
            uint32_t kind = 2;
            if (!found) where = (file_off + p) | (1ull << 63);
            else if (e == s || lds[s - l0] == '#') continue;
            else kind = vc_row(lds, s - l0, e - l0);
            ++n_data;
            n_snps += kind == 1;
            if (kind == 2) {                                     // (rare: an atomic of its own)
                const unsigned long long at = atomicAdd(&res[2], 1ull);
                if (at < capacity) res[3 + at] = where;
            }
        }
    }
    // per wave: two sums, one atomic instruction (lanes 0 and 1 add one counter each)
    for (uint32_t d = 32; d; d >>= 1) {
        n_snps += __shfl_xor(n_snps, d);
        n_data += __shfl_xor(n_data, d);
    }
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t mine = lane == 0 ? n_snps : n_data;
    if (lane < 2 && mine) atomicAdd(&res[lane], (unsigned long long)mine);
}

}  // namespace

int snpgpu_enqueue_vcf_count(snpgpu_ctx *ctx, const uint8_t *d_buf, uint32_t n, uint32_t own_from, uint64_t file_off, uint64_t *d_res, uint32_t capacity) {
    if (((uintptr_t)d_buf & 15) || (own_from != 0 && own_from != VC_LOOK) || (own_from == 0) != (file_off == 0))
        return snpgpu_set_error(ctx, SNPGPU_E_ARG, "vcf count: a piece starts on a 16-byte boundary, with the look-back of the piece before it or at the start of the file");
    if (n <= own_from) return SNPGPU_OK;
    const uint32_t blocks = (n - own_from + VC_TILE - 1) / VC_TILE;
    hipEvent_t ta = snpgpu_time_begin(ctx);
    hipLaunchKernelGGL(vcf_count_kernel, dim3(blocks), dim3(VC_THREADS), 0, ctx->stream, d_buf, n, own_from, file_off, (unsigned long long *)d_res, capacity);
    snpgpu_time_end(ctx, SNPGPU_K_VCF_COUNT, ta);
    HIP_TRY(ctx, hipGetLastError());
    return SNPGPU_OK;
}
