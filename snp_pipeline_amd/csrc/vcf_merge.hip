// merge_vcfs on the device: the multi-sample snpma.vcf from the per-sample consensus.vcf files (merge_vcfs.py:96-139 of the
// reference, which hands the work to bgzip, tabix and `bcftools merge --merge all --info-rules NS:sum`).
//
// Three kernels; stream.hip drives them (snpgpu_merge_vcf_files):
//   parse   every data line of the streamed text that is inside the grammar below becomes one snpgpu_merge_cell.  As in
//           vcf_count.hip a line belongs to the block (and the launch) in whose bytes its TERMINATOR lies, so tile and chunk
//           edges carry no state.  A line outside the grammar, or one whose start is outside the window, is reported by file
//           offset; the host parses it with the SAME routine (mg_parse is host and device code) in its wider setting.
//   rows    one wave per (CHROM, POS): the union of the ALT symbols in column order — for every symbol the smallest (column,
//           index in that column's ALT) that carries it, symbols ordered by that pair —, the union of the filters likewise, NS,
//           and the byte length of the row (columns beyond 64 are a loop of the same wave) ...
//   write   ... and, after a prefix sum over the row lengths, the same walk again writing the text at each row's offset.
// Where the records would not fit the device the merge runs in bounded memory (snpgpu_merge_vcf_files_opts): the `lines` kernel
// below is the parse kernel's walk once for the keys of all lines and once per range of sites for that range's records.
//
// The grammar (the pipeline's own writer, vcf_rows.hip): ten TAB-separated columns; POS a count; ID and QUAL '.'; REF one byte;
// ALT '.' or up to 8 distinct one-byte symbols; FILTER equal to FT; INFO NS=<n>; FORMAT GT:SDP:RD:AD:RDF:RDR:ADF:ADR:FT; GT '.'
// or one digit; SDP RD RDF RDR counts; AD ADF ADR one value ('.' or a count) per ALT symbol (one value under ALT '.'); FT PASS
// or ';'-joined filter ids of the header in header order.  On the device a count has at most 9 digits and NS is 1; the host
// takes 10 digits below 2^32 - 1 and any NS.  Nothing else is pinned by the reference's files, and nothing else is merged.
#include "internal.h"
#include "prims.h"

namespace {

constexpr uint32_t MG_TILE = SNPGPU_VCF_TILE, MG_LOOK = SNPGPU_VCF_LOOK, MG_THREADS = 256, MG_LANE_BYTES = MG_TILE / MG_THREADS;
static_assert(MG_LANE_BYTES == 64 && MG_LOOK % 16 == 0, "a lane scans four 16-byte words");
constexpr uint32_t MG_DOT = 0xFFFFFFFFu;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__host__ __device__ inline bool mg_num(const uint8_t *p, uint32_t a, uint32_t b, uint32_t max_digits, uint32_t *out) {
    if (b <= a || b - a > max_digits) return false;
    uint64_t v = 0;
    for (uint32_t i = a; i < b; ++i) {
        const uint32_t d = p[i] - 48u;
        if (d > 9u) return false;
        v = v * 10 + d;
    }
    if (v >= MG_DOT) return false;
    *out = (uint32_t)v;
    return true;
}

}  // namespace

// The record of the data line p[s, e) (no terminator, no CR), false when the line is outside the grammar.  filt: the filter ids
// back to back, filt_off[n_filt + 1].  strict: the device's setting.
__host__ __device__ bool snpgpu_merge_parse_line(const uint8_t *p, uint32_t s, uint32_t e, const uint8_t *filt, const uint32_t *filt_off, uint32_t n_filt,
                                                 bool strict, snpgpu_merge_cell *c) {
    uint32_t tab[9], n_tab = 0;
    for (uint32_t i = s; i < e; ++i)
        if (p[i] == '\t') {
            if (n_tab == 9) return false;
            tab[n_tab++] = i;
        }
    if (n_tab != 9 || tab[0] == s) return false;
    const uint32_t digits = strict ? 9 : 10;
    uint64_t h = 1469598103934665603ull;                        // FNV-1a over CHROM: which contig it is comes out of a sort of these
    for (uint32_t i = s; i < tab[0]; ++i) h = (h ^ p[i]) * 1099511628211ull;
    c->key = h;
    if (!mg_num(p, tab[0] + 1, tab[1], digits, &c->pos)) return false;
    if (tab[2] - tab[1] != 2 || p[tab[1] + 1] != '.' || tab[5] - tab[4] != 2 || p[tab[4] + 1] != '.') return false;
    if (tab[3] - tab[2] != 2) return false;
    const uint8_t ref = p[tab[2] + 1];
    if (ref == '.' || ref == ',') return false;
    c->ref = ref;
    uint32_t n_alt = 0;
    for (uint32_t k = 0; k < 8; ++k) c->alt[k] = 0;
    if (!(tab[4] - tab[3] == 2 && p[tab[3] + 1] == '.')) {
        const uint32_t a = tab[3] + 1, b = tab[4];
        if (b <= a || ((b - a) & 1) == 0 || (b - a + 1) / 2 > 8) return false;
        for (uint32_t i = a; i < b; ++i) {
            if ((i - a) & 1) { if (p[i] != ',') return false; continue; }
            const uint8_t sym = p[i];
            if (sym == '.' || sym == ',' || sym == ref) return false;
            for (uint32_t k = 0; k < n_alt; ++k) if (c->alt[k] == sym) return false;
            c->alt[n_alt++] = sym;
        }
    }
    c->n_alt = (uint8_t)n_alt;
    if (tab[7] - tab[6] < 5 || p[tab[6] + 1] != 'N' || p[tab[6] + 2] != 'S' || p[tab[6] + 3] != '=') return false;
    if (!mg_num(p, tab[6] + 4, tab[7], digits, &c->ns)) return false;
    if (strict && !(tab[7] - tab[6] == 5 && c->ns == 1)) return false;
    const char fmt[] = "GT:SDP:RD:AD:RDF:RDR:ADF:ADR:FT";
    if (tab[8] - tab[7] - 1 != sizeof(fmt) - 1) return false;
    for (uint32_t i = 0; i < sizeof(fmt) - 1; ++i) if (p[tab[7] + 1 + i] != (uint8_t)fmt[i]) return false;
    uint32_t col[8], n_col = 0;
    for (uint32_t i = tab[8] + 1; i < e; ++i)
        if (p[i] == ':') {
            if (n_col == 8) return false;
            col[n_col++] = i;
        }
    if (n_col != 8) return false;
    const uint32_t f0 = tab[8] + 1;
    if (col[0] - f0 != 1) return false;
    if (p[f0] == '.') c->gt = 0xFF;
    else {
        const uint32_t g = p[f0] - 48u;
        if (g > n_alt) return false;                            // (and no digit at all: g is huge)
        c->gt = (uint8_t)g;
    }
    if (!mg_num(p, col[0] + 1, col[1], digits, &c->sdp) || !mg_num(p, col[1] + 1, col[2], digits, &c->rd) ||
        !mg_num(p, col[3] + 1, col[4], digits, &c->rdf) || !mg_num(p, col[4] + 1, col[5], digits, &c->rdr)) return false;
    const uint32_t va[3] = {col[2] + 1, col[5] + 1, col[6] + 1}, vb[3] = {col[3], col[6], col[7]};
    for (uint32_t v = 0; v < 3; ++v) {
        uint32_t *dst = v == 0 ? c->ad : v == 1 ? c->adf : c->adr;
        uint32_t k = 0, a = va[v];
        for (uint32_t i = va[v]; i <= vb[v]; ++i) {
            if (i < vb[v] && p[i] != ',') continue;
            uint32_t value = MG_DOT;
            if (!(i - a == 1 && p[a] == '.') && !mg_num(p, a, i, digits, &value)) return false;
            if (k >= 8) return false;
            dst[k++] = value;
            a = i + 1;
        }
        if (k != (n_alt ? n_alt : 1)) return false;
        for (; k < 8; ++k) dst[k] = MG_DOT;
    }
    // FT: the same bytes as FILTER; PASS, or filter ids in header order
    const uint32_t ft_a = col[7] + 1, ft_n = e - ft_a, fl_a = tab[5] + 1;
    if (ft_n == 0 || tab[6] - fl_a != ft_n) return false;
    for (uint32_t i = 0; i < ft_n; ++i) if (p[ft_a + i] != p[fl_a + i]) return false;
    uint32_t mask = 0;
    if (!(ft_n == 4 && p[ft_a] == 'P' && p[ft_a + 1] == 'A' && p[ft_a + 2] == 'S' && p[ft_a + 3] == 'S')) {
        uint32_t next = 0, a = ft_a;
        for (uint32_t i = ft_a; i <= e; ++i) {
            if (i < e && p[i] != ';') continue;
            bool hit = false;
            for (; next < n_filt && !hit; ++next) {
                const uint32_t len = filt_off[next + 1] - filt_off[next];
                if (len != i - a) continue;
                hit = true;
                for (uint32_t k = 0; k < len; ++k) if (filt[filt_off[next] + k] != p[a + k]) { hit = false; break; }
                if (hit) mask |= 1u << next;
            }
            if (!hit) return false;
            a = i + 1;
        }
    }
    c->ft_mask = mask;
    c->idx = 0;
    c->pad = 0;
    return true;
}

namespace {

// buf[0, n): a piece of the file of `column` that starts at file offset file_off; this launch owns the terminators at
// [own_from, n).  ctl: [0] cells [1] lines left to the host [2] error bits.  unusual: (column, offset) pairs — the offset of the
// line's first byte, or of its terminator with bit 63 set when the line does not start inside the window.
__global__ void __launch_bounds__(MG_THREADS) merge_parse_kernel(const uint8_t *__restrict__ buf, uint32_t n, uint32_t own_from, uint64_t file_off, uint32_t column,
                                                                  snpgpu_merge_cell *__restrict__ cells, uint64_t cell_cap, unsigned long long *__restrict__ ctl,
                                                                  unsigned long long *__restrict__ unusual, uint32_t unusual_cap,
                                                                  const uint8_t *__restrict__ filt, const uint32_t *__restrict__ filt_off, uint32_t n_filt) {
    __shared__ u32x4 tile4[(MG_LOOK + MG_TILE) / 16];
    const uint32_t t0 = own_from + blockIdx.x * MG_TILE;
    const uint32_t t1 = n - t0 < MG_TILE ? n : t0 + MG_TILE;
    const uint32_t l0 = t0 >= MG_LOOK ? t0 - MG_LOOK : 0;
    for (uint32_t i = threadIdx.x; i < (MG_LOOK + MG_TILE) / 16; i += MG_THREADS)
        if (l0 + i * 16 < t1) tile4[i] = __builtin_nontemporal_load((const u32x4 *)(buf + l0) + i);
    __syncthreads();
    const uint8_t *lds = (const uint8_t *)tile4;                 // lds[i] is buf[l0 + i]
    const uint32_t lane0 = t0 + threadIdx.x * MG_LANE_BYTES;
    for (uint32_t w = 0; w < MG_LANE_BYTES / 16 && lane0 + w * 16 < t1; ++w) {
        const u32x4 v = tile4[(lane0 + w * 16 - l0) / 16];
        const uint32_t words[4] = {v.x, v.y, v.z, v.w};
        for (uint32_t k = 0; k < 16; ++k) {
            if (((words[k / 4] >> (8 * (k % 4))) & 0xFF) != '\n') continue;
            const uint32_t p = lane0 + w * 16 + k;
            if (p >= t1) continue;
            const uint32_t lim = p >= MG_LOOK ? p - MG_LOOK + 1 : 0;
            uint32_t s = p;
            while (s > lim && lds[s - 1 - l0] != '\n') --s;
            const bool found = s == 0 ? file_off == 0 : lds[s - 1 - l0] == '\n';
            uint32_t e = p;
            if (e > s && lds[e - 1 - l0] == '\r') --e;
            uint64_t where = file_off + s;
            bool ok = false;
            snpgpu_merge_cell c;
            if (!found) where = (file_off + p) | (1ull << 63);
            else if (e == s || lds[s - l0] == '#') continue;
            else ok = snpgpu_merge_parse_line(lds, s - l0, e - l0, filt, filt_off, n_filt, true, &c);
            if (ok) {
                c.off = where;
                c.column = column;
                const unsigned long long at = atomicAdd(&ctl[0], 1ull);
                if (at < cell_cap) cells[at] = c;
                else atomicOr(&ctl[2], 1ull);
            } else {
                const unsigned long long at = atomicAdd(&ctl[1], 1ull);
                if (at < unusual_cap) { unusual[2 * at] = column; unusual[2 * at + 1] = where; }
            }
        }
    }
}

__device__ __forceinline__ uint32_t lower_bound64(const uint64_t *a, uint32_t n, uint64_t key) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void merge_hash_keys_kernel(const snpgpu_merge_cell *cells, uint64_t n, uint64_t *keys, uint32_t *zeros) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { keys[i] = cells[i].key; zeros[i] = 0; }
}

// which of the n_u distinct CHROM hashes a cell has, and the first (column, offset) that carries each
__global__ void merge_contig_first_kernel(snpgpu_merge_cell *cells, uint64_t n, const uint64_t *uniq, const uint32_t *n_u, unsigned long long *first) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t at = lower_bound64(uniq, n_u[0], cells[i].key);
    cells[i].idx = at;
    atomicMin(&first[at], ((unsigned long long)cells[i].column << 40) | (cells[i].off & ((1ull << 40) - 1)));
}

__global__ void merge_site_keys_kernel(snpgpu_merge_cell *cells, uint64_t n, const uint32_t *rank, uint64_t *keys, uint32_t *cols) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = ((uint64_t)rank[cells[i].idx] << 32) | cells[i].pos;
    cells[i].key = key;
    keys[i] = key;
    cols[i] = cells[i].column;
}

// table[site][column] = cell + 1; a second record of one column at one position is an error (ctl[2] bit 1, ctl[3] = a cell of it)
__global__ void merge_scatter_kernel(const snpgpu_merge_cell *cells, uint64_t n, const uint64_t *sites, const uint32_t *n_sites, uint32_t n_col, uint32_t *table,
                                     unsigned long long *ctl) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = lower_bound64(sites, n_sites[0], cells[i].key);
    if (atomicCAS(&table[(uint64_t)s * n_col + cells[i].column], 0u, (uint32_t)i + 1) != 0) {
        atomicOr(&ctl[2], 2ull);
        ctl[3] = i;
    }
}

// ---- the bounded route (stream.hip: merge_vcf_files_bounded): a key pass over all files, then one pass per range of sites -----
// CHROM hash and POS of the line p[s, e) as snpgpu_merge_parse_line (strict) derives them; false where it fails on them
__device__ __forceinline__ bool mg_line_key(const uint8_t *p, uint32_t s, uint32_t e, uint64_t *hash, uint32_t *pos) {
    uint32_t t0 = s;
    uint64_t h = 1469598103934665603ull;
    for (; t0 < e && p[t0] != '\t'; ++t0) h = (h ^ p[t0]) * 1099511628211ull;
    if (t0 == s || t0 == e) return false;
    uint32_t t1 = t0 + 1;
    while (t1 < e && p[t1] != '\t') ++t1;
    *hash = h;
    return t1 < e && mg_num(p, t0 + 1, t1, 9, pos);
}

// a record of the site range into its slot [site - lo][column]; a slot taken is a position that comes twice in one file
// (ctl[2] bit 1, ctl[3] = column << 40 | offset of a line of it)
__device__ __forceinline__ void mg_place(const snpgpu_merge_cell &c, uint64_t slot, snpgpu_merge_cell *cells, uint32_t *table, unsigned long long *ctl) {
    if (atomicCAS(&table[slot], 0u, (uint32_t)slot + 1) == 0) {
        cells[slot] = c;
        atomicAdd(&ctl[0], 1ull);
    } else {
        atomicOr(&ctl[2], 2ull);
        ctl[3] = ((unsigned long long)c.column << 40) | (c.off & ((1ull << 40) - 1));
    }
}

// The walk of merge_parse_kernel over the same bytes with the same ownership rule.  kKeys: every line inside the grammar leaves its
// snpgpu_merge_key, every other line its (column, offset) for the host, as there.  !kKeys: a line whose (contig, POS) ranks inside
// [rg.lo, rg.hi) of the sorted site keys becomes the record of its slot; the lines of the host are the host's (it holds their
// records from the key pass), so nothing is reported.
template <bool kKeys>
__global__ void __launch_bounds__(MG_THREADS) merge_lines_kernel(const uint8_t *__restrict__ buf, uint32_t n, uint32_t own_from, uint64_t file_off, uint32_t column,
                                                                  snpgpu_merge_key *__restrict__ keys, uint64_t key_cap, const snpgpu_merge_range rg,
                                                                  unsigned long long *__restrict__ ctl, unsigned long long *__restrict__ unusual, uint32_t unusual_cap,
                                                                  const uint8_t *__restrict__ filt, const uint32_t *__restrict__ filt_off, uint32_t n_filt) {
    __shared__ u32x4 tile4[(MG_LOOK + MG_TILE) / 16];
    const uint32_t t0 = own_from + blockIdx.x * MG_TILE;
    const uint32_t t1 = n - t0 < MG_TILE ? n : t0 + MG_TILE;
    const uint32_t l0 = t0 >= MG_LOOK ? t0 - MG_LOOK : 0;
    for (uint32_t i = threadIdx.x; i < (MG_LOOK + MG_TILE) / 16; i += MG_THREADS)
        if (l0 + i * 16 < t1) tile4[i] = __builtin_nontemporal_load((const u32x4 *)(buf + l0) + i);
    __syncthreads();
    const uint8_t *lds = (const uint8_t *)tile4;                 // lds[i] is buf[l0 + i]
    const uint32_t lane0 = t0 + threadIdx.x * MG_LANE_BYTES;
    for (uint32_t w = 0; w < MG_LANE_BYTES / 16 && lane0 + w * 16 < t1; ++w) {
        const u32x4 v = tile4[(lane0 + w * 16 - l0) / 16];
        const uint32_t words[4] = {v.x, v.y, v.z, v.w};
        for (uint32_t k = 0; k < 16; ++k) {
            if (((words[k / 4] >> (8 * (k % 4))) & 0xFF) != '\n') continue;
            const uint32_t p = lane0 + w * 16 + k;
            if (p >= t1) continue;
            const uint32_t lim = p >= MG_LOOK ? p - MG_LOOK + 1 : 0;
            uint32_t s = p;
            while (s > lim && lds[s - 1 - l0] != '\n') --s;
            const bool found = s == 0 ? file_off == 0 : lds[s - 1 - l0] == '\n';
            uint32_t e = p;
            if (e > s && lds[e - 1 - l0] == '\r') --e;
            if (found && (e == s || lds[s - l0] == '#')) continue;
            snpgpu_merge_cell c;
            if (kKeys) {
                const uint64_t where = found ? file_off + s : (file_off + p) | (1ull << 63);
                if (found && snpgpu_merge_parse_line(lds, s - l0, e - l0, filt, filt_off, n_filt, true, &c)) {
                    const unsigned long long at = atomicAdd(&ctl[0], 1ull);
                    if (at < key_cap) keys[at] = snpgpu_merge_key{c.key, where, c.pos, column};
                    else atomicOr(&ctl[2], 1ull);
                } else {
                    const unsigned long long at = atomicAdd(&ctl[1], 1ull);
                    if (at < unusual_cap) { unusual[2 * at] = column; unusual[2 * at + 1] = where; }
                }
            } else {
                uint64_t hash;
                uint32_t pos;
                if (!found || !mg_line_key(lds, s - l0, e - l0, &hash, &pos)) continue;
                const uint32_t contig = lower_bound64(rg.hashes, rg.n_contigs, hash);
                if (contig == rg.n_contigs || rg.hashes[contig] != hash) continue;
                const uint64_t key = ((uint64_t)rg.rank[contig] << 32) | pos;
                const uint32_t site = lower_bound64(rg.sites, rg.n_sites, key);
                if (site < rg.lo || site >= rg.hi || rg.sites[site] != key) continue;
                if (!snpgpu_merge_parse_line(lds, s - l0, e - l0, filt, filt_off, n_filt, true, &c)) continue;
                c.key = key;
                c.idx = site;
                c.off = file_off + s;
                c.column = column;
                mg_place(c, (uint64_t)(site - rg.lo) * rg.n_col + column, rg.cells, rg.table, ctl);
            }
        }
    }
}

__global__ void merge_key_hashes_kernel(const snpgpu_merge_key *rec, uint32_t n, uint64_t *keys, uint32_t *zeros) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { keys[i] = rec[i].hash; zeros[i] = 0; }
}

// which of the batch's n_u distinct CHROM hashes a key has, and the first (column, offset) that carries each
__global__ void merge_key_first_kernel(const snpgpu_merge_key *rec, uint32_t n, const uint64_t *uniq, const uint32_t *n_u, uint32_t *which, unsigned long long *first) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t at = lower_bound64(uniq, n_u[0], rec[i].hash);
    which[i] = at;
    atomicMin(&first[at], ((unsigned long long)rec[i].column << 40) | (rec[i].off & ((1ull << 40) - 1)));
}

// keys[i] = (id[which[i]] << 32) | POS: id is the contig's number for now (order of appearance over the batches)
__global__ void merge_key_sites_kernel(const snpgpu_merge_key *rec, uint32_t n, const uint32_t *which, const uint32_t *id, uint64_t *keys, uint32_t *zeros) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { keys[i] = ((uint64_t)id[which[i]] << 32) | rec[i].pos; zeros[i] = 0; }
}

// the site union once every batch is in: the contig's number for now becomes its rank in order of first appearance over the columns
__global__ void merge_key_rank_kernel(uint64_t *keys, uint32_t n, const uint32_t *rank, uint32_t *zeros) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { keys[i] = ((uint64_t)rank[keys[i] >> 32] << 32) | (uint32_t)keys[i]; zeros[i] = 0; }
}

// the records the host parsed (idx = the site's rank, key and column set) into their slots of the range that starts at site lo
__global__ void merge_place_kernel(const snpgpu_merge_cell *extra, uint32_t n, uint32_t lo, uint32_t n_col, snpgpu_merge_cell *cells, uint32_t *table, unsigned long long *ctl) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) mg_place(extra[i], (uint64_t)(extra[i].idx - lo) * n_col + extra[i].column, cells, table, ctl);
}

template <bool kWrite>
struct Emit {
    uint8_t *p;
    uint64_t n = 0;
    __device__ __forceinline__ void ch(uint32_t c) { if (kWrite) p[n] = (uint8_t)c; ++n; }
    __device__ __forceinline__ void num(uint32_t v) {
        uint8_t d[10];
        uint32_t k = 0;
        do { d[k++] = (uint8_t)(48 + v % 10); v /= 10; } while (v);
        while (k) ch(d[--k]);
    }
    __device__ __forceinline__ void text(const uint8_t *s, uint32_t len) { for (uint32_t i = 0; i < len; ++i) ch(s[i]); }
    __device__ __forceinline__ void filters(uint32_t mask, const uint8_t *order, uint32_t n_order, const uint8_t *filt, const uint32_t *filt_off) {
        if (!n_order) { ch('P'); ch('A'); ch('S'); ch('S'); return; }
        bool sep = false;
        for (uint32_t k = 0; k < n_order; ++k) {
            const uint32_t f = order[k];
            if (!(mask >> f & 1)) continue;
            if (sep) ch(';');
            sep = true;
            text(filt + filt_off[f], filt_off[f + 1] - filt_off[f]);
        }
    }
};

constexpr uint32_t MR_WAVES = 4;

// One wave per site of [site_lo, site_hi).  kWrite = false: row_len[site] = bytes of the row with its LF.  kWrite = true: the row at
// out + (row_end[site] - its length - out_base), out_base being the text offset at which this round's buffer starts.
template <bool kWrite>
__global__ void __launch_bounds__(64 * MR_WAVES) merge_rows_kernel(const snpgpu_merge_cell *__restrict__ cells, const uint32_t *__restrict__ table, uint32_t n_col,
                                                                    const uint64_t *__restrict__ site_keys, uint32_t site_lo, uint32_t site_hi, uint64_t out_base,
                                                                    const uint8_t *__restrict__ names,
                                                                    const uint32_t *__restrict__ name_off, const uint8_t *__restrict__ filt,
                                                                    const uint32_t *__restrict__ filt_off, uint64_t *__restrict__ row_len,
                                                                    const uint64_t *__restrict__ row_end, uint8_t *__restrict__ out, unsigned long long *__restrict__ ctl) {
    __shared__ uint32_t a_first[MR_WAVES][256];                  // per symbol: the smallest column * 16 + index in its ALT that carries it
    __shared__ uint32_t f_first[MR_WAVES][32];                   // per filter: the smallest column * 32 + id
    __shared__ uint8_t a_new[MR_WAVES][256], a_order[MR_WAVES][256], f_order[MR_WAVES][32];
    __shared__ uint32_t first_col[MR_WAVES];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t site_raw = site_lo + blockIdx.x * MR_WAVES + w;
    const bool live = site_raw < site_hi;
    const uint32_t site = live ? site_raw : site_hi - 1;         // (a spare wave walks the last site again and writes nothing)
    for (uint32_t i = lane; i < 256; i += 64) a_first[w][i] = ~0u;
    if (lane < 32) f_first[w][lane] = ~0u;
    if (lane == 0) first_col[w] = ~0u;
    __syncthreads();
    const uint32_t *row = table + (uint64_t)site * n_col;
    uint32_t ns = 0;
    for (uint32_t c = lane; c < n_col; c += 64) {
        const uint32_t ci = row[c];
        if (!ci) continue;
        const snpgpu_merge_cell &cell = cells[ci - 1];
        for (uint32_t k = 0; k < cell.n_alt; ++k) atomicMin(&a_first[w][cell.alt[k]], c * 16 + k);
        for (uint32_t m = cell.ft_mask; m; m &= m - 1) { const uint32_t f = __ffs(m) - 1; atomicMin(&f_first[w][f], c * 32 + f); }
        atomicMin(&first_col[w], c);
        ns += cell.ns;
    }
    for (uint32_t d = 32; d; d >>= 1) ns += __shfl_xor(ns, d);
    __syncthreads();
    // the order of the symbols: rank = how many carry a smaller pair
    uint32_t n_alt = 0, n_flt = 0;
    for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t sym = lane + 64 * j, mine = a_first[w][sym];
        n_alt += __popcll(__ballot(mine != ~0u));                // (the whole wave is here in every round: no lane leaves the loop early)
        if (mine != ~0u) {
            uint32_t rank = 0;
            for (uint32_t t = 0; t < 256; ++t) rank += a_first[w][t] < mine;
            a_order[w][rank] = (uint8_t)sym;
            a_new[w][sym] = (uint8_t)(rank + 1);               // (at most 255 symbols besides REF)
        }
    }
    {
        const uint32_t mine = lane < 32 ? f_first[w][lane] : ~0u;
        n_flt = __popcll(__ballot(mine != ~0u));
        if (mine != ~0u) {
            uint32_t rank = 0;
            for (uint32_t t = 0; t < 32; ++t) rank += f_first[w][t] < mine;
            f_order[w][rank] = (uint8_t)lane;
        }
    }
    __syncthreads();
    const snpgpu_merge_cell &head = cells[row[first_col[w]] - 1];   // (a site has at least one record)
    const uint8_t ref = head.ref;
    uint32_t union_mask = 0;
    for (uint32_t k = 0; k < n_flt; ++k) union_mask |= 1u << f_order[w][k];
    // the fixed columns: the same for every lane; lane 0 writes them
    const uint64_t key = site_keys[site];
    const uint32_t contig = (uint32_t)(key >> 32);
    uint64_t base = 0;
    uint8_t *dst = kWrite ? out + (row_end[site] - row_len[site] - out_base) : nullptr;
    {
        Emit<kWrite> em;                                        // every lane counts the fixed columns, lane 0 writes them
        em.p = dst;
        const bool wr = lane == 0 && live;
        Emit<false> cnt;
        cnt.p = nullptr;
#define MG_PREFIX(E)                                                                                          \
        E.text(names + name_off[contig], name_off[contig + 1] - name_off[contig]); E.ch('\t');                    \
        E.num((uint32_t)key); E.ch('\t'); E.ch('.'); E.ch('\t'); E.ch(ref); E.ch('\t');                           \
        if (!n_alt) E.ch('.');                                                                                    \
        for (uint32_t k = 0; k < n_alt; ++k) { if (k) E.ch(','); E.ch(a_order[w][k]); }                           \
        E.ch('\t'); E.ch('.'); E.ch('\t'); E.filters(union_mask, f_order[w], n_flt, filt, filt_off); E.ch('\t'); \
        E.ch('N'); E.ch('S'); E.ch('='); E.num(ns); E.ch('\t');                                                   \
        { const char fmt[] = "GT:SDP:RD:AD:RDF:RDR:ADF:ADR:FT"; for (uint32_t i = 0; i < sizeof(fmt) - 1; ++i) E.ch(fmt[i]); }
        MG_PREFIX(cnt)
        if (kWrite && wr) { MG_PREFIX(em) }
#undef MG_PREFIX
        base = cnt.n;
    }
    // the sample columns, 64 at a time: lengths, a prefix sum over the wave, then the text
    for (uint32_t c0 = 0; c0 < n_col; c0 += 64) {
        const uint32_t c = c0 + lane;
        const uint32_t ci = c < n_col ? row[c] : 0;
        uint64_t len = 0;
        for (int pass = 0; pass < (kWrite ? 2 : 1); ++pass) {
            const bool writing = pass == 1;
            uint64_t at = 0;
            if (writing) {
                const uint32_t incl = wave_inclusive_sum((uint32_t)len);
                at = base + incl - len;
                base += __shfl(incl, 63);
            }
            if (c < n_col && (!writing || live)) {
                uint8_t *q = writing ? dst + at : nullptr;
                uint64_t m = 0;
#define PUT(ch_) do { const uint8_t b_ = (uint8_t)(ch_); if (writing) q[m] = b_; ++m; } while (0)   // (ch_ may step a counter: both passes evaluate it)
                auto put_num = [&](uint32_t v) {
                    uint8_t d[10];
                    uint32_t k = 0;
                    do { d[k++] = (uint8_t)(48 + v % 10); v /= 10; } while (v);
                    while (k) PUT(d[--k]);
                };
                PUT('\t');
                if (!ci) {
                    for (uint32_t k = 0; k < 9; ++k) { if (k) PUT(':'); PUT('.'); }
                } else {
                    const snpgpu_merge_cell &cell = cells[ci - 1];
                    if (cell.ref != ref) atomicOr(&ctl[2], 4ull);
                    auto put_vec = [&](const uint32_t *own) {
                        if (!n_alt) { PUT('.'); return; }
                        for (uint32_t k = 0; k < n_alt; ++k) {
                            if (k) PUT(',');
                            const uint8_t sym = a_order[w][k];
                            uint32_t v = MG_DOT;
                            for (uint32_t j = 0; j < cell.n_alt; ++j) if (cell.alt[j] == sym) v = own[j];
                            if (v == MG_DOT) PUT('.'); else put_num(v);
                        }
                    };
                    if (cell.gt == 0xFF) PUT('.');
                    else put_num(cell.gt ? a_new[w][cell.alt[cell.gt - 1]] : 0u);
                    PUT(':'); put_num(cell.sdp); PUT(':'); put_num(cell.rd); PUT(':'); put_vec(cell.ad);
                    PUT(':'); put_num(cell.rdf); PUT(':'); put_num(cell.rdr); PUT(':'); put_vec(cell.adf); PUT(':'); put_vec(cell.adr); PUT(':');
                    if (!cell.ft_mask) { PUT('P'); PUT('A'); PUT('S'); PUT('S'); }
                    else {
                        bool sep = false;
                        for (uint32_t mm = cell.ft_mask; mm; mm &= mm - 1) {           // its own filters: header order, as it wrote them
                            const uint32_t f = __ffs(mm) - 1;
                            if (sep) PUT(';');
                            sep = true;
                            for (uint32_t k = filt_off[f]; k < filt_off[f + 1]; ++k) PUT(filt[k]);
                        }
                    }
                }
#undef PUT
                len = m;
            }
        }
        if (!kWrite) {
            const uint32_t incl = wave_inclusive_sum((uint32_t)len);
            base += __shfl(incl, 63);
        }
    }
    if (live && lane == 0) {
        if (kWrite) dst[base] = '\n';
        else row_len[site] = base + 1;
    }
}

struct PlusU64 { __device__ uint64_t operator()(const uint64_t &a, const uint64_t &b) const { return a + b; } };

inline uint32_t nblk(uint64_t n) { return (uint32_t)((n + 255) / 256); }

}  // namespace

int snpgpu_enqueue_merge_parse(snpgpu_ctx *ctx, const uint8_t *d_buf, uint32_t n, uint32_t own_from, uint64_t file_off, uint32_t column, snpgpu_merge_cell *d_cells,
                               uint64_t cell_cap, uint64_t *d_ctl, uint64_t *d_unusual, uint32_t unusual_cap, const uint8_t *d_filt, const uint32_t *d_filt_off,
                               uint32_t n_filt) {
    if (((uintptr_t)d_buf & 15) || (own_from != 0 && own_from != MG_LOOK) || (own_from == 0) != (file_off == 0))
        return snpgpu_set_error(ctx, SNPGPU_E_ARG, "vcf merge: a piece starts on a 16-byte boundary, with the look-back of the piece before it or at the start of the file");
    if (n <= own_from) return SNPGPU_OK;
    const uint32_t blocks = (n - own_from + MG_TILE - 1) / MG_TILE;
    hipEvent_t ta = snpgpu_time_begin(ctx);
    hipLaunchKernelGGL(merge_parse_kernel, dim3(blocks), dim3(MG_THREADS), 0, ctx->stream, d_buf, n, own_from, file_off, column, d_cells, cell_cap,
                       (unsigned long long *)d_ctl, (unsigned long long *)d_unusual, unusual_cap, d_filt, d_filt_off, n_filt);
    snpgpu_time_end(ctx, SNPGPU_K_VCF_MERGE, ta);
    HIP_TRY(ctx, hipGetLastError());
    return SNPGPU_OK;
}

int snpgpu_enqueue_merge_hash_keys(snpgpu_ctx *ctx, const snpgpu_merge_cell *d_cells, uint64_t n, uint64_t *d_keys, uint32_t *d_zeros) {
    if (n) merge_hash_keys_kernel<<<nblk(n), 256, 0, ctx->stream>>>(d_cells, n, d_keys, d_zeros);
    HIP_TRY(ctx, hipGetLastError());
    return SNPGPU_OK;
}

int snpgpu_enqueue_merge_contig_first(snpgpu_ctx *ctx, snpgpu_merge_cell *d_cells, uint64_t n, const uint64_t *d_uniq, const uint32_t *d_n_uniq, uint64_t *d_first) {
    if (n) merge_contig_first_kernel<<<nblk(n), 256, 0, ctx->stream>>>(d_cells, n, d_uniq, d_n_uniq, (unsigned long long *)d_first);
    HIP_TRY(ctx, hipGetLastError());
    return SNPGPU_OK;
}

int snpgpu_enqueue_merge_site_keys(snpgpu_ctx *ctx, snpgpu_merge_cell *d_cells, uint64_t n, const uint32_t *d_rank, uint64_t *d_keys, uint32_t *d_cols) {
    if (n) merge_site_keys_kernel<<<nblk(n), 256, 0, ctx->stream>>>(d_cells, n, d_rank, d_keys, d_cols);
    HIP_TRY(ctx, hipGetLastError());
    return SNPGPU_OK;
}

int snpgpu_enqueue_merge_scatter(snpgpu_ctx *ctx, const snpgpu_merge_cell *d_cells, uint64_t n, const uint64_t *d_sites, const uint32_t *d_n_sites, uint32_t n_col,
                                 uint32_t *d_table, uint64_t *d_ctl) {
    if (n) merge_scatter_kernel<<<nblk(n), 256, 0, ctx->stream>>>(d_cells, n, d_sites, d_n_sites, n_col, d_table, (unsigned long long *)d_ctl);
    HIP_TRY(ctx, hipGetLastError());
    return SNPGPU_OK;
}

// The bounded route.  keys != 0: the key pass (d_keys[key_cap], unusual as in snpgpu_enqueue_merge_parse); else the pass of a site range.
int snpgpu_enqueue_merge_lines(snpgpu_ctx *ctx, const uint8_t *d_buf, uint32_t n, uint32_t own_from, uint64_t file_off, uint32_t column, snpgpu_merge_key *d_keys,
                               uint64_t key_cap, const snpgpu_merge_range *range, uint64_t *d_ctl, uint64_t *d_unusual, uint32_t unusual_cap, const uint8_t *d_filt,
                               const uint32_t *d_filt_off, uint32_t n_filt) {
    if (((uintptr_t)d_buf & 15) || (own_from != 0 && own_from != MG_LOOK) || (own_from == 0) != (file_off == 0))
        return snpgpu_set_error(ctx, SNPGPU_E_ARG, "vcf merge: a piece starts on a 16-byte boundary, with the look-back of the piece before it or at the start of the file");
    if (!d_keys == !range) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "vcf merge: either the key pass or a site range");
    if (range && (range->lo >= range->hi || range->hi > range->n_sites)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "vcf merge: an empty or outlying range of sites");
    if (n <= own_from) return SNPGPU_OK;
    const uint32_t blocks = (n - own_from + MG_TILE - 1) / MG_TILE;
    hipEvent_t ta = snpgpu_time_begin(ctx);
    if (d_keys)
        hipLaunchKernelGGL(merge_lines_kernel<true>, dim3(blocks), dim3(MG_THREADS), 0, ctx->stream, d_buf, n, own_from, file_off, column, d_keys, key_cap,
                           snpgpu_merge_range{}, (unsigned long long *)d_ctl, (unsigned long long *)d_unusual, unusual_cap, d_filt, d_filt_off, n_filt);
    else
        hipLaunchKernelGGL(merge_lines_kernel<false>, dim3(blocks), dim3(MG_THREADS), 0, ctx->stream, d_buf, n, own_from, file_off, column, (snpgpu_merge_key *)nullptr,
                           (uint64_t)0, *range, (unsigned long long *)d_ctl, (unsigned long long *)nullptr, 0u, d_filt, d_filt_off, n_filt);
    snpgpu_time_end(ctx, SNPGPU_K_VCF_MERGE, ta);
    HIP_TRY(ctx, hipGetLastError());
    return SNPGPU_OK;
}

int snpgpu_enqueue_merge_key_hashes(snpgpu_ctx *ctx, const snpgpu_merge_key *d_rec, uint32_t n, uint64_t *d_keys, uint32_t *d_zeros) {
    if (n) merge_key_hashes_kernel<<<nblk(n), 256, 0, ctx->stream>>>(d_rec, n, d_keys, d_zeros);
    HIP_TRY(ctx, hipGetLastError());
    return SNPGPU_OK;
}

int snpgpu_enqueue_merge_key_first(snpgpu_ctx *ctx, const snpgpu_merge_key *d_rec, uint32_t n, const uint64_t *d_uniq, const uint32_t *d_n_uniq, uint32_t *d_which,
                                   uint64_t *d_first) {
    if (n) merge_key_first_kernel<<<nblk(n), 256, 0, ctx->stream>>>(d_rec, n, d_uniq, d_n_uniq, d_which, (unsigned long long *)d_first);
    HIP_TRY(ctx, hipGetLastError());
    return SNPGPU_OK;
}

int snpgpu_enqueue_merge_key_sites(snpgpu_ctx *ctx, const snpgpu_merge_key *d_rec, uint32_t n, const uint32_t *d_which, const uint32_t *d_id, uint64_t *d_keys,
                                   uint32_t *d_zeros) {
    if (n) merge_key_sites_kernel<<<nblk(n), 256, 0, ctx->stream>>>(d_rec, n, d_which, d_id, d_keys, d_zeros);
    HIP_TRY(ctx, hipGetLastError());
    return SNPGPU_OK;
}

int snpgpu_enqueue_merge_key_rank(snpgpu_ctx *ctx, uint64_t *d_keys, uint32_t n, const uint32_t *d_rank, uint32_t *d_zeros) {
    if (n) merge_key_rank_kernel<<<nblk(n), 256, 0, ctx->stream>>>(d_keys, n, d_rank, d_zeros);
    HIP_TRY(ctx, hipGetLastError());
    return SNPGPU_OK;
}

int snpgpu_enqueue_merge_place(snpgpu_ctx *ctx, const snpgpu_merge_cell *d_extra, uint32_t n, uint32_t lo, uint32_t n_col, snpgpu_merge_cell *d_cells, uint32_t *d_table,
                               uint64_t *d_ctl) {
    if (n) merge_place_kernel<<<nblk(n), 256, 0, ctx->stream>>>(d_extra, n, lo, n_col, d_cells, d_table, (unsigned long long *)d_ctl);
    HIP_TRY(ctx, hipGetLastError());
    return SNPGPU_OK;
}

size_t snpgpu_merge_rows_scan_words(uint32_t n_sites) { return prim_gscan_blocks(n_sites); }

// rows: write == 0, over all n_sites: lengths and their running sum (d_row_end, inclusive).  write != 0, once per round: the text of the
// sites [site_lo, site_hi) into d_out, whose first byte is the text offset out_base = row_end[site_lo] - row_len[site_lo].
int snpgpu_enqueue_merge_rows(snpgpu_ctx *ctx, int write, const snpgpu_merge_cell *d_cells, const uint32_t *d_table, uint32_t n_col, const uint64_t *d_site_keys,
                              uint32_t n_sites, uint32_t site_lo, uint32_t site_hi, uint64_t out_base, const uint8_t *d_names, const uint32_t *d_name_off, const uint8_t *d_filt, const uint32_t *d_filt_off,
                              uint64_t *d_row_len, uint64_t *d_row_end, uint64_t *d_scan_ws, uint8_t *d_out, uint64_t *d_ctl) {
    if (!n_sites) return SNPGPU_OK;
    if (!write) { site_lo = 0; site_hi = n_sites; }
    if (site_lo >= site_hi || site_hi > n_sites) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "vcf merge: an empty or outlying range of sites");
    const uint32_t blocks = (site_hi - site_lo + MR_WAVES - 1) / MR_WAVES;
    hipEvent_t ta = snpgpu_time_begin(ctx);
    if (!write) {
        merge_rows_kernel<false><<<blocks, 64 * MR_WAVES, 0, ctx->stream>>>(d_cells, d_table, n_col, d_site_keys, site_lo, site_hi, 0, d_names, d_name_off, d_filt,
                                                                             d_filt_off, d_row_len, d_row_end, nullptr, (unsigned long long *)d_ctl);
        prim_inclusive_scan<uint64_t, PlusU64>(ctx->stream, d_row_len, d_row_end, n_sites, d_scan_ws, PlusU64());
    } else {
        merge_rows_kernel<true><<<blocks, 64 * MR_WAVES, 0, ctx->stream>>>(d_cells, d_table, n_col, d_site_keys, site_lo, site_hi, out_base, d_names, d_name_off, d_filt,
                                                                            d_filt_off, d_row_len, d_row_end, d_out, (unsigned long long *)d_ctl);
    }
    snpgpu_time_end(ctx, SNPGPU_K_VCF_MERGE, ta);
    HIP_TRY(ctx, hipGetLastError());
    return SNPGPU_OK;
}
