// The text outputs of the distance step: host-side formatting (no device code).
//
// snp_distance_pairwise.tsv / snp_distance_matrix.tsv replace the two print loops of snppipeline/distance.py:100-115.  At BASELINE
// configs[4] (10 000 samples) the pairwise file has 10^8 lines: Python's "%s\t%s\t%i\n" loop takes ~35 s for what the distance
// kernel computed in 38 ms.  Every other file here is additive.
//
// Sink.  A writer puts its text into a sink: put(char), put(const char *, size_t), put_i32 (str(int)), a flag `failed`; the other
// numbers and the Newick line are the templates of csrc/text_host.h.  Out holds 4 MiB and lets a full buffer leave with write(), or
// with pwrite() at a running offset (several threads, each its own range of the file); FileOut is the first with its own file;
// CountOut stores nothing and adds the lengths up.
//
// Block scheme (write_row_blocks).  A file of independent rows is a header and a format(sink, r0, r1) for the rows [r0, r1).  Small
// files (below 2^22 values) go through one FileOut.  Else the rows are split into one block per writer thread; every thread runs
// its block into a CountOut, a prefix sum over the counts gives every block its place in the file, and the threads run the same
// format into an Out at that place, side by side.  The text is stated once, so the count cannot disagree with it; a block that
// does not end where the next begins is still an error (E_IO).
#include <errno.h>
#include <fcntl.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "internal.h"
#include "linkage_host.h"
#include "nj_host.h"

namespace {

typedef TxtNames Names;

struct Out {
    int fd;
    bool ranged;                                                // pwrite() at `at`, else write()
    uint64_t at;                                                // bytes that have left (ranged: from the start of the file)
    std::vector<char> buf;
    size_t n = 0;
    bool failed = false;
    Out(int fd_, bool ranged_, uint64_t at_) : fd(fd_), ranged(ranged_), at(at_), buf((size_t)4 << 20) {}
    void flush() {
        size_t done = 0;
        while (!failed && done < n) {
            const ssize_t w = ranged ? pwrite(fd, buf.data() + done, n - done, (off_t)(at + done)) : write(fd, buf.data() + done, n - done);
            if (w < 0) { if (errno == EINTR) continue; failed = true; break; }
            done += (size_t)w;
        }
        at += n;
        n = 0;
    }
    // room for `len` more bytes (len <= half the buffer)
    char *reserve(size_t len) { if (n + len > buf.size()) flush(); return buf.data() + n; }
    void put(const char *s, size_t len) {
        while (len) {                                           // names longer than the buffer are cut into pieces
            const size_t part = len < buf.size() / 2 ? len : buf.size() / 2;
            memcpy(reserve(part), s, part);
            n += part; s += part; len -= part;
        }
    }
    void put(char c) { *reserve(1) = c; ++n; }
    void put_i32(int32_t v) {                                   // "%i" / str(int)
        char *p = reserve(12);
        char tmp[12];
        int k = 0;
        uint32_t u = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
        do { tmp[k++] = (char)('0' + u % 10); u /= 10; } while (u);
        if (v < 0) tmp[k++] = '-';
        for (int i = 0; i < k; ++i) p[i] = tmp[k - 1 - i];
        n += (size_t)k;
    }
};

struct FileOut : Out {
    explicit FileOut(const char *path) : Out(open(path, O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0666), false, 0) { failed = fd < 0; }
    ~FileOut() { if (fd >= 0) close(fd); }
    int finish() {
        flush();
        if (fd >= 0 && close(fd) != 0) failed = true;
        fd = -1;
        return failed ? SNPGPU_E_IO : SNPGPU_OK;
    }
};

struct CountOut {
    uint64_t n = 0;
    static constexpr bool failed = false;
    void put(const char *, size_t len) { n += len; }
    void put(char) { ++n; }
    void put_i32(int32_t v) {                                   // the sign and the digits, without a branch
        const uint32_t u = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
        n += (v < 0) + 1u + (u >= 10u) + (u >= 100u) + (u >= 1000u) + (u >= 10000u) + (u >= 100000u) + (u >= 1000000u) + (u >= 10000000u) +
             (u >= 100000000u) + (u >= 1000000000u);
    }
};

// `work`: the number of values the file holds.  `values_before`: null when every row holds the same number of values, else n + 1
// rising counts (a CSR's row offsets): the blocks then hold equal shares of the values, not of the rows, so that a few dense rows do
// not leave one thread with the whole file (a single row is never split).
template <typename Head, typename Format>
int write_row_blocks(const char *path, uint32_t n, uint64_t work, const uint64_t *values_before, Head header, Format format) {
    unsigned T = snpgpu_writer_threads(0);
    if (work < ((uint64_t)1 << 22)) T = 1;                      // small files: one thread, one stream of write() calls
    if (T > n) T = n ? n : 1;
    if (T <= 1) {
        FileOut o(path);
        if (o.failed) return SNPGPU_E_IO;
        header(o);
        format(o, 0u, n);
        return o.finish();
    }
    auto first_row = [&](unsigned t) -> uint32_t {
        if (t >= T) return n;
        if (!values_before) return (uint32_t)((uint64_t)n * t / T);
        const uint64_t want = (uint64_t)((unsigned __int128)work * t / T);          // the first row that starts at or behind this share
        return (uint32_t)(std::lower_bound(values_before, values_before + n, want) - values_before);
    };
    auto on_threads = [&](auto block) {
        std::vector<std::thread> th;
        for (unsigned t = 1; t < T; ++t) th.emplace_back(block, t);
        block(0u);
        for (auto &x : th) x.join();
    };
    CountOut head;
    header(head);
    std::vector<uint64_t> at(T + 1, head.n);
    on_threads([&](unsigned t) { CountOut c; format(c, first_row(t), first_row(t + 1)); at[t + 1] = c.n; });
    for (unsigned t = 0; t < T; ++t) at[t + 1] += at[t];
    const int fd = open(path, O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0666);
    if (fd < 0) return SNPGPU_E_IO;
    bool failed = ftruncate(fd, (off_t)at[T]) != 0;
    std::vector<uint8_t> bad(T, 0);
    auto write_block = [&](unsigned t) {
        Out o(fd, true, t ? at[t] : 0);                             // the first block starts with the header
        if (t == 0) header(o);
        format(o, first_row(t), first_row(t + 1));
        o.flush();
        bad[t] = o.failed || o.at != at[t + 1];
    };
    if (!failed) {
        on_threads(write_block);
        for (unsigned t = 0; t < T; ++t) failed = failed || bad[t];
    }
    if (close(fd) != 0) failed = true;
    return failed ? SNPGPU_E_IO : SNPGPU_OK;
}

// "id\tid\tdistance": the row of distance.py:105-106
template <typename Sink>
inline void put_pair(Sink &o, const Names &a, uint32_t i, const Names &b, uint32_t j, int32_t d) {
    a.put(o, i); o.put('\t');
    b.put(o, j); o.put('\t');
    o.put_i32(d);
}
template <typename Sink, size_t N>
inline void put_text(Sink &o, const char (&text)[N]) { o.put(text, N - 1); }

// the column as the files name it: its 1-based number, or contig name and position
struct SiteTable {
    Names chrom;
    const uint32_t *chrom_of;
    const uint64_t *pos_of;
    bool given, ok;
    SiteTable(const char *n, const uint64_t *o, const uint32_t *c, const uint64_t *p) : chrom{n, o}, chrom_of(c), pos_of(p) {
        given = n || o || c || p;
        ok = !given || (o && c && p);
    }
    template <typename Sink>
    void put(Sink &o, uint32_t s) const {
        if (!given) { txt_put_u64(o, (uint64_t)s + 1); return; }
        chrom.put(o, chrom_of[s]); o.put('\t');
        txt_put_u64(o, pos_of[s]);
    }
};

}  // namespace

// At 10 000 samples the pairwise file is 3 GB in 10^8 lines: formatted by one thread that alone takes longer than everything
// else the distance subcommand does, and the reason the block scheme exists.
extern "C" int snpgpu_write_distance_tsv(const char *path, int layout, const char *ids, const uint64_t *id_off, uint32_t n,
                                         const int32_t *matrix, uint64_t row_stride) {
    if (!path || (layout != SNPGPU_TSV_PAIRWISE && layout != SNPGPU_TSV_MATRIX) || (n && (!ids || !id_off || !matrix)) || row_stride < n)
        return SNPGPU_E_ARG;
    const Names names{ids, id_off};
    auto header = [&](auto &o) {
        if (layout == SNPGPU_TSV_PAIRWISE) { put_text(o, "Seq1\tSeq2\tDistance\n"); return; }         // distance.py:100-105
        for (uint32_t j = 0; j < n; ++j) { o.put('\t'); names.put(o, j); }                      // distance.py:107-114
        if (n == 0) o.put('\t');                                // '\t%s\n' % '\t'.join([])
        o.put('\n');
    };
    auto format = [&](auto &o, uint32_t r0, uint32_t r1) {
        for (uint32_t i = r0; i < r1 && !o.failed; ++i) {
            const int32_t *row = matrix + (size_t)i * row_stride;
            if (layout == SNPGPU_TSV_PAIRWISE) {
                for (uint32_t j = 0; j < n; ++j) { put_pair(o, names, i, names, j, row[j]); o.put('\n'); }
            } else {
                names.put(o, i);
                for (uint32_t j = 0; j < n; ++j) { o.put('\t'); o.put_i32(row[j]); }
                o.put('\n');
            }
        }
    };
    return write_row_blocks(path, n, (uint64_t)n * n, nullptr, header, format);
}

// ---- close pairs and clusters (additive: the rows of distance.py:93-106 under a threshold, and their single-linkage groups) ----
namespace {
// does a CSR over n rows rise from 0, with every column below n_cols
bool csr_ok(uint32_t n, const uint64_t *row_off, const uint32_t *col, uint32_t n_cols) {
    for (uint32_t i = 0; i < n; ++i)
        if (row_off[i] > row_off[i + 1]) return false;
    const uint64_t n_entries = n ? row_off[n] : 0;
    for (uint64_t e = 0; e < n_entries; ++e)
        if (col[e] >= n_cols) return false;
    return true;
}
// the file of a CSR whose rows name ids of `rows`, its columns ids of `cols`
int write_csr_pairs(const char *path, const Names &rows, uint32_t n, const Names &cols, const uint64_t *row_off, const uint32_t *col, const int32_t *dist) {
    auto header = [&](auto &o) { put_text(o, "Seq1\tSeq2\tDistance\n"); };                             // distance.py:100
    auto format = [&](auto &o, uint32_t r0, uint32_t r1) {
        for (uint32_t i = r0; i < r1 && !o.failed; ++i)
            for (uint64_t e = row_off[i]; e < row_off[i + 1]; ++e) { put_pair(o, rows, i, cols, col[e], dist[e]); o.put('\n'); }
    };
    return write_row_blocks(path, n, n ? row_off[n] : 0, row_off, header, format);
}
}  // namespace

extern "C" int snpgpu_write_close_pairs_tsv(const char *path, const char *ids, const uint64_t *id_off, uint32_t n, const uint64_t *row_off,
                                            const uint32_t *col, const int32_t *dist) {
    if (!path || (n && (!ids || !id_off || !row_off))) return SNPGPU_E_ARG;
    if (n && (row_off[0] != 0 || (row_off[n] && (!col || !dist)))) return SNPGPU_E_ARG;
    if (!csr_ok(n, row_off, col, n)) return SNPGPU_E_ARG;
    return write_csr_pairs(path, {ids, id_off}, n, {ids, id_off}, row_off, col, dist);
}

// The nearest-neighbour file (csrc/nearest.hip): the rows of a CSR over the queries whose columns name database samples.
extern "C" int snpgpu_write_nearest_tsv(const char *path, const char *q_ids, const uint64_t *q_id_off, uint32_t q, const char *db_ids,
                                        const uint64_t *db_id_off, uint32_t n, const uint64_t *row_off, const uint32_t *col, const int32_t *dist) {
    if (!path || (q && (!q_ids || !q_id_off || !row_off))) return SNPGPU_E_ARG;
    if (q && (row_off[0] != 0 || (row_off[q] && (!col || !dist || !db_ids || !db_id_off)))) return SNPGPU_E_ARG;
    if (!csr_ok(q, row_off, col, n)) return SNPGPU_E_ARG;
    return write_csr_pairs(path, {q_ids, q_id_off}, q, {db_ids, db_id_off}, row_off, col, dist);
}

// Pair lists with their compared-site counts (csrc/compared.hip): the rows of a close-pairs, tree or nearest file with a fourth
// column; a[] names ids of the first table, b[] of the second.
extern "C" int snpgpu_write_pair_rows_tsv(const char *path, const char *a_ids, const uint64_t *a_id_off, uint32_t n_a, const char *b_ids,
                                          const uint64_t *b_id_off, uint32_t n_b, const uint32_t *a, const uint32_t *b, const int32_t *dist,
                                          const int32_t *compared, uint64_t n_rows) {
    if (!path || n_rows >> 32 || (n_rows && (!a || !b || !dist || !compared || !a_ids || !a_id_off || !b_ids || !b_id_off))) return SNPGPU_E_ARG;
    for (uint64_t p = 0; p < n_rows; ++p)
        if (a[p] >= n_a || b[p] >= n_b) return SNPGPU_E_ARG;
    const Names a_names{a_ids, a_id_off}, b_names{b_ids, b_id_off};
    auto header = [&](auto &o) { put_text(o, "Seq1\tSeq2\tDistance\tCompared\n"); };
    auto format = [&](auto &o, uint32_t p0, uint32_t p1) {
        for (uint32_t p = p0; p < p1 && !o.failed; ++p) {
            put_pair(o, a_names, a[p], b_names, b[p], dist[p]); o.put('\t');
            o.put_i32(compared[p]); o.put('\n');
        }
    };
    return write_row_blocks(path, (uint32_t)n_rows, n_rows, nullptr, header, format);
}

extern "C" int snpgpu_write_clusters_tsv(const char *path, const char *ids, const uint64_t *id_off, uint32_t n, const int32_t *thresholds,
                                         uint32_t n_thresholds, const uint32_t *numbers) {
    const uint32_t k = n_thresholds;
    if (!path || (k && !thresholds) || (n && (!ids || !id_off || (k && !numbers)))) return SNPGPU_E_ARG;
    const Names names{ids, id_off};
    auto header = [&](auto &o) {
        put_text(o, "Id\t");
        for (uint32_t t = 0; t < k; ++t) { if (t) o.put('\t'); o.put_i32(thresholds[t]); }
        o.put('\n');
    };
    auto format = [&](auto &o, uint32_t r0, uint32_t r1) {
        for (uint32_t i = r0; i < r1 && !o.failed; ++i) {
            names.put(o, i);
            for (uint32_t t = 0; t < k; ++t) { o.put('\t'); o.put_i32((int32_t)numbers[(size_t)t * n + i]); }
            o.put('\n');
        }
    };
    return write_row_blocks(path, n, (uint64_t)n * k, nullptr, header, format);
}

// ---- minimum spanning tree and dendrogram (additive: the tree of csrc/mst.hip as text) ----
extern "C" int snpgpu_write_mst_tsv(const char *path, const char *ids, const uint64_t *id_off, uint32_t n, const uint32_t *u, const uint32_t *v,
                                    const int32_t *dist, uint32_t n_edges) {
    if (!path || (n && (!ids || !id_off)) || (n_edges && (!u || !v || !dist))) return SNPGPU_E_ARG;
    for (uint32_t e = 0; e < n_edges; ++e)
        if (u[e] >= n || v[e] >= n) return SNPGPU_E_ARG;
    const Names names{ids, id_off};
    FileOut o(path);
    if (o.failed) return SNPGPU_E_IO;
    put_text(o, "Seq1\tSeq2\tDistance\n");
    for (uint32_t e = 0; e < n_edges && !o.failed; ++e) { put_pair(o, names, u[e], names, v[e], dist[e]); o.put('\n'); }
    return o.finish();
}

namespace {
// One Newick line (csrc/text_host.h) of the binary tree child[] over n leaves whose last join is the root; above[node]: the length
// of the branch above a node, in millionths.
int write_newick(const char *path, const Names &names, uint32_t n, const std::vector<uint32_t> &child, const std::vector<uint64_t> &above) {
    FileOut o(path);
    if (o.failed) return SNPGPU_E_IO;
    const uint32_t root = (uint32_t)(n + child.size() / 2) - 1;      // (n == 1: leaf 0)
    if (n)
        txt_put_newick(o, names, n, child.data(), root, [&](uint32_t node) {
            if (node != root) { o.put(':'); txt_put_millionths_short(o, above[node]); }
        });
    put_text(o, ";\n");
    return o.finish();
}
}  // namespace

// The edges in their order join the groups of their ends under a node of height d / 2, never through a float: half of d_parent -
// d_child is (d_parent - d_child) * 500 000 millionths, below 2^51.
extern "C" int snpgpu_write_dendrogram_newick(const char *path, const char *ids, const uint64_t *id_off, uint32_t n, const uint32_t *u, const uint32_t *v,
                                              const int32_t *dist, uint32_t n_edges) {
    if (!path || (n && (!ids || !id_off)) || (n_edges && (!u || !v || !dist))) return SNPGPU_E_ARG;
    if (n_edges != (n ? n - 1 : 0)) return SNPGPU_E_ARG;
    std::vector<uint32_t> parent(n), top(n), least(n), child((size_t)n_edges * 2);   // union-find; per set root: its node and its smallest sample
    std::vector<uint64_t> above((size_t)n + n_edges, 0);
    for (uint32_t i = 0; i < n; ++i) parent[i] = top[i] = least[i] = i;
    auto find = [&](uint32_t x) {
        while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
        return x;
    };
    auto d_of = [&](uint32_t node) -> uint64_t { return node < n ? 0 : (uint64_t)dist[node - n]; };
    for (uint32_t e = 0; e < n_edges; ++e) {
        if (u[e] >= n || v[e] >= n || u[e] == v[e] || dist[e] < 0) return SNPGPU_E_ARG;
        if (e) {                                                     // ascending (d, i, j)
            const uint32_t lo0 = std::min(u[e - 1], v[e - 1]), hi0 = std::max(u[e - 1], v[e - 1]), lo1 = std::min(u[e], v[e]), hi1 = std::max(u[e], v[e]);
            if (dist[e - 1] > dist[e] || (dist[e - 1] == dist[e] && (lo0 > lo1 || (lo0 == lo1 && hi0 >= hi1)))) return SNPGPU_E_ARG;
        }
        uint32_t a = find(u[e]), b = find(v[e]);
        if (a == b) return SNPGPU_E_ARG;                             // a cycle: not a tree
        if (least[b] < least[a]) std::swap(a, b);                    // the child with the smaller sample is written first
        child[2 * (size_t)e] = top[a];
        child[2 * (size_t)e + 1] = top[b];
        above[top[a]] = ((uint64_t)dist[e] - d_of(top[a])) * 500000u;
        above[top[b]] = ((uint64_t)dist[e] - d_of(top[b])) * 500000u;
        parent[b] = a;
        top[a] = n + e;
    }
    return write_newick(path, {ids, id_off}, n, child, above);
}

// ---- the differing sites of pairs (additive: the entries of csrc/pair_sites.hip as text) ----
// One row per entry, pair by pair in the order given: the two ids, the column (1-based) — or, with a site table, the contig name
// and position of the column —, and the two bases with their case.  The table is the caller's: chrom_of_site / pos_of_site hold
// one entry per column of the matrix and every `site` lies below their length (not checked here: the writer is not told it).
extern "C" int snpgpu_write_pair_sites_tsv(const char *path, const char *ids, const uint64_t *id_off, uint32_t n, const uint32_t *a, const uint32_t *b,
                                           uint64_t n_pairs, const uint64_t *pair_off, const uint32_t *site, const uint8_t *bases, const char *chrom_names,
                                           const uint64_t *chrom_off, const uint32_t *chrom_of_site, const uint64_t *pos_of_site) {
    const SiteTable table(chrom_names, chrom_off, chrom_of_site, pos_of_site);
    if (!path || (n && (!ids || !id_off)) || n_pairs >> 32 || (n_pairs && (!a || !b || !pair_off)) || !table.ok) return SNPGPU_E_ARG;
    const uint64_t n_entries = n_pairs ? pair_off[n_pairs] : 0;
    if (n_pairs && (pair_off[0] != 0 || (n_entries && (!site || !bases)))) return SNPGPU_E_ARG;
    for (uint64_t p = 0; p < n_pairs; ++p)
        if (pair_off[p] > pair_off[p + 1] || a[p] >= n || b[p] >= n) return SNPGPU_E_ARG;
    if (table.given && n_entries && !chrom_names) return SNPGPU_E_ARG;
    const Names names{ids, id_off};
    auto header = [&](auto &o) {
        if (table.given) put_text(o, "Seq1\tSeq2\tChrom\tPos\tBase1\tBase2\n");
        else put_text(o, "Seq1\tSeq2\tSite\tBase1\tBase2\n");
    };
    auto format = [&](auto &o, uint32_t p0, uint32_t p1) {
        for (uint32_t p = p0; p < p1 && !o.failed; ++p)
            for (uint64_t e = pair_off[p]; e < pair_off[p + 1]; ++e) {
                names.put(o, a[p]); o.put('\t');
                names.put(o, b[p]); o.put('\t');
                table.put(o, site[e]);
                o.put('\t'); o.put("ACGTacgt"[bases[e] & 7]);
                o.put('\t'); o.put("ACGTacgt"[(bases[e] >> 4) & 7]);
                o.put('\n');
            }
    };
    return write_row_blocks(path, (uint32_t)n_pairs, n_entries, pair_off, header, format);
}

// ---- per-site allele counts and cluster-defining SNPs (additive: the arrays of csrc/cluster_snps.hip as text) ----
extern "C" int snpgpu_write_site_counts_tsv(const char *path, const int32_t *counts, uint32_t n_sites, uint32_t n_rows, const char *chrom_names, const uint64_t *chrom_off,
                                            const uint32_t *chrom_of_site, const uint64_t *pos_of_site) {
    const SiteTable table(chrom_names, chrom_off, chrom_of_site, pos_of_site);
    if (!path || (n_sites && !counts) || !table.ok || (table.given && n_sites && !chrom_names)) return SNPGPU_E_ARG;
    for (uint32_t s = 0; s < n_sites; ++s) {
        uint64_t sum = 0;
        for (int b = 0; b < 4; ++b) {
            if (counts[4 * (size_t)s + b] < 0) return SNPGPU_E_ARG;
            sum += (uint64_t)counts[4 * (size_t)s + b];
        }
        if (sum > n_rows) return SNPGPU_E_ARG;
    }
    FileOut o(path);
    if (o.failed) return SNPGPU_E_IO;
    if (table.given) put_text(o, "Chrom\tPos\tA\tC\tG\tT\tOther\n");
    else put_text(o, "Site\tA\tC\tG\tT\tOther\n");
    for (uint32_t s = 0; s < n_sites && !o.failed; ++s) {
        table.put(o, s);
        uint64_t sum = 0;
        for (int b = 0; b < 4; ++b) {
            o.put('\t');
            txt_put_u64(o, (uint64_t)counts[4 * (size_t)s + b]);
            sum += (uint64_t)counts[4 * (size_t)s + b];
        }
        o.put('\t');
        txt_put_u64(o, n_rows - sum);
        o.put('\n');
    }
    return o.finish();
}

extern "C" int snpgpu_write_cluster_snps_tsv(const char *path, const int32_t *thresholds, const uint32_t *n_clusters, uint32_t n_labellings, const uint64_t *cluster_off,
                                             const uint32_t *sizes, const uint32_t *site, const uint8_t *base, const uint32_t *members, uint32_t n_sites,
                                             const char *chrom_names, const uint64_t *chrom_off, const uint32_t *chrom_of_site, const uint64_t *pos_of_site) {
    const SiteTable table(chrom_names, chrom_off, chrom_of_site, pos_of_site);
    if (!path || !table.ok || (n_labellings && (!thresholds || !n_clusters || !cluster_off))) return SNPGPU_E_ARG;
    uint64_t at = 0;                                                 // the offsets rise from 0 through every block
    size_t o_off = 0, o_size = 0;
    for (uint32_t t = 0; t < n_labellings; ++t) {
        if (n_clusters[t] && !sizes) return SNPGPU_E_ARG;
        if (cluster_off[o_off] != at) return SNPGPU_E_ARG;
        for (uint32_t c = 0; c < n_clusters[t]; ++c) {
            if (cluster_off[o_off + c + 1] < cluster_off[o_off + c]) return SNPGPU_E_ARG;
        }
        at = cluster_off[o_off + n_clusters[t]];
        o_off += (size_t)n_clusters[t] + 1;
    }
    if (at && (!site || !base || !members || (table.given && !chrom_names))) return SNPGPU_E_ARG;
    for (uint64_t e = 0; e < at; ++e)
        if (site[e] >= n_sites || base[e] > 3) return SNPGPU_E_ARG;
    FileOut o(path);
    if (o.failed) return SNPGPU_E_IO;
    if (table.given) put_text(o, "Threshold\tCluster\tChrom\tPos\tBase\tMembers\tSize\n");
    else put_text(o, "Threshold\tCluster\tSite\tBase\tMembers\tSize\n");
    o_off = 0;
    for (uint32_t t = 0; t < n_labellings; ++t) {
        for (uint32_t c = 0; c < n_clusters[t] && !o.failed; ++c)
            for (uint64_t e = cluster_off[o_off + c]; e < cluster_off[o_off + c + 1]; ++e) {
                o.put_i32(thresholds[t]); o.put('\t');
                txt_put_u64(o, (uint64_t)c + 1); o.put('\t');
                table.put(o, site[e]); o.put('\t');
                o.put("ACGT"[base[e]]); o.put('\t');
                txt_put_u64(o, members[e]); o.put('\t');
                txt_put_u64(o, sizes[o_size + c]); o.put('\n');
            }
        o_off += (size_t)n_clusters[t] + 1;
        o_size += n_clusters[t];
    }
    return o.finish();
}

// ---- complete- and average-linkage trees (additive: the merges of csrc/linkage.hip as text; the arithmetic is linkage_host.h) ----
extern "C" int snpgpu_write_linkage_tsv(const char *path, const char *ids, const uint64_t *id_off, uint32_t n, int kind, const uint32_t *a, const uint32_t *b,
                                        const uint32_t *size_a, const uint32_t *size_b, const uint64_t *num, uint32_t n_merges) {
    if (!path || (n && (!ids || !id_off)) || !lnk_merges_ok(n, kind, a, b, size_a, size_b, num, n_merges, false, kind == SNPGPU_LINKAGE_AVERAGE)) return SNPGPU_E_ARG;
    const Names names{ids, id_off};
    FileOut o(path);
    if (o.failed) return SNPGPU_E_IO;
    put_text(o, "Seq1\tSeq2\tSize1\tSize2\tDistance\n");
    for (uint32_t e = 0; e < n_merges && !o.failed; ++e) {
        names.put(o, a[e]); o.put('\t');
        names.put(o, b[e]); o.put('\t');
        txt_put_u64(o, size_a[e]); o.put('\t');
        txt_put_u64(o, size_b[e]); o.put('\t');
        if (kind == SNPGPU_LINKAGE_COMPLETE) txt_put_u64(o, num[e]);
        else txt_put_millionths_fixed(o, lnk_average_millionths(num[e], size_a[e], size_b[e]));   // S / (sa sb), half up, exactly six decimals
        o.put('\n');
    }
    return o.finish();
}

// A cluster's node is looked up by its id, which the merge names.  Heights in integer millionths.
extern "C" int snpgpu_write_linkage_newick(const char *path, const char *ids, const uint64_t *id_off, uint32_t n, int kind, const uint32_t *a, const uint32_t *b,
                                           const uint32_t *size_a, const uint32_t *size_b, const uint64_t *num, uint32_t n_merges) {
    if (!path || (n && (!ids || !id_off)) || !lnk_merges_ok(n, kind, a, b, size_a, size_b, num, n_merges, true, true)) return SNPGPU_E_ARG;
    std::vector<uint32_t> top(n), child((size_t)n_merges * 2);
    std::vector<uint64_t> height(n_merges), above((size_t)n + n_merges, 0);
    for (uint32_t i = 0; i < n; ++i) top[i] = i;
    auto h_of = [&](uint32_t node) -> uint64_t { return node < n ? 0 : height[node - n]; };
    for (uint32_t e = 0; e < n_merges; ++e) {                        // the last merge is the root: every other cluster has retired
        height[e] = lnk_height(kind, num[e], size_a[e], size_b[e]);
        if (height[e] < h_of(top[a[e]]) || height[e] < h_of(top[b[e]])) return SNPGPU_E_ARG;      // a child above its parent: not this linkage's tree
        child[2 * (size_t)e] = top[a[e]];                            // a < b: the child with the smaller sample first
        child[2 * (size_t)e + 1] = top[b[e]];
        above[top[a[e]]] = height[e] - h_of(top[a[e]]);
        above[top[b[e]]] = height[e] - h_of(top[b[e]]);
        top[a[e]] = n + e;
    }
    return write_newick(path, {ids, id_off}, n, child, above);
}

// ---- neighbour-joining tree and its bootstrap support (additive: the records of csrc/nj.hip and the counts of csrc/nj_bootstrap.hip
// as text; the checks and the writer are nj_host.h) ----
extern "C" int snpgpu_write_nj_newick(const char *path, const char *ids, const uint64_t *id_off, uint32_t n, const uint32_t *a, const uint32_t *b,
                                      const int64_t *len_a, const int64_t *len_b, uint32_t n_merges, const uint32_t *star, const int64_t *star_len) {
    if (!path || (n && (!ids || !id_off)) || !nj_records_ok(n, a, b, len_a, len_b, n_merges, star, star_len)) return SNPGPU_E_ARG;
    FileOut o(path);
    if (o.failed) return SNPGPU_E_IO;
    nj_put_newick(o, ids, id_off, n, a, b, len_a, len_b, n_merges, star, star_len);
    return o.finish();
}

extern "C" int snpgpu_write_nj_newick_support(const char *path, const char *ids, const uint64_t *id_off, uint32_t n, const uint32_t *a, const uint32_t *b,
                                              const int64_t *len_a, const int64_t *len_b, uint32_t n_merges, const uint32_t *star, const int64_t *star_len,
                                              const uint32_t *support, uint32_t replicates) {
    if (!path || (n && (!ids || !id_off)) || !nj_records_ok(n, a, b, len_a, len_b, n_merges, star, star_len) || !nj_support_ok(support, n_merges, replicates))
        return SNPGPU_E_ARG;
    FileOut o(path);
    if (o.failed) return SNPGPU_E_IO;
    nj_put_newick(o, ids, id_off, n, a, b, len_a, len_b, n_merges, star, star_len, n_merges ? support : nullptr, replicates);
    return o.finish();
}

extern "C" int snpgpu_write_nj_support(const char *path, const char *ids, const uint64_t *id_off, uint32_t n, const uint32_t *a, const uint32_t *b, uint32_t n_merges,
                                       const uint32_t *support, uint32_t replicates) {
    if (!path || (n && (!ids || !id_off)) || !nj_joins_ok(n, a, b, n_merges) || !nj_support_ok(support, n_merges, replicates)) return SNPGPU_E_ARG;
    const Names names{ids, id_off};
    FileOut o(path);
    if (o.failed) return SNPGPU_E_IO;
    put_text(o, "Seq1\tSeq2\tSize\tSupport\tReplicates\n");
    std::vector<uint32_t> size(n, 1);
    for (uint32_t e = 0; e < n_merges && !o.failed; ++e) {
        size[a[e]] += size[b[e]];
        names.put(o, a[e]); o.put('\t');
        names.put(o, b[e]); o.put('\t');
        txt_put_u64(o, size[a[e]]); o.put('\t');
        txt_put_u64(o, support[e]); o.put('\t');
        txt_put_u64(o, replicates); o.put('\n');
    }
    return o.finish();
}
