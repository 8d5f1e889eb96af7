// snp_distance_pairwise.tsv / snp_distance_matrix.tsv from the N x N matrix: host-side text formatting (no device code).
//
// Replaces the two print loops of snppipeline/distance.py:100-115.  At BASELINE configs[4] (10 000 samples) the pairwise
// file has 10^8 lines: Python's "%s\t%s\t%i\n" loop takes ~35 s for what the distance kernel computed in 38 ms; here the
// rows are formatted into a 4 MiB buffer and written with plain write(2) calls.
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

struct FileOut {
    int fd = -1;
    std::vector<char> buf;
    size_t n = 0;
    bool failed = false;
    explicit FileOut(const char *path) : buf((size_t)4 << 20) {
        fd = open(path, O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0666);
        failed = fd < 0;
    }
    ~FileOut() { if (fd >= 0) close(fd); }
    void flush() {
        size_t done = 0;
        while (!failed && done < n) {
            const ssize_t w = write(fd, buf.data() + done, n - done);
            if (w < 0) { if (errno == EINTR) continue; failed = true; break; }
            done += (size_t)w;
        }
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
    int finish() {
        flush();
        if (fd >= 0 && close(fd) != 0) failed = true;
        fd = -1;
        return failed ? SNPGPU_E_IO : SNPGPU_OK;
    }
};
// bytes of str(v)
inline uint32_t digits_i32(int32_t v) {
    uint32_t u = v < 0 ? 0u - (uint32_t)v : (uint32_t)v, k = v < 0 ? 2u : 1u;
    while (u >= 10) { u /= 10; ++k; }
    return k;
}

// Rows [r0, r1) of one of the two layouts into `o` (a FileOut-like sink with put / put_i32).
template <typename Sink>
void format_rows(Sink &o, int layout, const char *ids, const uint64_t *id_off, uint32_t n, const int32_t *matrix, uint64_t row_stride, uint32_t r0, uint32_t r1) {
    auto name = [&](uint32_t i) { o.put(ids + id_off[i], (size_t)(id_off[i + 1] - id_off[i])); };
    for (uint32_t i = r0; i < r1 && !o.failed; ++i) {
        const int32_t *row = matrix + (size_t)i * row_stride;
        if (layout == SNPGPU_TSV_PAIRWISE) {
            for (uint32_t j = 0; j < n; ++j) { name(i); o.put('\t'); name(j); o.put('\t'); o.put_i32(row[j]); o.put('\n'); }
        } else {
            name(i);
            for (uint32_t j = 0; j < n; ++j) { o.put('\t'); o.put_i32(row[j]); }
            o.put('\n');
        }
    }
}

// A sink that writes its buffer at a running offset of an open file (several threads, each its own range of the file).
struct RangeOut {
    int fd;
    uint64_t at;
    std::vector<char> buf;
    size_t n = 0;
    bool failed = false;
    RangeOut(int fd_, uint64_t at_) : fd(fd_), at(at_), buf((size_t)4 << 20) {}
    void flush() {
        size_t done = 0;
        while (!failed && done < n) {
            const ssize_t w = pwrite(fd, buf.data() + done, n - done, (off_t)(at + done));
            if (w < 0) { if (errno == EINTR) continue; failed = true; break; }
            done += (size_t)w;
        }
        at += n;
        n = 0;
    }
    char *reserve(size_t len) { if (n + len > buf.size()) flush(); return buf.data() + n; }
    void put(const char *s, size_t len) {
        while (len) {
            const size_t part = len < buf.size() / 2 ? len : buf.size() / 2;
            memcpy(reserve(part), s, part);
            n += part; s += part; len -= part;
        }
    }
    void put(char c) { *reserve(1) = c; ++n; }
    void put_i32(int32_t v) {
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

}  // namespace

// At 10 000 samples the pairwise file is 3 GB in 10^8 lines: formatted by one thread that alone takes longer than everything
// else the distance subcommand does.  So: the byte length of every row's text first (threads over row blocks), a prefix sum
// gives every block its place in the file, and the blocks are formatted and written with pwrite() side by side.
extern "C" int snpgpu_write_distance_tsv(const char *path, int layout, const char *ids, const uint64_t *id_off, uint32_t n,
                                         const int32_t *matrix, uint64_t row_stride) {
    if (!path || (layout != SNPGPU_TSV_PAIRWISE && layout != SNPGPU_TSV_MATRIX) || (n && (!ids || !id_off || !matrix)) || row_stride < n)
        return SNPGPU_E_ARG;
    unsigned T = snpgpu_writer_threads(0);
    if ((uint64_t)n * n < ((uint64_t)1 << 22)) T = 1;            // small matrices: one thread, one stream of write() calls
    if (T > n) T = n ? n : 1;
    if (T <= 1) {
        FileOut o(path);
        if (o.failed) return SNPGPU_E_IO;
        if (layout == SNPGPU_TSV_PAIRWISE) o.put("Seq1\tSeq2\tDistance\n", 19);           // distance.py:100-105
        else {                                                  // distance.py:107-114
            for (uint32_t j = 0; j < n; ++j) { o.put('\t'); o.put(ids + id_off[j], (size_t)(id_off[j + 1] - id_off[j])); }
            if (n == 0) o.put('\t');                            // '\t%s\n' % '\t'.join([])
            o.put('\n');
        }
        format_rows(o, layout, ids, id_off, n, matrix, row_stride, 0, n);
        return o.finish();
    }
    // ---- sizes ----
    const uint64_t names_total = id_off[n] - id_off[0];
    std::vector<uint64_t> block_bytes(T, 0);
    auto block = [&](unsigned t, uint32_t &r0, uint32_t &r1) { r0 = (uint32_t)((uint64_t)n * t / T); r1 = (uint32_t)((uint64_t)n * (t + 1) / T); };
    auto size_rows = [&](unsigned t) {
        uint32_t r0, r1;
        block(t, r0, r1);
        uint64_t total = 0;
        for (uint32_t i = r0; i < r1; ++i) {
            const int32_t *row = matrix + (size_t)i * row_stride;
            uint64_t d = 0;
            for (uint32_t j = 0; j < n; ++j) d += digits_i32(row[j]);
            const uint64_t li = id_off[i + 1] - id_off[i];
            total += layout == SNPGPU_TSV_PAIRWISE ? (uint64_t)n * (li + 3) + names_total + d      // n lines: id_i \t id_j \t d \n
                                                   : li + (uint64_t)n + d + 1;                      // id_i (\t d) x n \n
        }
        block_bytes[t] = total;
    };
    {
        std::vector<std::thread> th;
        for (unsigned t = 1; t < T; ++t) th.emplace_back(size_rows, t);
        size_rows(0);
        for (auto &x : th) x.join();
    }
    const uint64_t header = layout == SNPGPU_TSV_PAIRWISE ? 19 : names_total + n + 1;
    std::vector<uint64_t> at(T + 1, header);
    for (unsigned t = 0; t < T; ++t) at[t + 1] = at[t] + block_bytes[t];
    const int fd = open(path, O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0666);
    if (fd < 0) return SNPGPU_E_IO;
    bool failed = ftruncate(fd, (off_t)at[T]) != 0;
    {
        RangeOut h(fd, 0);
        if (layout == SNPGPU_TSV_PAIRWISE) h.put("Seq1\tSeq2\tDistance\n", 19);
        else {
            for (uint32_t j = 0; j < n; ++j) { h.put('\t'); h.put(ids + id_off[j], (size_t)(id_off[j + 1] - id_off[j])); }
            h.put('\n');
        }
        h.flush();
        failed = failed || h.failed || h.at != header;
    }
    std::vector<uint8_t> bad(T, 0);
    auto write_rows = [&](unsigned t) {
        uint32_t r0, r1;
        block(t, r0, r1);
        RangeOut o(fd, at[t]);
        format_rows(o, layout, ids, id_off, n, matrix, row_stride, r0, r1);
        o.flush();
        bad[t] = o.failed || o.at != at[t + 1];
    };
    if (!failed) {
        std::vector<std::thread> th;
        for (unsigned t = 1; t < T; ++t) th.emplace_back(write_rows, t);
        write_rows(0);
        for (auto &x : th) x.join();
        for (unsigned t = 0; t < T; ++t) failed = failed || bad[t];
    }
    if (close(fd) != 0) failed = true;
    return failed ? SNPGPU_E_IO : SNPGPU_OK;
}

// ---- close pairs and clusters (additive: the rows of distance.py:93-106 under a threshold, and their single-linkage groups) ----
namespace {

// The thread scheme of snpgpu_write_distance_tsv for any text of n independent row blocks: header(sink) writes header_bytes
// bytes, size_rows(r0, r1) is the byte length of the rows [r0, r1), format_rows_of(sink, r0, r1) writes them.  `work`: the
// number of values the file holds (below 2^22 one thread writes it with plain write() calls).  `values_before`: null when every
// row holds the same number of values, else n + 1 rising counts (a CSR's row offsets): the blocks then hold equal shares of the
// values, not of the rows, so that a few dense rows do not leave one thread with the whole file (a single row is never split).
template <typename Head, typename Size, typename Format>
int write_row_blocks(const char *path, uint32_t n, uint64_t work, const uint64_t *values_before, uint64_t header_bytes, Head header, Size size_rows,
                     Format format_rows_of) {
    unsigned T = snpgpu_writer_threads(0);
    if (work < ((uint64_t)1 << 22)) T = 1;
    if (T > n) T = n ? n : 1;
    if (T <= 1) {
        FileOut o(path);
        if (o.failed) return SNPGPU_E_IO;
        header(o);
        format_rows_of(o, 0u, n);
        return o.finish();
    }
    std::vector<uint64_t> block_bytes(T, 0);
    auto first_row = [&](unsigned t) -> uint32_t {
        if (t >= T) return n;
        if (!values_before) return (uint32_t)((uint64_t)n * t / T);
        const uint64_t want = (uint64_t)((unsigned __int128)work * t / T);          // the first row that starts at or behind this share
        return (uint32_t)(std::lower_bound(values_before, values_before + n, want) - values_before);
    };
    auto block = [&](unsigned t, uint32_t &r0, uint32_t &r1) { r0 = first_row(t); r1 = first_row(t + 1); };
    auto size_block = [&](unsigned t) { uint32_t r0, r1; block(t, r0, r1); block_bytes[t] = size_rows(r0, r1); };
    {
        std::vector<std::thread> th;
        for (unsigned t = 1; t < T; ++t) th.emplace_back(size_block, t);
        size_block(0);
        for (auto &x : th) x.join();
    }
    std::vector<uint64_t> at(T + 1, header_bytes);
    for (unsigned t = 0; t < T; ++t) at[t + 1] = at[t] + block_bytes[t];
    const int fd = open(path, O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0666);
    if (fd < 0) return SNPGPU_E_IO;
    bool failed = ftruncate(fd, (off_t)at[T]) != 0;
    {
        RangeOut h(fd, 0);
        header(h);
        h.flush();
        failed = failed || h.failed || h.at != header_bytes;
    }
    std::vector<uint8_t> bad(T, 0);
    auto write_block = [&](unsigned t) {
        uint32_t r0, r1;
        block(t, r0, r1);
        RangeOut o(fd, at[t]);
        format_rows_of(o, r0, r1);
        o.flush();
        bad[t] = o.failed || o.at != at[t + 1];
    };
    if (!failed) {
        std::vector<std::thread> th;
        for (unsigned t = 1; t < T; ++t) th.emplace_back(write_block, t);
        write_block(0);
        for (auto &x : th) x.join();
        for (unsigned t = 0; t < T; ++t) failed = failed || bad[t];
    }
    if (close(fd) != 0) failed = true;
    return failed ? SNPGPU_E_IO : SNPGPU_OK;
}

}  // namespace

extern "C" int snpgpu_write_close_pairs_tsv(const char *path, const char *ids, const uint64_t *id_off, uint32_t n, const uint64_t *row_off,
                                            const uint32_t *col, const int32_t *dist) {
    if (!path || (n && (!ids || !id_off || !row_off))) return SNPGPU_E_ARG;
    const uint64_t n_edges = n ? row_off[n] : 0;
    if (n && (row_off[0] != 0 || (n_edges && (!col || !dist)))) return SNPGPU_E_ARG;
    for (uint32_t i = 0; i < n; ++i)
        if (row_off[i] > row_off[i + 1]) return SNPGPU_E_ARG;
    for (uint64_t e = 0; e < n_edges; ++e)
        if (col[e] >= n) return SNPGPU_E_ARG;
    auto len = [&](uint32_t i) { return id_off[i + 1] - id_off[i]; };
    auto header = [&](auto &o) { o.put("Seq1\tSeq2\tDistance\n", 19); };                          // distance.py:100
    auto size_rows = [&](uint32_t r0, uint32_t r1) {
        uint64_t total = 0;
        for (uint32_t i = r0; i < r1; ++i)
            for (uint64_t e = row_off[i]; e < row_off[i + 1]; ++e) total += len(i) + len(col[e]) + digits_i32(dist[e]) + 3;
        return total;
    };
    auto format = [&](auto &o, uint32_t r0, uint32_t r1) {
        for (uint32_t i = r0; i < r1 && !o.failed; ++i)
            for (uint64_t e = row_off[i]; e < row_off[i + 1]; ++e) {                             // "%s\t%s\t%i\n" of distance.py:105-106
                o.put(ids + id_off[i], (size_t)len(i)); o.put('\t');
                o.put(ids + id_off[col[e]], (size_t)len(col[e])); o.put('\t');
                o.put_i32(dist[e]); o.put('\n');
            }
    };
    return write_row_blocks(path, n, n_edges, row_off, 19, header, size_rows, format);
}

// The nearest-neighbour file (csrc/nearest.hip): the rows of a CSR over the queries whose columns name database samples.
extern "C" int snpgpu_write_nearest_tsv(const char *path, const char *q_ids, const uint64_t *q_id_off, uint32_t q, const char *db_ids,
                                        const uint64_t *db_id_off, uint32_t n, const uint64_t *row_off, const uint32_t *col, const int32_t *dist) {
    if (!path || (q && (!q_ids || !q_id_off || !row_off))) return SNPGPU_E_ARG;
    const uint64_t n_entries = q ? row_off[q] : 0;
    if (q && (row_off[0] != 0 || (n_entries && (!col || !dist || !db_ids || !db_id_off)))) return SNPGPU_E_ARG;
    for (uint32_t i = 0; i < q; ++i)
        if (row_off[i] > row_off[i + 1]) return SNPGPU_E_ARG;
    for (uint64_t e = 0; e < n_entries; ++e)
        if (col[e] >= n) return SNPGPU_E_ARG;
    auto q_len = [&](uint32_t i) { return q_id_off[i + 1] - q_id_off[i]; };
    auto db_len = [&](uint32_t j) { return db_id_off[j + 1] - db_id_off[j]; };
    auto header = [&](auto &o) { o.put("Seq1\tSeq2\tDistance\n", 19); };
    auto size_rows = [&](uint32_t r0, uint32_t r1) {
        uint64_t total = 0;
        for (uint32_t i = r0; i < r1; ++i)
            for (uint64_t e = row_off[i]; e < row_off[i + 1]; ++e) total += q_len(i) + db_len(col[e]) + digits_i32(dist[e]) + 3;
        return total;
    };
    auto format = [&](auto &o, uint32_t r0, uint32_t r1) {
        for (uint32_t i = r0; i < r1 && !o.failed; ++i)
            for (uint64_t e = row_off[i]; e < row_off[i + 1]; ++e) {
                o.put(q_ids + q_id_off[i], (size_t)q_len(i)); o.put('\t');
                o.put(db_ids + db_id_off[col[e]], (size_t)db_len(col[e])); o.put('\t');
                o.put_i32(dist[e]); o.put('\n');
            }
    };
    return write_row_blocks(path, q, n_entries, row_off, 19, header, size_rows, format);
}

// Pair lists with their compared-site counts (csrc/compared.hip): the rows of a close-pairs, tree or nearest file with a fourth
// column; a[] names ids of the first table, b[] of the second.
extern "C" int snpgpu_write_pair_rows_tsv(const char *path, const char *a_ids, const uint64_t *a_id_off, uint32_t n_a, const char *b_ids,
                                          const uint64_t *b_id_off, uint32_t n_b, const uint32_t *a, const uint32_t *b, const int32_t *dist,
                                          const int32_t *compared, uint64_t n_rows) {
    if (!path || n_rows >> 32 || (n_rows && (!a || !b || !dist || !compared || !a_ids || !a_id_off || !b_ids || !b_id_off))) return SNPGPU_E_ARG;
    for (uint64_t p = 0; p < n_rows; ++p)
        if (a[p] >= n_a || b[p] >= n_b) return SNPGPU_E_ARG;
    auto a_len = [&](uint32_t i) { return a_id_off[i + 1] - a_id_off[i]; };
    auto b_len = [&](uint32_t j) { return b_id_off[j + 1] - b_id_off[j]; };
    auto header = [&](auto &o) { o.put("Seq1\tSeq2\tDistance\tCompared\n", 28); };
    auto size_rows = [&](uint32_t p0, uint32_t p1) {
        uint64_t total = 0;
        for (uint32_t p = p0; p < p1; ++p) total += a_len(a[p]) + b_len(b[p]) + digits_i32(dist[p]) + digits_i32(compared[p]) + 4;
        return total;
    };
    auto format = [&](auto &o, uint32_t p0, uint32_t p1) {
        for (uint32_t p = p0; p < p1 && !o.failed; ++p) {
            o.put(a_ids + a_id_off[a[p]], (size_t)a_len(a[p])); o.put('\t');
            o.put(b_ids + b_id_off[b[p]], (size_t)b_len(b[p])); o.put('\t');
            o.put_i32(dist[p]); o.put('\t');
            o.put_i32(compared[p]); o.put('\n');
        }
    };
    return write_row_blocks(path, (uint32_t)n_rows, n_rows, nullptr, 28, header, size_rows, format);
}

extern "C" int snpgpu_write_clusters_tsv(const char *path, const char *ids, const uint64_t *id_off, uint32_t n, const int32_t *thresholds,
                                         uint32_t n_thresholds, const uint32_t *numbers) {
    const uint32_t k = n_thresholds;
    if (!path || (k && !thresholds) || (n && (!ids || !id_off || (k && !numbers)))) return SNPGPU_E_ARG;
    uint64_t header_bytes = 3 + (k ? k : 1);                        // "Id\t", k - 1 separators, "\n"
    for (uint32_t t = 0; t < k; ++t) header_bytes += digits_i32(thresholds[t]);
    auto header = [&](auto &o) {
        o.put("Id\t", 3);
        for (uint32_t t = 0; t < k; ++t) { if (t) o.put('\t'); o.put_i32(thresholds[t]); }
        o.put('\n');
    };
    auto size_rows = [&](uint32_t r0, uint32_t r1) {
        uint64_t total = 0;
        for (uint32_t i = r0; i < r1; ++i) {
            total += id_off[i + 1] - id_off[i] + k + 1;
            for (uint32_t t = 0; t < k; ++t) total += digits_i32((int32_t)numbers[(size_t)t * n + i]);
        }
        return total;
    };
    auto format = [&](auto &o, uint32_t r0, uint32_t r1) {
        for (uint32_t i = r0; i < r1 && !o.failed; ++i) {
            o.put(ids + id_off[i], (size_t)(id_off[i + 1] - id_off[i]));
            for (uint32_t t = 0; t < k; ++t) { o.put('\t'); o.put_i32((int32_t)numbers[(size_t)t * n + i]); }
            o.put('\n');
        }
    };
    return write_row_blocks(path, n, (uint64_t)n * k, nullptr, header_bytes, header, size_rows, format);
}

// ---- minimum spanning tree and dendrogram (additive: the tree of csrc/mst.hip as text) ----
namespace {
// a Newick leaf: the id as it is when it is [A-Za-z0-9.|-]+, else in single quotes with every ' doubled
template <typename Sink>
inline void put_newick_label(Sink &o, const char *s, size_t len) {
    bool bare = len > 0;
    for (size_t k = 0; k < len && bare; ++k) {
        const unsigned char c = (unsigned char)s[k];
        bare = (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z') || (c >= '0' && c <= '9') || c == '.' || c == '|' || c == '-';
    }
    if (bare) { o.put(s, len); return; }
    o.put('\'');
    for (size_t k = 0; k < len; ++k) { if (s[k] == '\'') o.put('\''); o.put(s[k]); }
    o.put('\'');
}
}  // namespace
extern "C" int snpgpu_write_mst_tsv(const char *path, const char *ids, const uint64_t *id_off, uint32_t n, const uint32_t *u, const uint32_t *v,
                                    const int32_t *dist, uint32_t n_edges) {
    if (!path || (n && (!ids || !id_off)) || (n_edges && (!u || !v || !dist))) return SNPGPU_E_ARG;
    for (uint32_t e = 0; e < n_edges; ++e)
        if (u[e] >= n || v[e] >= n) return SNPGPU_E_ARG;
    FileOut o(path);
    if (o.failed) return SNPGPU_E_IO;
    o.put("Seq1\tSeq2\tDistance\n", 19);
    for (uint32_t e = 0; e < n_edges && !o.failed; ++e) {
        o.put(ids + id_off[u[e]], (size_t)(id_off[u[e] + 1] - id_off[u[e]])); o.put('\t');
        o.put(ids + id_off[v[e]], (size_t)(id_off[v[e] + 1] - id_off[v[e]])); o.put('\t');
        o.put_i32(dist[e]); o.put('\n');
    }
    return o.finish();
}

// Newick, one line: the edges in their order join the groups of their ends under a node of height d / 2.  Node k < n is leaf k,
// node n + e the join of edge e.  Written with an explicit stack: a chain of 10 000 nested joins is an ordinary tree here.
extern "C" int snpgpu_write_dendrogram_newick(const char *path, const char *ids, const uint64_t *id_off, uint32_t n, const uint32_t *u, const uint32_t *v,
                                              const int32_t *dist, uint32_t n_edges) {
    if (!path || (n && (!ids || !id_off)) || (n_edges && (!u || !v || !dist))) return SNPGPU_E_ARG;
    if (n_edges != (n ? n - 1 : 0)) return SNPGPU_E_ARG;
    std::vector<uint32_t> parent(n), top(n), least(n), child((size_t)n_edges * 2);   // union-find; per set root: its node and its smallest sample
    for (uint32_t i = 0; i < n; ++i) parent[i] = top[i] = least[i] = i;
    auto find = [&](uint32_t x) {
        while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
        return x;
    };
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
        parent[b] = a;
        top[a] = n + e;
    }
    FileOut o(path);
    if (o.failed) return SNPGPU_E_IO;
    auto d_of = [&](uint32_t node) -> int64_t { return node < n ? 0 : (int64_t)dist[node - n]; };
    auto label = [&](uint32_t i) { put_newick_label(o, ids + id_off[i], (size_t)(id_off[i + 1] - id_off[i])); };
    auto length = [&](int64_t twice) {                               // ":" and half of d_parent - d_child, never through a float
        o.put(':');
        o.put_i32((int32_t)(twice / 2));
        if (twice & 1) o.put(".5", 2);
    };
    if (n) {
        struct Frame { uint32_t node, up, state; };                  // up: the parent node (or itself at the root); state: children written
        std::vector<Frame> stack;
        const uint32_t root = n + n_edges - 1;                       // (n == 1: leaf 0)
        stack.push_back({n_edges ? root : 0u, n_edges ? root : 0u, 0u});
        while (!stack.empty() && !o.failed) {
            Frame &f = stack.back();
            if (f.node < n) {
                label(f.node);
                if (f.up != f.node) length(d_of(f.up));
                stack.pop_back();
                continue;
            }
            const uint32_t e = f.node - n;
            if (f.state == 0) { o.put('('); f.state = 1; const uint32_t c = child[2 * (size_t)e]; const uint32_t me = f.node; stack.push_back({c, me, 0u}); continue; }
            if (f.state == 1) { o.put(','); f.state = 2; const uint32_t c = child[2 * (size_t)e + 1]; const uint32_t me = f.node; stack.push_back({c, me, 0u}); continue; }
            o.put(')');
            if (f.up != f.node) length(d_of(f.up) - d_of(f.node));
            stack.pop_back();
        }
    }
    o.put(";\n", 2);
    return o.finish();
}

// ---- the differing sites of pairs (additive: the entries of csrc/pair_sites.hip as text) ----
namespace {
inline uint32_t digits_u64(uint64_t u) {
    uint32_t k = 1;
    while (u >= 10) { u /= 10; ++k; }
    return k;
}
template <typename Sink>
inline void put_u64(Sink &o, uint64_t u) {
    char tmp[20];
    int k = 20;
    do { tmp[--k] = (char)('0' + u % 10); u /= 10; } while (u);
    o.put(tmp + k, (size_t)(20 - k));
}
}  // namespace

// One row per entry, pair by pair in the order given: the two ids, the column (1-based) — or, with a site table, the contig name
// and position of the column —, and the two bases with their case.  The table is the caller's: chrom_of_site / pos_of_site hold
// one entry per column of the matrix and every `site` lies below their length (not checked here: the writer is not told it).
extern "C" int snpgpu_write_pair_sites_tsv(const char *path, const char *ids, const uint64_t *id_off, uint32_t n, const uint32_t *a, const uint32_t *b,
                                           uint64_t n_pairs, const uint64_t *pair_off, const uint32_t *site, const uint8_t *bases, const char *chrom_names,
                                           const uint64_t *chrom_off, const uint32_t *chrom_of_site, const uint64_t *pos_of_site) {
    if (!path || (n && (!ids || !id_off)) || n_pairs >> 32 || (n_pairs && (!a || !b || !pair_off))) return SNPGPU_E_ARG;
    const bool table = chrom_names || chrom_off || chrom_of_site || pos_of_site;
    if (table && (!chrom_off || !chrom_of_site || !pos_of_site)) return SNPGPU_E_ARG;
    const uint64_t n_entries = n_pairs ? pair_off[n_pairs] : 0;
    if (n_pairs && (pair_off[0] != 0 || (n_entries && (!site || !bases)))) return SNPGPU_E_ARG;
    for (uint64_t p = 0; p < n_pairs; ++p)
        if (pair_off[p] > pair_off[p + 1] || a[p] >= n || b[p] >= n) return SNPGPU_E_ARG;
    if (table && n_entries && !chrom_names) return SNPGPU_E_ARG;
    auto len = [&](uint32_t i) { return id_off[i + 1] - id_off[i]; };
    auto chrom_len = [&](uint32_t s) { const uint32_t c = chrom_of_site[s]; return chrom_off[c + 1] - chrom_off[c]; };
    const uint64_t header_bytes = table ? 32 : 27;
    auto header = [&](auto &o) {
        if (table) o.put("Seq1\tSeq2\tChrom\tPos\tBase1\tBase2\n", 32);
        else o.put("Seq1\tSeq2\tSite\tBase1\tBase2\n", 27);
    };
    auto size_rows = [&](uint32_t p0, uint32_t p1) {
        uint64_t total = 0;
        for (uint32_t p = p0; p < p1; ++p) {
            const uint64_t names = len(a[p]) + len(b[p]);
            for (uint64_t e = pair_off[p]; e < pair_off[p + 1]; ++e)
                total += names + (table ? chrom_len(site[e]) + digits_u64(pos_of_site[site[e]]) + 8 : digits_u64((uint64_t)site[e] + 1) + 7);
        }
        return total;
    };
    auto format = [&](auto &o, uint32_t p0, uint32_t p1) {
        for (uint32_t p = p0; p < p1 && !o.failed; ++p)
            for (uint64_t e = pair_off[p]; e < pair_off[p + 1]; ++e) {
                const uint32_t s = site[e];
                o.put(ids + id_off[a[p]], (size_t)len(a[p])); o.put('\t');
                o.put(ids + id_off[b[p]], (size_t)len(b[p])); o.put('\t');
                if (table) {
                    o.put(chrom_names + chrom_off[chrom_of_site[s]], (size_t)chrom_len(s)); o.put('\t');
                    put_u64(o, pos_of_site[s]);
                } else {
                    put_u64(o, (uint64_t)s + 1);
                }
                o.put('\t'); o.put("ACGTacgt"[bases[e] & 7]);
                o.put('\t'); o.put("ACGTacgt"[(bases[e] >> 4) & 7]);
                o.put('\n');
            }
    };
    return write_row_blocks(path, (uint32_t)n_pairs, n_entries, pair_off, header_bytes, header, size_rows, format);
}

// ---- per-site allele counts and cluster-defining SNPs (additive: the arrays of csrc/cluster_snps.hip as text) ----
namespace {
struct SiteTable {
    const char *names;
    const uint64_t *off;
    const uint32_t *chrom_of;
    const uint64_t *pos_of;
    bool given, ok;
    SiteTable(const char *n, const uint64_t *o, const uint32_t *c, const uint64_t *p) : names(n), off(o), chrom_of(c), pos_of(p) {
        given = n || o || c || p;
        ok = !given || (o && c && p);
    }
    // the column as the files name it: its 1-based number, or contig name and position
    void put(FileOut &o, uint32_t s) const {
        if (!given) { put_u64(o, (uint64_t)s + 1); return; }
        const uint32_t c = chrom_of[s];
        o.put(names + off[c], (size_t)(off[c + 1] - off[c])); o.put('\t');
        put_u64(o, pos_of[s]);
    }
};
}  // namespace

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
    if (table.given) o.put("Chrom\tPos\tA\tC\tG\tT\tOther\n", 24);
    else o.put("Site\tA\tC\tG\tT\tOther\n", 19);
    for (uint32_t s = 0; s < n_sites && !o.failed; ++s) {
        table.put(o, s);
        uint64_t sum = 0;
        for (int b = 0; b < 4; ++b) {
            o.put('\t');
            put_u64(o, (uint64_t)counts[4 * (size_t)s + b]);
            sum += (uint64_t)counts[4 * (size_t)s + b];
        }
        o.put('\t');
        put_u64(o, n_rows - sum);
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
    if (table.given) o.put("Threshold\tCluster\tChrom\tPos\tBase\tMembers\tSize\n", 46);
    else o.put("Threshold\tCluster\tSite\tBase\tMembers\tSize\n", 41);
    o_off = 0;
    for (uint32_t t = 0; t < n_labellings; ++t) {
        for (uint32_t c = 0; c < n_clusters[t] && !o.failed; ++c)
            for (uint64_t e = cluster_off[o_off + c]; e < cluster_off[o_off + c + 1]; ++e) {
                o.put_i32(thresholds[t]); o.put('\t');
                put_u64(o, (uint64_t)c + 1); o.put('\t');
                table.put(o, site[e]); o.put('\t');
                o.put("ACGT"[base[e]]); o.put('\t');
                put_u64(o, members[e]); o.put('\t');
                put_u64(o, sizes[o_size + c]); o.put('\n');
            }
        o_off += (size_t)n_clusters[t] + 1;
        o_size += n_clusters[t];
    }
    return o.finish();
}

// ---- complete- and average-linkage trees (additive: the merges of csrc/linkage.hip as text; the arithmetic is linkage_host.h) ----
namespace {
// millionths as the integer part and, when the fraction is not zero, "." and its six digits without trailing zeros
inline void put_millionths_short(FileOut &o, uint64_t v) {
    put_u64(o, v / 1000000u);
    uint32_t frac = (uint32_t)(v % 1000000u);
    if (!frac) return;
    char d[7] = {'.', 0, 0, 0, 0, 0, 0};
    for (int k = 6; k >= 1; --k) { d[k] = (char)('0' + frac % 10); frac /= 10; }
    size_t len = 7;
    while (d[len - 1] == '0') --len;
    o.put(d, len);
}
}  // namespace

extern "C" int snpgpu_write_linkage_tsv(const char *path, const char *ids, const uint64_t *id_off, uint32_t n, int kind, const uint32_t *a, const uint32_t *b,
                                        const uint32_t *size_a, const uint32_t *size_b, const uint64_t *num, uint32_t n_merges) {
    if (!path || (n && (!ids || !id_off)) || !lnk_merges_ok(n, kind, a, b, size_a, size_b, num, n_merges, false, kind == SNPGPU_LINKAGE_AVERAGE)) return SNPGPU_E_ARG;
    FileOut o(path);
    if (o.failed) return SNPGPU_E_IO;
    o.put("Seq1\tSeq2\tSize1\tSize2\tDistance\n", 31);
    for (uint32_t e = 0; e < n_merges && !o.failed; ++e) {
        o.put(ids + id_off[a[e]], (size_t)(id_off[a[e] + 1] - id_off[a[e]])); o.put('\t');
        o.put(ids + id_off[b[e]], (size_t)(id_off[b[e] + 1] - id_off[b[e]])); o.put('\t');
        put_u64(o, size_a[e]); o.put('\t');
        put_u64(o, size_b[e]); o.put('\t');
        if (kind == SNPGPU_LINKAGE_COMPLETE) {
            put_u64(o, num[e]);
        } else {                                                     // S / (sa sb), half up, exactly six decimals
            const uint64_t q = lnk_average_millionths(num[e], size_a[e], size_b[e]);
            char d[7] = {'.', 0, 0, 0, 0, 0, 0};
            uint32_t frac = (uint32_t)(q % 1000000u);
            for (int k = 6; k >= 1; --k) { d[k] = (char)('0' + frac % 10); frac /= 10; }
            put_u64(o, q / 1000000u);
            o.put(d, 7);
        }
        o.put('\n');
    }
    return o.finish();
}

// Newick, one line, in the grammar of snpgpu_write_dendrogram_newick.  Node k < n is leaf k, node n + e the join of merge e; a
// cluster's node is looked up by its id, which the merge names.  Heights in integer millionths, explicit stack.
extern "C" int snpgpu_write_linkage_newick(const char *path, const char *ids, const uint64_t *id_off, uint32_t n, int kind, const uint32_t *a, const uint32_t *b,
                                           const uint32_t *size_a, const uint32_t *size_b, const uint64_t *num, uint32_t n_merges) {
    if (!path || (n && (!ids || !id_off)) || !lnk_merges_ok(n, kind, a, b, size_a, size_b, num, n_merges, true, true)) return SNPGPU_E_ARG;
    std::vector<uint32_t> top(n), child((size_t)n_merges * 2);
    std::vector<uint64_t> height(n_merges);
    for (uint32_t i = 0; i < n; ++i) top[i] = i;
    auto h_of = [&](uint32_t node) -> uint64_t { return node < n ? 0 : height[node - n]; };
    for (uint32_t e = 0; e < n_merges; ++e) {
        height[e] = lnk_height(kind, num[e], size_a[e], size_b[e]);
        if (height[e] < h_of(top[a[e]]) || height[e] < h_of(top[b[e]])) return SNPGPU_E_ARG;      // a child above its parent: not this linkage's tree
        child[2 * (size_t)e] = top[a[e]];                            // a < b: the child with the smaller sample first
        child[2 * (size_t)e + 1] = top[b[e]];
        top[a[e]] = n + e;
    }
    FileOut o(path);
    if (o.failed) return SNPGPU_E_IO;
    auto label = [&](uint32_t i) { put_newick_label(o, ids + id_off[i], (size_t)(id_off[i + 1] - id_off[i])); };
    if (n) {
        struct Frame { uint32_t node, up, state; };                  // up: the parent node (or itself at the root); state: children written
        std::vector<Frame> stack;
        const uint32_t root = n_merges ? n + n_merges - 1 : 0u;      // the last merge is the root: every other cluster has retired
        stack.push_back({root, root, 0u});
        while (!stack.empty() && !o.failed) {
            Frame &f = stack.back();
            if (f.node < n) {
                label(f.node);
                if (f.up != f.node) { o.put(':'); put_millionths_short(o, h_of(f.up)); }
                stack.pop_back();
                continue;
            }
            const uint32_t e = f.node - n, me = f.node;
            if (f.state == 0) { o.put('('); f.state = 1; const uint32_t c = child[2 * (size_t)e]; stack.push_back({c, me, 0u}); continue; }
            if (f.state == 1) { o.put(','); f.state = 2; const uint32_t c = child[2 * (size_t)e + 1]; stack.push_back({c, me, 0u}); continue; }
            o.put(')');
            if (f.up != f.node) { o.put(':'); put_millionths_short(o, h_of(f.up) - h_of(f.node)); }
            stack.pop_back();
        }
    }
    o.put(";\n", 2);
    return o.finish();
}

// ---- neighbour-joining tree (additive: the records of csrc/nj.hip as text; the check and the writer are nj_host.h) ----
extern "C" int snpgpu_write_nj_newick(const char *path, const char *ids, const uint64_t *id_off, uint32_t n, const uint32_t *a, const uint32_t *b,
                                      const int64_t *len_a, const int64_t *len_b, uint32_t n_merges, const uint32_t *star, const int64_t *star_len) {
    if (!path || (n && (!ids || !id_off)) || !nj_records_ok(n, a, b, len_a, len_b, n_merges, star, star_len)) return SNPGPU_E_ARG;
    FileOut o(path);
    if (o.failed) return SNPGPU_E_IO;
    nj_put_newick(o, ids, id_off, n, a, b, len_a, len_b, n_merges, star, star_len);
    return o.finish();
}

// ---- bootstrap support of that tree (additive: the counts of csrc/nj_bootstrap.hip as text; the checks and the writer are nj_host.h) ----
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
    FileOut o(path);
    if (o.failed) return SNPGPU_E_IO;
    o.put("Seq1\tSeq2\tSize\tSupport\tReplicates\n", 34);
    std::vector<uint32_t> size(n, 1);
    for (uint32_t e = 0; e < n_merges && !o.failed; ++e) {
        size[a[e]] += size[b[e]];
        o.put(ids + id_off[a[e]], (size_t)(id_off[a[e] + 1] - id_off[a[e]])); o.put('\t');
        o.put(ids + id_off[b[e]], (size_t)(id_off[b[e] + 1] - id_off[b[e]])); o.put('\t');
        put_u64(o, size[a[e]]); o.put('\t');
        put_u64(o, support[e]); o.put('\t');
        put_u64(o, replicates); o.put('\n');
    }
    return o.finish();
}
