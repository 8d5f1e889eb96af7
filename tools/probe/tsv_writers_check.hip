// The host writers of the close-pairs and clusters files (csrc/tsv_out.hip: snpgpu_write_close_pairs_tsv,
// snpgpu_write_clusters_tsv) as a stand-alone program, so that they can be built with AddressSanitizer and
// UndefinedBehaviorSanitizer on the host side and a read past an id, an offset or a CSR array shows up as a report:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fno-gpu-sanitize -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/probe/tsv_writers_check.hip snp_pipeline_amd/csrc/tsv_out.hip \
//         snp_pipeline_amd/csrc/host_budget.hip -lpthread -o check
//   ./check DIR
//
// Every input array lies in a heap block of exactly its size.  Cases: no ids; one id; ids of 1 and of 300 bytes; 10^5 rows with
// enough values (over 2^22) that the writers take their threaded route, evenly spread and with nearly all of them in 50 rows.  Each file is compared with the text the program builds
// itself ("%s\t%s\t%i\n" rows of distance.py:105-106 under a header; "Id" and thresholds, then id and numbers).  It uses no HIP
// call and needs no device.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/snpgpu.h"

template <typename T>
struct Exact {                                  // a heap block of exactly n elements (one byte when n == 0)
    T *p;
    explicit Exact(const std::vector<T> &v) : p((T *)malloc(v.size() ? v.size() * sizeof(T) : 1)) {
        if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    }
    ~Exact() { free(p); }
};

static bool same_as_file(const std::string &path, const std::string &want) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    std::string got;
    char buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) got.append(buf, n);
    fclose(f);
    return got == want;
}

struct Case {
    std::vector<std::string> ids;
    std::vector<uint64_t> row_off;              // n + 1
    std::vector<uint32_t> col;
    std::vector<int32_t> dist;
    std::vector<int32_t> thresholds;
    std::vector<uint32_t> numbers;              // [k][n]
};

static int run(const std::string &dir, const char *name, const Case &c) {
    const uint32_t n = (uint32_t)c.ids.size(), k = (uint32_t)c.thresholds.size();
    std::vector<char> blob;
    std::vector<uint64_t> id_off(1, 0);
    for (const auto &s : c.ids) { blob.insert(blob.end(), s.begin(), s.end()); id_off.push_back(blob.size()); }
    Exact<char> x_blob(blob);
    Exact<uint64_t> x_id_off(id_off), x_row_off(c.row_off);
    Exact<uint32_t> x_col(c.col), x_numbers(c.numbers);
    Exact<int32_t> x_dist(c.dist), x_thr(c.thresholds);
    int failures = 0;

    std::string want = "Seq1\tSeq2\tDistance\n";
    for (uint32_t i = 0; i < n; ++i)
        for (uint64_t e = c.row_off[i]; e < c.row_off[i + 1]; ++e) want += c.ids[i] + "\t" + c.ids[c.col[e]] + "\t" + std::to_string(c.dist[e]) + "\n";
    const std::string p1 = dir + "/" + name + ".close.tsv";
    int rc = snpgpu_write_close_pairs_tsv(p1.c_str(), x_blob.p, x_id_off.p, n, x_row_off.p, x_col.p, x_dist.p);
    if (rc != SNPGPU_OK || !same_as_file(p1, want)) { fprintf(stderr, "%s: close pairs differ (rc %d)\n", name, rc); ++failures; }

    want = "Id\t";
    for (uint32_t t = 0; t < k; ++t) want += (t ? "\t" : "") + std::to_string(c.thresholds[t]);
    want += "\n";
    for (uint32_t i = 0; i < n; ++i) {
        want += c.ids[i];
        for (uint32_t t = 0; t < k; ++t) want += "\t" + std::to_string(c.numbers[(size_t)t * n + i]);
        want += "\n";
    }
    const std::string p2 = dir + "/" + name + ".clusters.tsv";
    rc = snpgpu_write_clusters_tsv(p2.c_str(), x_blob.p, x_id_off.p, n, x_thr.p, k, x_numbers.p);
    if (rc != SNPGPU_OK || !same_as_file(p2, want)) { fprintf(stderr, "%s: clusters differ (rc %d)\n", name, rc); ++failures; }

    const std::string nowhere = dir + "/no_such_directory/x.tsv";
    if (snpgpu_write_close_pairs_tsv(nowhere.c_str(), x_blob.p, x_id_off.p, n, x_row_off.p, x_col.p, x_dist.p) != SNPGPU_E_IO ||
        snpgpu_write_clusters_tsv(nowhere.c_str(), x_blob.p, x_id_off.p, n, x_thr.p, k, x_numbers.p) != SNPGPU_E_IO) {
        fprintf(stderr, "%s: a path that cannot be created is not SNPGPU_E_IO\n", name);
        ++failures;
    }
    printf("%-12s n %u, %zu entries, %u thresholds: %s\n", name, n, c.col.size(), k, failures ? "FAILED" : "ok");
    return failures;
}

// a CSR with `per_row` entries per row (the diagonal among them, columns ascending) and numbers for the thresholds
static void fill(Case &c, uint32_t per_row, const std::vector<int32_t> &thresholds) {
    const uint32_t n = (uint32_t)c.ids.size();
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(seed >> 33); };
    c.row_off.assign(1, 0);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t m = per_row < n ? per_row : n, first = i + m <= n ? i : n - m;
        for (uint32_t j = 0; j < m; ++j) {
            c.col.push_back(first + j);
            c.dist.push_back(first + j == i ? 0 : (int32_t)(next() % 3 ? next() % 100 : next() & 0x7FFFFFFF));
        }
        c.row_off.push_back(c.col.size());
    }
    c.thresholds = thresholds;
    for (size_t t = 0; t < thresholds.size(); ++t)
        for (uint32_t i = 0; i < n; ++i) c.numbers.push_back(1 + next() % (n ? n : 1));
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s DIR\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    int failures = 0;
    {
        Case c;
        fill(c, 0, {0, 5, 20});
        failures += run(dir, "empty", c);
    }
    {
        Case c;
        fill(c, 0, {});
        failures += run(dir, "empty_k0", c);
    }
    {
        Case c;
        c.ids = {"only"};
        fill(c, 1, {7});
        failures += run(dir, "one", c);
    }
    {
        Case c;
        c.ids = {"a", std::string(300, 'L'), "b", std::string(300, 'M')};
        fill(c, 3, {0, 2147483647});
        failures += run(dir, "short_long", c);
    }
    {
        Case c;
        for (uint32_t i = 0; i < 100000; ++i) c.ids.push_back("sample_" + std::to_string(i * 7919u % 100003u));
        std::vector<int32_t> thr;
        for (int32_t t = 0; t < 45; ++t) thr.push_back(t * t);
        fill(c, 45, thr);
        failures += run(dir, "rows_1e5", c);
    }
    {
        // nearly all entries in 50 of the 10^5 rows: the writer's blocks follow the entries, so most blocks hold one row or none
        Case c;
        for (uint32_t i = 0; i < 100000; ++i) c.ids.push_back("r" + std::to_string(i));
        c.row_off.assign(1, 0);
        for (uint32_t i = 0; i < 100000; ++i) {
            const bool dense = i >= 40000 && i < 40050;
            for (uint32_t j = dense ? 0 : i; j < (dense ? 90000u : i + 1); ++j) { c.col.push_back(j); c.dist.push_back((int32_t)((i + j) % 1000)); }
            c.row_off.push_back(c.col.size());
        }
        c.thresholds = {3};
        c.numbers.assign(100000, 1);
        failures += run(dir, "dense_rows", c);
    }
    printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
