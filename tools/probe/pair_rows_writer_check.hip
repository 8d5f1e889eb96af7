// The host writer of the four-column pair files (csrc/tsv_out.hip: snpgpu_write_pair_rows_tsv) as a stand-alone program, so that it
// can be built with AddressSanitizer and UndefinedBehaviorSanitizer on the host side and a read past an id, an offset or a row shows
// up as a report:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fno-gpu-sanitize -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/probe/pair_rows_writer_check.hip snp_pipeline_amd/csrc/tsv_out.hip \
//         snp_pipeline_amd/csrc/host_budget.hip -lpthread -o check
//   ./check DIR
//
// Every input array lies in a heap block of exactly its size.  Cases: no rows; two id tables with ids of 1 and of 300 bytes; one
// table given twice; 4.3 million rows (over 2^22), so that the writer takes its threaded route, with the extremes of int32 among
// the numbers; an index equal to the size of its table in either column.  Each file is compared with the text the program builds
// itself.  It uses no HIP call and needs no device.
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

struct Table {
    std::vector<char> blob;
    std::vector<uint64_t> off;
    explicit Table(const std::vector<std::string> &ids) : off(1, 0) {
        for (const auto &s : ids) { blob.insert(blob.end(), s.begin(), s.end()); off.push_back(blob.size()); }
    }
};

static int run(const std::string &dir, const char *name, const std::vector<std::string> &a_ids, const std::vector<std::string> &b_ids, uint64_t rows) {
    const uint32_t n_a = (uint32_t)a_ids.size(), n_b = (uint32_t)b_ids.size();
    std::vector<uint32_t> a, b;
    std::vector<int32_t> dist, compared;
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(seed >> 33); };
    for (uint64_t p = 0; p < rows; ++p) {
        a.push_back(next() % n_a);
        b.push_back(next() % n_b);
        dist.push_back(p % 1000 == 7 ? INT32_MIN : (int32_t)(next() % 300));
        compared.push_back(p % 1000 == 9 ? INT32_MAX : (int32_t)(next() % 200001));
    }
    const Table ta(a_ids), tb(b_ids);
    Exact<char> x_a_blob(ta.blob), x_b_blob(tb.blob);
    Exact<uint64_t> x_a_off(ta.off), x_b_off(tb.off);
    Exact<uint32_t> x_a(a), x_b(b);
    Exact<int32_t> x_dist(dist), x_compared(compared);
    std::string want = "Seq1\tSeq2\tDistance\tCompared\n";
    for (uint64_t p = 0; p < rows; ++p)
        want += a_ids[a[p]] + "\t" + b_ids[b[p]] + "\t" + std::to_string(dist[p]) + "\t" + std::to_string(compared[p]) + "\n";
    int failures = 0;
    const std::string path = dir + "/" + name + ".tsv";
    const int rc = snpgpu_write_pair_rows_tsv(path.c_str(), x_a_blob.p, x_a_off.p, n_a, x_b_blob.p, x_b_off.p, n_b, x_a.p, x_b.p, x_dist.p, x_compared.p, rows);
    if (rc != SNPGPU_OK || !same_as_file(path, want)) { fprintf(stderr, "%s: the file differs (rc %d)\n", name, rc); ++failures; }
    const std::string nowhere = dir + "/no_such_directory/x.tsv";
    if (snpgpu_write_pair_rows_tsv(nowhere.c_str(), x_a_blob.p, x_a_off.p, n_a, x_b_blob.p, x_b_off.p, n_b, x_a.p, x_b.p, x_dist.p, x_compared.p, rows) != SNPGPU_E_IO) {
        fprintf(stderr, "%s: a path that cannot be created is not SNPGPU_E_IO\n", name);
        ++failures;
    }
    if (rows) {                                 // an index equal to the size of its table, in either column: refused, nothing read behind a table
        for (int column = 0; column < 2; ++column) {
            std::vector<uint32_t> bad = column ? b : a;
            bad[rows - 1] = column ? n_b : n_a;
            Exact<uint32_t> x_bad(bad);
            const std::string refused = dir + "/" + name + ".refused.tsv";
            if (snpgpu_write_pair_rows_tsv(refused.c_str(), x_a_blob.p, x_a_off.p, n_a, x_b_blob.p, x_b_off.p, n_b, column ? x_a.p : x_bad.p, column ? x_bad.p : x_b.p,
                                           x_dist.p, x_compared.p, rows) != SNPGPU_E_ARG) {
                fprintf(stderr, "%s: an index outside table %d is not SNPGPU_E_ARG\n", name, column);
                ++failures;
            }
        }
    }
    printf("%-12s %u and %u ids, %llu rows: %s\n", name, n_a, n_b, (unsigned long long)rows, failures ? "FAILED" : "ok");
    return failures;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s DIR\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    int failures = 0;
    const std::vector<std::string> few = {"a", std::string(300, 'L'), "b"}, other = {"x", "s\xc3\xa9", std::string(300, 'M'), "y", "z"};
    std::vector<std::string> many;
    for (uint32_t i = 0; i < 500; ++i) many.push_back("sample_" + std::to_string(i * 7919u % 100003u));
    failures += run(dir, "empty", few, other, 0);
    failures += run(dir, "two_tables", few, other, 40);
    failures += run(dir, "one_table", other, other, 3000);
    failures += run(dir, "threaded", many, few, ((uint64_t)1 << 22) + 100000);
    printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
