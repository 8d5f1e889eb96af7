// The host writers of the minimum-spanning-tree and dendrogram files (csrc/tsv_out.hip: snpgpu_write_mst_tsv,
// snpgpu_write_dendrogram_newick) as a stand-alone program, so that they can be built with AddressSanitizer and
// UndefinedBehaviorSanitizer on the host side and a read past an id, an offset or an edge array shows up as a report:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fno-gpu-sanitize -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/probe/mst_writers_check.hip snp_pipeline_amd/csrc/tsv_out.hip \
//         snp_pipeline_amd/csrc/host_budget.hip -lpthread -o check
//   ./check DIR
//
// Every input array lies in a heap block of exactly its size.  Cases: no ids; one id (bare, and one that needs quotes); a tree of
// three with an odd and an even distance and ids with a quote, a space and an underscore; equal distances; a chain of 100 000
// nested joins (the writer must not recurse); a distance of 2^31 - 1; edge lists that are not a tree (refused).  Each file is
// compared with the text spelled out here or built by the program itself.  It uses no HIP call and needs no device.
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

struct Edge { int32_t d; uint32_t u, v; };

// rc of the Newick writer must be want_rc; on success both files must hold the given texts (an empty want_newick: built-in skip)
static int run(const std::string &dir, const char *name, const std::vector<std::string> &ids, const std::vector<Edge> &edges, int want_rc,
               const std::string &want_newick) {
    std::vector<char> blob;
    std::vector<uint64_t> id_off(1, 0);
    for (const auto &s : ids) { blob.insert(blob.end(), s.begin(), s.end()); id_off.push_back(blob.size()); }
    std::vector<uint32_t> u, v;
    std::vector<int32_t> d;
    for (const auto &e : edges) { u.push_back(e.u); v.push_back(e.v); d.push_back(e.d); }
    Exact<char> x_blob(blob);
    Exact<uint64_t> x_off(id_off);
    Exact<uint32_t> x_u(u), x_v(v);
    Exact<int32_t> x_d(d);
    const uint32_t n = (uint32_t)ids.size(), m = (uint32_t)edges.size();
    const std::string nwk = dir + "/" + name + ".nwk", tsv = dir + "/" + name + ".tsv";
    const int rc = snpgpu_write_dendrogram_newick(nwk.c_str(), x_blob.p, x_off.p, n, x_u.p, x_v.p, x_d.p, m);
    if (rc != want_rc) { fprintf(stderr, "%s: newick rc %d, wanted %d\n", name, rc, want_rc); return 1; }
    if (rc != SNPGPU_OK) return 0;
    if (!same_as_file(nwk, want_newick)) { fprintf(stderr, "%s: newick text differs\n", name); return 1; }
    std::string want_tsv = "Seq1\tSeq2\tDistance\n";
    for (const auto &e : edges) want_tsv += ids[e.u] + "\t" + ids[e.v] + "\t" + std::to_string(e.d) + "\n";
    if (snpgpu_write_mst_tsv(tsv.c_str(), x_blob.p, x_off.p, n, x_u.p, x_v.p, x_d.p, m) != SNPGPU_OK || !same_as_file(tsv, want_tsv)) {
        fprintf(stderr, "%s: mst text differs\n", name);
        return 1;
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s DIR\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    int bad = 0;
    bad += run(dir, "none", {}, {}, SNPGPU_OK, ";\n");
    bad += run(dir, "one", {"a"}, {}, SNPGPU_OK, "a;\n");
    bad += run(dir, "one_quoted", {"a_b"}, {}, SNPGPU_OK, "'a_b';\n");
    bad += run(dir, "empty_id", {"", "b"}, {{3, 0, 1}}, SNPGPU_OK, "('':1.5,b:1.5);\n");
    bad += run(dir, "three", {"it's", "two words", "c_d"}, {{2, 1, 2}, {7, 0, 1}}, SNPGPU_OK, "('it''s':3.5,('two words':1,'c_d':1):2.5);\n");
    bad += run(dir, "ties", {"a", "b", "c"}, {{4, 0, 1}, {4, 0, 2}}, SNPGPU_OK, "((a:2,b:2):0,c:2);\n");
    bad += run(dir, "largest", {"a", "b"}, {{2147483647, 0, 1}}, SNPGPU_OK, "(a:1073741823.5,b:1073741823.5);\n");
    bad += run(dir, "reversed_ends", {"a", "b", "c"}, {{1, 2, 1}, {2, 1, 0}}, SNPGPU_OK, "(a:1,(b:0.5,c:0.5):0.5);\n");
    bad += run(dir, "too_few", {"a", "b", "c"}, {{1, 0, 1}}, SNPGPU_E_ARG, "");
    bad += run(dir, "cycle", {"a", "b", "c"}, {{1, 0, 1}, {2, 0, 1}}, SNPGPU_E_ARG, "");
    bad += run(dir, "descending", {"a", "b", "c"}, {{2, 0, 1}, {1, 1, 2}}, SNPGPU_E_ARG, "");
    bad += run(dir, "past_n", {"a", "b", "c"}, {{1, 0, 1}, {2, 1, 3}}, SNPGPU_E_ARG, "");
    bad += run(dir, "loop", {"a", "b", "c"}, {{1, 0, 1}, {2, 2, 2}}, SNPGPU_E_ARG, "");
    {
        const uint32_t n = 100000;
        std::vector<std::string> ids;
        std::vector<Edge> edges;
        for (uint32_t i = 0; i < n; ++i) ids.push_back("s" + std::to_string(i));
        for (uint32_t i = 0; i + 1 < n; ++i) edges.push_back({1, i, i + 1});
        std::string want(n - 1, '(');
        want += "s0:0.5,s1:0.5)";
        for (uint32_t i = 2; i < n; ++i) want += ":0,s" + std::to_string(i) + ":0.5)";
        bad += run(dir, "chain", ids, edges, SNPGPU_OK, want + ";\n");
    }
    if (snpgpu_write_mst_tsv((dir + "/no_such_dir/x.tsv").c_str(), "a", (const uint64_t[]){0, 1}, 1, nullptr, nullptr, nullptr, 0) != SNPGPU_E_IO) {
        fprintf(stderr, "an unwritable path is not SNPGPU_E_IO\n");
        ++bad;
    }
    printf(bad ? "FAILED: %d\n" : "ok\n", bad);
    return bad ? 1 : 0;
}
