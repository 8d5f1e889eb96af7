// The host writer of the differing-sites files (csrc/tsv_out.hip: snpgpu_write_pair_sites_tsv) as a stand-alone program, so that
// it can be built with AddressSanitizer and UndefinedBehaviorSanitizer on the host side and a read past an id, an offset, an entry
// or the site table shows up as a report:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fno-gpu-sanitize -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/probe/pair_sites_writer_check.hip snp_pipeline_amd/csrc/tsv_out.hip \
//         snp_pipeline_amd/csrc/host_budget.hip -lpthread -o check
//   ./check DIR
//
// Every input array lies in a heap block of exactly its size.  Cases: no pairs; pairs without entries; ids of 1 and of 300 bytes
// with lower-case letters; 2 000 pairs with enough entries (over 2^22) that the writer takes its threaded route, evenly spread and
// with nearly all of them in 3 pairs.  Each case is written without and with a site table and compared with the text the program
// builds itself.  It uses no HIP call and needs no device.
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
    std::vector<std::string> ids, chroms;
    uint32_t columns = 0;                       // of the matrix: the site table has this many entries
    std::vector<uint32_t> a, b;
    std::vector<uint64_t> pair_off;             // pairs + 1
    std::vector<uint32_t> site;
    std::vector<uint8_t> bases;
};

static int run(const std::string &dir, const char *name, const Case &c) {
    const uint32_t n = (uint32_t)c.ids.size();
    const uint64_t m = c.a.size();
    std::vector<char> blob, chrom_blob;
    std::vector<uint64_t> id_off(1, 0), chrom_off(1, 0), pos_of(c.columns);
    std::vector<uint32_t> chrom_of(c.columns);
    for (const auto &s : c.ids) { blob.insert(blob.end(), s.begin(), s.end()); id_off.push_back(blob.size()); }
    for (const auto &s : c.chroms) { chrom_blob.insert(chrom_blob.end(), s.begin(), s.end()); chrom_off.push_back(chrom_blob.size()); }
    for (uint32_t k = 0; k < c.columns; ++k) {
        chrom_of[k] = (uint32_t)((uint64_t)k * c.chroms.size() / c.columns);
        pos_of[k] = k % 7 == 3 ? 4000000000ull + k : 1 + (uint64_t)k * 13;
    }
    Exact<char> x_blob(blob), x_chrom_blob(chrom_blob);
    Exact<uint64_t> x_id_off(id_off), x_chrom_off(chrom_off), x_pos_of(pos_of), x_pair_off(c.pair_off);
    Exact<uint32_t> x_a(c.a), x_b(c.b), x_site(c.site), x_chrom_of(chrom_of);
    Exact<uint8_t> x_bases(c.bases);
    int failures = 0;
    for (int table = 0; table < 2; ++table) {
        std::string want = table ? "Seq1\tSeq2\tChrom\tPos\tBase1\tBase2\n" : "Seq1\tSeq2\tSite\tBase1\tBase2\n";
        for (uint64_t p = 0; p < m; ++p)
            for (uint64_t e = c.pair_off[p]; e < c.pair_off[p + 1]; ++e) {
                const uint32_t s = c.site[e];
                want += c.ids[c.a[p]] + "\t" + c.ids[c.b[p]] + "\t";
                want += table ? c.chroms[chrom_of[s]] + "\t" + std::to_string(pos_of[s]) : std::to_string((uint64_t)s + 1);
                want += "\t";
                want += "ACGTacgt"[c.bases[e] & 7];
                want += "\t";
                want += "ACGTacgt"[(c.bases[e] >> 4) & 7];
                want += "\n";
            }
        const std::string path = dir + "/" + name + (table ? ".pos.tsv" : ".site.tsv");
        const int rc = snpgpu_write_pair_sites_tsv(path.c_str(), x_blob.p, x_id_off.p, n, x_a.p, x_b.p, m, x_pair_off.p, x_site.p, x_bases.p,
                                                   table ? x_chrom_blob.p : nullptr, table ? x_chrom_off.p : nullptr, table ? x_chrom_of.p : nullptr,
                                                   table ? x_pos_of.p : nullptr);
        if (rc != SNPGPU_OK || !same_as_file(path, want)) { fprintf(stderr, "%s: the %s file differs (rc %d)\n", name, table ? "position" : "site", rc); ++failures; }
    }
    const std::string nowhere = dir + "/no_such_directory/x.tsv";
    if (snpgpu_write_pair_sites_tsv(nowhere.c_str(), x_blob.p, x_id_off.p, n, x_a.p, x_b.p, m, x_pair_off.p, x_site.p, x_bases.p, nullptr, nullptr, nullptr, nullptr) !=
        SNPGPU_E_IO) {
        fprintf(stderr, "%s: a path that cannot be created is not SNPGPU_E_IO\n", name);
        ++failures;
    }
    printf("%-12s n %u, %llu pairs, %zu entries: %s\n", name, n, (unsigned long long)m, c.site.size(), failures ? "FAILED" : "ok");
    return failures;
}

// pair p = (p % n, (p * 7 + 1) % n) with entries(p) entries at rising columns
template <typename Entries>
static void fill(Case &c, uint32_t pairs, Entries entries) {
    const uint32_t n = (uint32_t)c.ids.size();
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(seed >> 33); };
    c.pair_off.assign(1, 0);
    for (uint32_t p = 0; p < pairs; ++p) {
        c.a.push_back(p % n);
        c.b.push_back((uint32_t)(((uint64_t)p * 7 + 1) % n));
        const uint32_t k = entries(p);
        for (uint32_t j = 0; j < k; ++j) {
            c.site.push_back((uint32_t)((uint64_t)j * c.columns / k));
            c.bases.push_back((uint8_t)((next() & 7) | (next() & 7) << 4));
        }
        c.pair_off.push_back(c.site.size());
    }
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s DIR\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    int failures = 0;
    {
        Case c;
        c.pair_off.assign(1, 0);
        failures += run(dir, "empty", c);
    }
    {
        Case c;
        c.ids = {"x", "y"};
        c.chroms = {"chr"};
        c.columns = 5;
        fill(c, 4, [](uint32_t) { return 0u; });
        failures += run(dir, "no_entries", c);
    }
    {
        Case c;
        c.ids = {"a", std::string(300, 'L'), "b", std::string(300, 'M')};
        c.chroms = {"c", std::string(200, 'K')};
        c.columns = 40;
        fill(c, 9, [](uint32_t p) { return p % 3 ? 1u + p : 0u; });
        failures += run(dir, "short_long", c);
    }
    {
        Case c;
        for (uint32_t i = 0; i < 500; ++i) c.ids.push_back("sample_" + std::to_string(i * 7919u % 100003u));
        c.chroms = {"NC_000001.1", "NC_000002.1", "plasmid"};
        c.columns = 200000;
        fill(c, 2000, [](uint32_t) { return 2200u; });
        failures += run(dir, "pairs_2000", c);
    }
    {
        // nearly all entries in 3 of the 2 000 pairs: the writer's blocks follow the entries, so most blocks hold one pair or none
        Case c;
        for (uint32_t i = 0; i < 500; ++i) c.ids.push_back("r" + std::to_string(i));
        c.chroms = {"one"};
        c.columns = 2000000;
        fill(c, 2000, [](uint32_t p) { return p == 700 || p == 701 || p == 1999 ? 1500000u : p % 2; });
        failures += run(dir, "dense_pairs", c);
    }
    printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
