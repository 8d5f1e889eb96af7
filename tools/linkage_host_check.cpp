// Stand-alone check of the host code of the linkage trees, meant to be built with the host sanitizers and run on the CPU:
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Iinclude -Isnp_pipeline_amd/csrc \
//         tools/linkage_host_check.cpp snp_pipeline_amd/csrc/tsv_out.hip snp_pipeline_amd/csrc/host_budget.hip -o linkage_host_check
// It orders merge lists (lnk_sort_merges: what snpgpu_linkage_dev does last), checks and cuts them (lnk_merges_ok, lnk_cut: the body of snpgpu_linkage_cut)
// and writes both texts through snpgpu_write_linkage_tsv / snpgpu_write_linkage_newick, over random trees of 0 ... 300 samples,
// both kinds, ids that need quoting, and the lists the writers must refuse.  No GPU is touched.
#include <stdio.h>
#include <stdlib.h>
#include <unistd.h>

#include <string>
#include <vector>

#include "linkage_host.h"
#include "snpgpu.h"

namespace {

uint64_t state = 88172645463325252ull;
uint32_t rnd(uint32_t below) {
    state ^= state << 13; state ^= state >> 7; state ^= state << 17;
    return below ? (uint32_t)(state % below) : 0;
}

struct Tree {
    std::vector<uint32_t> a, b, sa, sb;
    std::vector<uint64_t> num;
};

// a random agglomeration of n samples with heights that rise
Tree random_tree(uint32_t n, int kind, uint32_t step) {
    Tree t;
    std::vector<uint32_t> live, size(n, 1);
    for (uint32_t i = 0; i < n; ++i) live.push_back(i);
    uint64_t d = 0;
    while (live.size() > 1) {
        uint32_t x = rnd((uint32_t)live.size()), y = rnd((uint32_t)live.size() - 1);
        if (y >= x) ++y;
        uint32_t lo = live[x] < live[y] ? live[x] : live[y], hi = live[x] < live[y] ? live[y] : live[x];
        d += rnd(step);
        t.a.push_back(lo); t.b.push_back(hi); t.sa.push_back(size[lo]); t.sb.push_back(size[hi]);
        t.num.push_back(kind == SNPGPU_LINKAGE_AVERAGE ? d * size[lo] * size[hi] + rnd(size[lo] * size[hi]) : d);
        if (kind == SNPGPU_LINKAGE_AVERAGE) ++d;                     // the next quotient lies above this one
        size[lo] += size[hi];
        live.erase(live.begin() + (live[x] == hi ? x : y));
    }
    return t;
}

int failures = 0;
void expect(bool ok, const char *what, uint32_t n, int kind) {
    if (!ok) { fprintf(stderr, "FAILED: %s (n = %u, kind = %d)\n", what, n, kind); ++failures; }
}

}  // namespace

int main() {
    char path[] = "/tmp/linkage_host_check_XXXXXX";
    const int fd = mkstemp(path);
    if (fd < 0) { perror("mkstemp"); return 2; }
    close(fd);
    const uint32_t sizes[] = {0, 1, 2, 3, 17, 64, 300};
    for (int kind = 0; kind < 2; ++kind)
        for (uint32_t n : sizes)
            for (uint32_t step : {1u, 3u, 2000000000u}) {
                if (kind == SNPGPU_LINKAGE_AVERAGE && step > 3 && n > 64) continue;      // (sums of such entries over 150 x 150 pairs leave 64 bits)
                Tree t = random_tree(n, kind, step);
                const uint32_t m = (uint32_t)t.a.size();
                std::string ids;
                std::vector<uint64_t> off(n + 1, 0);
                for (uint32_t i = 0; i < n; ++i) {
                    ids += i % 3 == 0 ? "it's " : i % 3 == 1 ? "plain-" : "under_";
                    ids += std::to_string(i);
                    off[i + 1] = ids.size();
                }
                // the final ordering: shuffled records come back in key order
                std::vector<LnkMerge> rec(m);
                for (uint32_t e = 0; e < m; ++e) rec[e] = {t.num[e], t.a[e], t.b[e], t.sa[e], t.sb[e]};
                for (uint32_t e = m; e > 1; --e) std::swap(rec[e - 1], rec[rnd(e)]);
                lnk_sort_merges(kind, rec);
                bool ascending = true;
                for (uint32_t e = 1; e < m; ++e) ascending = ascending && !lnk_merge_less(kind, rec[e], rec[e - 1]);
                expect(ascending, "the merges are not in key order after the sort", n, kind);
                // the cut
                const int32_t thresholds[] = {-1, 0, 1, 7, 2147483647};
                std::vector<uint32_t> numbers((size_t)5 * n + 1), counts(5);
                const bool cut_ok = lnk_merges_ok(n, kind, t.a.data(), t.b.data(), t.sa.data(), t.sb.data(), t.num.data(), m, false, false);
                if (cut_ok) lnk_cut(kind, n, t.a.data(), t.b.data(), t.sa.data(), t.sb.data(), t.num.data(), m, thresholds, 5, numbers.data(), counts.data());
                expect(cut_ok && counts[0] == n && (step > 3 || counts[4] == (n ? 1u : 0u)), "the cut", n, kind);
                for (uint32_t k = 1; k < 5; ++k) expect(counts[k] <= counts[k - 1], "a wider threshold has more clusters", n, kind);
                // the writers
                expect(snpgpu_write_linkage_tsv(path, ids.data(), off.data(), n, kind, t.a.data(), t.b.data(), t.sa.data(), t.sb.data(), t.num.data(), m) == SNPGPU_OK,
                       "snpgpu_write_linkage_tsv", n, kind);
                expect(snpgpu_write_linkage_newick(path, ids.data(), off.data(), n, kind, t.a.data(), t.b.data(), t.sa.data(), t.sb.data(), t.num.data(), m) == SNPGPU_OK,
                       "snpgpu_write_linkage_newick", n, kind);
                if (m >= 2) {                                        // what is not a tree is refused before anything is indexed with it
                    Tree bad = t;
                    bad.b[m - 1] = n + 5;
                    expect(snpgpu_write_linkage_newick(path, ids.data(), off.data(), n, kind, bad.a.data(), bad.b.data(), bad.sa.data(), bad.sb.data(), bad.num.data(), m) == SNPGPU_E_ARG,
                           "an index past n is refused", n, kind);
                    expect(!lnk_merges_ok(n, kind, bad.a.data(), bad.b.data(), bad.sa.data(), bad.sb.data(), bad.num.data(), m, false, false),
                           "the cut's check refuses an index past n", n, kind);
                    bad = t;
                    bad.sa[m - 1] += 1;
                    expect(snpgpu_write_linkage_tsv(path, ids.data(), off.data(), n, kind, bad.a.data(), bad.b.data(), bad.sa.data(), bad.sb.data(), bad.num.data(), m) == SNPGPU_E_ARG,
                           "a wrong size is refused", n, kind);
                    expect(snpgpu_write_linkage_newick(path, ids.data(), off.data(), n, kind, t.a.data(), t.b.data(), t.sa.data(), t.sb.data(), t.num.data(), m - 1) == SNPGPU_E_ARG,
                           "a list that is not the whole tree is refused", n, kind);
                    bad = t;
                    bad.num[m - 1] = ~0ull;                          // 2^64 - 1 over few pairs: its millionths leave 64 bits
                    if (kind == SNPGPU_LINKAGE_COMPLETE || (uint64_t)bad.sa[m - 1] * bad.sb[m - 1] < 1000000u)
                        expect(snpgpu_write_linkage_newick(path, ids.data(), off.data(), n, kind, bad.a.data(), bad.b.data(), bad.sa.data(), bad.sb.data(), bad.num.data(), m) == SNPGPU_E_ARG,
                               "a distance beyond 64 bits of millionths is refused", n, kind);
                }
            }
    unlink(path);
    if (failures) return 1;
    printf("linkage host check ok\n");
    return 0;
}
