// Stand-alone check of the host code of the neighbour-joining tree (snp_pipeline_amd/csrc/nj_host.h), meant to be built with the
// host sanitizers and run on the CPU:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Isnp_pipeline_amd/csrc tools/nj_host_check.cpp -o nj_host_check
// It builds random trees of 0 ... 2 000 samples as records (merges in round order and the star), with lengths of either sign up to
// the ends of 64 bits and ids that need quoting, checks them (nj_records_ok: what snpgpu_write_nj_newick does first), writes them
// (nj_put_newick into a string: the function that entry point writes its file with) and compares the line with the tree joined
// slot by slot as strings; the same with bootstrap support counts (nj_support_ok, nj_joins_ok, nj_percent: what
// snpgpu_write_nj_newick_support and snpgpu_write_nj_support check and write); then the records the check must refuse.
// No GPU is touched and nothing but that header is compiled in.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "nj_host.h"

namespace {

uint64_t state = 88172645463325252ull;
uint64_t rnd64() {
    state ^= state << 13; state ^= state >> 7; state ^= state << 17;
    return state;
}
uint32_t rnd(uint32_t below) { return below ? (uint32_t)(rnd64() % below) : 0; }

struct Text {
    std::string s;
    void put(char c) { s.push_back(c); }
    void put(const char *p, size_t len) { s.append(p, len); }
};

struct Records {
    std::vector<uint32_t> a, b;
    std::vector<int64_t> la, lb;
    uint32_t star[3];
    int64_t star_len[3];
};

int64_t some_length(int kind) {
    switch (kind) {
        case 0: return (int64_t)rnd(40) << NJ_FRACTION_BITS;
        case 1: return (int64_t)rnd64() >> (rnd(40) + 1);              // either sign, every magnitude
        case 2: return rnd(2) ? INT64_MAX - (int64_t)rnd(3) : INT64_MIN + (int64_t)rnd(3);
        default: return (int64_t)rnd(2000000) - 1000000;              // around zero: the rounding of the last digit
    }
}

// a random tree of n samples: n - 3 joins of two live slots, the smaller slot stays
Records random_records(uint32_t n, int kind) {
    Records r;
    std::vector<uint32_t> live;
    for (uint32_t i = 0; i < n; ++i) live.push_back(i);
    while (live.size() > 3) {
        uint32_t x = rnd((uint32_t)live.size()), y = rnd((uint32_t)live.size() - 1);
        if (y >= x) ++y;
        if (x > y) std::swap(x, y);
        r.a.push_back(live[x]); r.b.push_back(live[y]);
        r.la.push_back(some_length(kind)); r.lb.push_back(some_length(kind));
        live.erase(live.begin() + y);
    }
    for (uint32_t s = 0; s < 3; ++s) {
        const bool there = n >= 2 && s < live.size();
        r.star[s] = there ? live[s] : NJ_NONE;
        r.star_len[s] = there ? some_length(kind) : 0;
    }
    return r;
}

std::string length_text(int64_t x) {
    Text t;
    nj_put_length(t, x);
    return t.s;
}

// the text the statement gives, built the slow way: strings joined per slot
std::string expected(const std::vector<std::string> &labels, const Records &r, const std::vector<uint32_t> *support = nullptr, uint32_t replicates = 0) {
    const uint32_t n = (uint32_t)labels.size();
    if (n == 0) return ";\n";
    if (n == 1) return labels[0] + ";\n";
    std::vector<std::string> text(labels);
    for (size_t e = 0; e < r.a.size(); ++e) {
        text[r.a[e]] = "(" + text[r.a[e]] + ":" + length_text(r.la[e]) + "," + text[r.b[e]] + ":" + length_text(r.lb[e]) + ")" +
                       (support ? std::to_string((200ull * (*support)[e] + replicates) / (2ull * replicates)) : std::string());
        text[r.b[e]].clear();
    }
    std::string out = "(";
    for (uint32_t s = 0; s < 3 && r.star[s] != NJ_NONE; ++s) out += (s ? "," : "") + text[r.star[s]] + ":" + length_text(r.star_len[s]);
    return out + ");\n";
}

int failures = 0;
void expect(bool ok, const char *what, uint32_t n, int kind) {
    if (!ok) { fprintf(stderr, "FAILED: %s (n = %u, kind = %d)\n", what, n, kind); ++failures; }
}

bool ok(uint32_t n, const Records &r) {
    return nj_records_ok(n, r.a.data(), r.b.data(), r.la.data(), r.lb.data(), (uint32_t)r.a.size(), r.star, r.star_len);
}

}  // namespace

int main() {
    // the length text by hand
    const int64_t one = (int64_t)1 << NJ_FRACTION_BITS;
    expect(length_text(0) == "0" && length_text(7 * one) == "7" && length_text(7 * one + one / 2) == "7.5", "whole and half lengths", 0, 0);
    expect(length_text(-one / 16) == "-0.0625" && length_text(-3 * one) == "-3", "negative lengths", 0, 0);
    expect(length_text(1) == "0.000001" && length_text(-1) == "-0.000001", "the last digit is rounded half up", 0, 0);
    expect(length_text(INT64_MAX) == "8796093022207.999999" && length_text(INT64_MIN) == "-8796093022208", "the ends of 64 bits", 0, 0);
    expect(nj_limit(0) == ((int64_t)1 << 61) && nj_limit(4) == ((int64_t)1 << 59) && nj_limit(3) == 768614336404564650ll, "the range limit", 0, 0);

    const uint32_t sizes[] = {0, 1, 2, 3, 4, 5, 17, 64, 300, 2000};
    for (int kind = 0; kind < 4; ++kind)
        for (uint32_t n : sizes) {
            const Records r = random_records(n, kind);
            const uint32_t m = (uint32_t)r.a.size();
            std::string ids;
            std::vector<uint64_t> off(n + 1, 0);
            std::vector<std::string> labels;
            for (uint32_t i = 0; i < n; ++i) {
                const std::string id = (i % 3 == 0 ? "it's " : i % 3 == 1 ? "plain-" : "under_") + std::to_string(i);
                ids += id;
                off[i + 1] = ids.size();
                Text t;
                nj_put_label(t, id.data(), id.size());
                labels.push_back(t.s);
            }
            expect(n < 1 || labels[0] == "'it''s 0'", "an id with a quote is quoted and the quote doubled", n, kind);
            expect(n < 2 || labels[1] == "plain-1", "a plain id stays bare", n, kind);
            expect(ok(n, r), "nj_records_ok refuses a tree", n, kind);
            Text t;
            nj_put_newick(t, ids.data(), off.data(), n, r.a.data(), r.b.data(), r.la.data(), r.lb.data(), m, r.star, r.star_len);
            expect(t.s == expected(labels, r), "nj_put_newick differs from the tree joined slot by slot", n, kind);
            // the same line with bootstrap support (what snpgpu_write_nj_newick_support writes), counts at both ends of their range
            for (uint32_t replicates : {1u, 3u, 8u, 1000u, 0xFFFFFFFFu}) {
                std::vector<uint32_t> support(m);
                for (uint32_t e = 0; e < m; ++e) support[e] = e == 0 ? 0u : e == 1 ? replicates : rnd(replicates) + (rnd(2) ? 1u : 0u);
                expect(nj_support_ok(support.data(), m, replicates) && nj_joins_ok(n, r.a.data(), r.b.data(), m), "counts within the replicates are refused", n, kind);
                Text with;
                nj_put_newick(with, ids.data(), off.data(), n, r.a.data(), r.b.data(), r.la.data(), r.lb.data(), m, r.star, r.star_len, m ? support.data() : nullptr, replicates);
                expect(with.s == expected(labels, r, &support, replicates), "nj_put_newick with support differs from the tree joined slot by slot", n, kind);
                expect(m > 0 || with.s == t.s, "without a join the line with support is the line without", n, kind);
                if (m && replicates < 0xFFFFFFFFu) {
                    support[m - 1] = replicates + 1;
                    expect(!nj_support_ok(support.data(), m, replicates), "a count above the replicates is refused", n, kind);
                }
                expect(!nj_support_ok(support.data(), m, 0) && (m == 0 || !nj_support_ok(nullptr, m, replicates)), "no replicate, or no counts beside a join, is refused", n, kind);
            }
            expect(nj_percent(0, 7) == 0 && nj_percent(7, 7) == 100 && nj_percent(1, 8) == 13 && nj_percent(1, 3) == 33 && nj_percent(0xFFFFFFFFu, 0xFFFFFFFFu) == 100,
                   "the percentage is half up and exact at the ends of 32 bits", n, kind);
            if (n >= 5) {                                            // what is not a tree is refused before anything is indexed with it
                expect(!nj_joins_ok(n, r.b.data(), r.a.data(), m) && !nj_joins_ok(n - 1, r.a.data(), r.b.data(), m), "joins that are no tree are refused", n, kind);
                Records bad = r;
                bad.b[m - 1] = n + 5;
                expect(!ok(n, bad), "an index past n is refused", n, kind);
                bad = r;
                bad.a[m - 1] = bad.b[m - 1];
                expect(!ok(n, bad), "a = b is refused", n, kind);
                bad = r;
                bad.a[m - 1] = r.b[0];                               // slot b of the first merge has retired (and may be above b)
                expect(!ok(n, bad), "a retired slot is refused", n, kind);
                bad = r;
                bad.a.pop_back(); bad.b.pop_back(); bad.la.pop_back(); bad.lb.pop_back();
                expect(!ok(n, bad), "a list that is not the whole tree is refused", n, kind);
                bad = r;
                std::swap(bad.star[0], bad.star[1]);
                expect(!ok(n, bad), "a star out of order is refused", n, kind);
                bad = r;
                bad.star[2] = NJ_NONE;
                expect(!ok(n, bad), "a star with a slot missing is refused", n, kind);
                bad = r;
                bad.star[1] = r.b[0];
                expect(!ok(n, bad), "a retired slot in the star is refused", n, kind);
                bad = r;
                bad.star[2] = n;
                expect(!ok(n, bad), "a star slot past n is refused", n, kind);
                expect(!nj_records_ok(n, nullptr, r.b.data(), r.la.data(), r.lb.data(), m, r.star, r.star_len), "a null array is refused", n, kind);
                expect(!nj_records_ok(n, r.a.data(), r.b.data(), r.la.data(), r.lb.data(), m, nullptr, r.star_len), "a null star is refused", n, kind);
            }
            if (n <= 2) {
                Records bad = r;
                bad.star[2] = 0;
                expect(!ok(n, bad), "a third star slot of fewer than three samples is refused", n, kind);
            }
        }
    if (failures) return 1;
    printf("nj host check ok\n");
    return 0;
}
