// Host arithmetic and text of the neighbour-joining tree (csrc/nj.hip, snpgpu_write_nj_newick of csrc/tsv_out.hip): the range
// bound, the floor division, a length in millionths, the check that records are a tree, and the Newick line — all in integers.
// No device code and no other header of the library, so a stand-alone program can include it.  The writer is a template over
// its sink (put(char), put(const char *, size_t)): the library writes a file through it, a check program a string.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#define NJ_FRACTION_BITS 20                  // F: a working value is (matrix entry) << F
#define NJ_NONE 0xFFFFFFFFu

typedef __int128 nj_i128;

// L: while every |w| <= L, every |Q| = |(r - 2) w - R - R| < 3 * 2^61 < 2^63
static inline int64_t nj_limit(uint32_t n) { return (int64_t)(((uint64_t)1 << 61) / (n ? n : 1u)); }

// a length x (fixed point, F fractional bits) in millionths, half up: floor((2 x 10^6 + 2^F) / 2^(F+1)); |result| < 2^63
static inline int64_t nj_millionths(int64_t x) {
    const nj_i128 twice = (nj_i128)x * 2000000 + ((nj_i128)1 << NJ_FRACTION_BITS);
    return (int64_t)(twice >> (NJ_FRACTION_BITS + 1));                // (an arithmetic shift: the floor)
}

// "-" when negative, the integer part, then, when the fraction is not zero, "." and its six digits without trailing zeros
template <typename Sink>
static inline void nj_put_length(Sink &o, int64_t x) {
    const int64_t m = nj_millionths(x);
    uint64_t u = m < 0 ? 0u - (uint64_t)m : (uint64_t)m;
    char tmp[32];
    size_t at = sizeof(tmp);
    uint32_t frac = (uint32_t)(u % 1000000u);
    u /= 1000000u;
    if (frac) {
        size_t kept = 6;
        while (frac % 10 == 0) { frac /= 10; --kept; }
        for (size_t k = 0; k < kept; ++k) { tmp[--at] = (char)('0' + frac % 10); frac /= 10; }
        tmp[--at] = '.';
    }
    do { tmp[--at] = (char)('0' + u % 10); u /= 10; } while (u);
    if (m < 0) tmp[--at] = '-';
    o.put(tmp + at, sizeof(tmp) - at);
}

// a Newick leaf as the other writers of the library put it: the id as it is when it is [A-Za-z0-9.|-]+, else in single quotes
// with every ' doubled
template <typename Sink>
static inline void nj_put_label(Sink &o, const char *s, size_t len) {
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

// records as the tree they are: max(n - 3, 0) merges a < b < n of live slots (b retires), and a star of the slots that are
// left, ascending: three for n >= 3, (0, 1, none) for n = 2, none at all for n <= 1
static inline bool nj_records_ok(uint32_t n, const uint32_t *a, const uint32_t *b, const int64_t *len_a, const int64_t *len_b, uint32_t n_merges,
                                 const uint32_t *star, const int64_t *star_len) {
    if (!star || !star_len || n_merges != (n > 3 ? n - 3 : 0u)) return false;
    if (n_merges && (!a || !b || !len_a || !len_b)) return false;
    std::vector<uint8_t> live(n, 1);
    for (uint32_t e = 0; e < n_merges; ++e) {
        if (a[e] >= b[e] || b[e] >= n || !live[a[e]] || !live[b[e]]) return false;
        live[b[e]] = 0;
    }
    uint32_t at = 0;
    if (n >= 2)
        for (uint32_t i = 0; i < n; ++i)
            if (live[i] && (at >= 3 || star[at++] != i)) return false;
    for (; at < 3; ++at)
        if (star[at] != NJ_NONE) return false;
    return true;
}

// Percent of the bootstrap (csrc/nj_bootstrap.hip): floor((200 count + B) / (2 B)), half up, in integers; B >= 1, count <= B
static inline uint32_t nj_percent(uint32_t count, uint32_t replicates) { return (uint32_t)((200ull * count + replicates) / (2ull * replicates)); }

template <typename Sink>
static inline void nj_put_u32(Sink &o, uint32_t v) {
    char tmp[12];
    size_t at = sizeof(tmp);
    do { tmp[--at] = (char)('0' + v % 10); v /= 10; } while (v);
    o.put(tmp + at, sizeof(tmp) - at);
}

// support counts as they go with records nj_records_ok accepts: one per merge, none above the replicates, of which there is one at least
static inline bool nj_support_ok(const uint32_t *support, uint32_t n_merges, uint32_t replicates) {
    if (replicates == 0 || (n_merges && !support)) return false;
    for (uint32_t e = 0; e < n_merges; ++e)
        if (support[e] > replicates) return false;
    return true;
}

// the merges alone as the joins of a tree of the n samples: max(n - 3, 0) of them, a < b < n, both live (b retires)
static inline bool nj_joins_ok(uint32_t n, const uint32_t *a, const uint32_t *b, uint32_t n_merges) {
    if (n_merges != (n > 3 ? n - 3 : 0u) || (n_merges && (!a || !b))) return false;
    std::vector<uint8_t> live(n, 1);
    for (uint32_t e = 0; e < n_merges; ++e) {
        if (a[e] >= b[e] || b[e] >= n || !live[a[e]] || !live[b[e]]) return false;
        live[b[e]] = 0;
    }
    return true;
}

// One Newick line of records nj_records_ok accepts.  Node k < n is leaf k, node n + e the join of merge e; inside a node the
// child whose smallest sample is smaller (slot a) comes first; the star is a trifurcation at the top (two children for n = 2).
// Written with an explicit stack: a chain of 10 000 nested joins is an ordinary tree here.  With support counts (nj_support_ok) the
// node of merge e carries nj_percent(support[e], replicates) between its ')' and its ':'; the trifurcation at the top carries none.
template <typename Sink>
static inline void nj_put_newick(Sink &o, const char *ids, const uint64_t *id_off, uint32_t n, const uint32_t *a, const uint32_t *b, const int64_t *len_a,
                                 const int64_t *len_b, uint32_t n_merges, const uint32_t *star, const int64_t *star_len, const uint32_t *support = nullptr,
                                 uint32_t replicates = 0) {
    auto label = [&](uint32_t i) { nj_put_label(o, ids + id_off[i], (size_t)(id_off[i + 1] - id_off[i])); };
    if (n == 1) label(0);
    if (n >= 2) {
        std::vector<uint32_t> top(n), child((size_t)n_merges * 2);
        std::vector<int64_t> above((size_t)n + n_merges, 0);         // the length of the branch above a node
        for (uint32_t i = 0; i < n; ++i) top[i] = i;
        for (uint32_t e = 0; e < n_merges; ++e) {
            child[2 * (size_t)e] = top[a[e]];
            child[2 * (size_t)e + 1] = top[b[e]];
            above[top[a[e]]] = len_a[e];
            above[top[b[e]]] = len_b[e];
            top[a[e]] = n + e;
        }
        struct Frame { uint32_t node, state; };
        std::vector<Frame> stack;
        o.put('(');
        for (uint32_t s = 0; s < 3 && star[s] != NJ_NONE; ++s) {
            if (s) o.put(',');
            above[top[star[s]]] = star_len[s];
            stack.push_back({top[star[s]], 0u});
            while (!stack.empty()) {
                Frame &f = stack.back();
                const uint32_t node = f.node;
                if (node >= n && f.state < 2) {
                    o.put(f.state ? ',' : '(');
                    const uint32_t c = child[2 * (size_t)(node - n) + f.state];
                    ++f.state;
                    stack.push_back({c, 0u});                        // (f is not used behind this)
                    continue;
                }
                if (node < n) label(node);
                else {
                    o.put(')');
                    if (support) nj_put_u32(o, nj_percent(support[node - n], replicates));
                }
                o.put(':');
                nj_put_length(o, above[node]);
                stack.pop_back();
            }
        }
        o.put(')');
    }
    o.put(";\n", 2);
}
