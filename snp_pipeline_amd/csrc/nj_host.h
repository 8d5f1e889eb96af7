// Host arithmetic and text of the neighbour-joining tree (csrc/nj.hip, snpgpu_write_nj_newick of csrc/tsv_out.hip): the range
// bound, the floor division, a length in millionths, the check that records are a tree, and the Newick line — all in integers.
// No device code and, of the library, only the text pieces of csrc/text_host.h (sink, numbers, Newick grammar), so a stand-alone
// program can include it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "text_host.h"

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

// a length and a leaf as the tree's line holds them: short millionths, a Newick label
template <typename Sink>
static inline void nj_put_length(Sink &o, int64_t x) {
    const int64_t m = nj_millionths(x);
    txt_put_millionths_short(o, m < 0 ? 0u - (uint64_t)m : (uint64_t)m, m < 0);
}
template <typename Sink>
static inline void nj_put_label(Sink &o, const char *s, size_t len) { txt_put_newick_label(o, s, len); }

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

// One Newick line of records nj_records_ok accepts (the grammar: csrc/text_host.h): the star is a trifurcation at the top (two
// children for n = 2), inside a node slot a comes first.  With support counts (nj_support_ok) the node of merge e carries
// nj_percent(support[e], replicates) between its ')' and its ':'; the trifurcation at the top carries none.
template <typename Sink>
static inline void nj_put_newick(Sink &o, const char *ids, const uint64_t *id_off, uint32_t n, const uint32_t *a, const uint32_t *b, const int64_t *len_a,
                                 const int64_t *len_b, uint32_t n_merges, const uint32_t *star, const int64_t *star_len, const uint32_t *support = nullptr,
                                 uint32_t replicates = 0) {
    const TxtNames names{ids, id_off};
    if (n == 1) nj_put_label(o, ids + id_off[0], names.len(0));
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
        o.put('(');
        for (uint32_t s = 0; s < 3 && star[s] != NJ_NONE; ++s) {
            if (s) o.put(',');
            above[top[star[s]]] = star_len[s];
            txt_put_newick(o, names, n, child.data(), top[star[s]], [&](uint32_t node) {
                if (node >= n && support) txt_put_u64(o, nj_percent(support[node - n], replicates));
                o.put(':');
                nj_put_length(o, above[node]);
            });
        }
        o.put(')');
    }
    o.put(";\n", 2);
}
