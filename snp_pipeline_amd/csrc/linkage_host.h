// Host arithmetic of the complete- and average-linkage trees (csrc/linkage.hip, the writers of csrc/tsv_out.hip): the order of the
// merges, the cut at a threshold and the heights in millionths, all in integers.  No device code and no other header of the
// library, so a stand-alone program can include it.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#define SNPGPU_LINKAGE_COMPLETE 0
#define SNPGPU_LINKAGE_AVERAGE 1

typedef unsigned __int128 lnk_u128;

struct LnkMerge {
    uint64_t num;                        // complete: d(A,B); average: S(A,B)
    uint32_t a, b, sa, sb;               // a = id of A < b = id of B, their sizes
};

// key (num / (sa sb), a, b); the rationals are compared by cross-multiplication: num < 2^64 and sa sb < 2^64, so 128 bits hold it
static inline bool lnk_merge_less(int kind, const LnkMerge &x, const LnkMerge &y) {
    if (kind == SNPGPU_LINKAGE_AVERAGE) {
        const lnk_u128 l = (lnk_u128)x.num * ((uint64_t)y.sa * y.sb), r = (lnk_u128)y.num * ((uint64_t)x.sa * x.sb);
        if (l != r) return l < r;
    } else if (x.num != y.num) {
        return x.num < y.num;
    }
    if (x.a != y.a) return x.a < y.a;
    return x.b < y.b;
}

static inline void lnk_sort_merges(int kind, std::vector<LnkMerge> &m) {
    std::sort(m.begin(), m.end(), [kind](const LnkMerge &x, const LnkMerge &y) { return lnk_merge_less(kind, x, y); });
}

// does the merge lie within T: complete num <= T, average num <= T sa sb
static inline bool lnk_within(int kind, uint64_t num, uint32_t sa, uint32_t sb, int32_t t) {
    if (t < 0) return false;
    if (kind == SNPGPU_LINKAGE_AVERAGE) return (lnk_u128)num <= (lnk_u128)(uint64_t)t * ((uint64_t)sa * sb);
    return num <= (uint64_t)t;
}

// the height of a join in millionths: round_half_up(num 10^6 / (2 sa sb)), complete linkage with sa sb taken as 1.
// num 10^6 < 2^84 and the quotient is below 2^64 for every S a matrix of int32 entries can give (S <= 2^31 sa sb).
static inline uint64_t lnk_height(int kind, uint64_t num, uint32_t sa, uint32_t sb) {
    const lnk_u128 pairs = kind == SNPGPU_LINKAGE_AVERAGE ? (lnk_u128)((uint64_t)sa * sb) : (lnk_u128)1;
    return (uint64_t)(((lnk_u128)num * 1000000u + pairs) / (2 * pairs));
}

// the Distance column of the merge file for average linkage, in millionths: round_half_up(S 10^6 / (sa sb))
static inline uint64_t lnk_average_millionths(uint64_t num, uint32_t sa, uint32_t sb) {
    const lnk_u128 pairs = (lnk_u128)((uint64_t)sa * sb);
    return (uint64_t)((2 * (lnk_u128)num * 1000000u + pairs) / (2 * pairs));
}

// do the quotients above fit 64 bits (always, for the sums of int32 entries: S <= 2^31 sa sb)
static inline bool lnk_millionths_fit(int kind, uint64_t num, uint32_t sa, uint32_t sb) {
    const lnk_u128 pairs = kind == SNPGPU_LINKAGE_AVERAGE ? (lnk_u128)((uint64_t)sa * sb) : (lnk_u128)1;
    return (((2 * (lnk_u128)num * 1000000u + pairs) / (2 * pairs)) >> 64) == 0;
}

// merges as the tree they are: a < b < n, both live clusters of the sizes given; n - 1 of them (none for n <= 1) when the whole
// tree is asked for, fewer than n otherwise; with `millionths`, distances that fit 64 bits as millionths
static inline bool lnk_merges_ok(uint32_t n, int kind, const uint32_t *a, const uint32_t *b, const uint32_t *sa, const uint32_t *sb, const uint64_t *num,
                                 uint32_t n_merges, bool whole_tree, bool millionths) {
    if (kind != SNPGPU_LINKAGE_COMPLETE && kind != SNPGPU_LINKAGE_AVERAGE) return false;
    if (n_merges && (!a || !b || !sa || !sb || !num)) return false;
    if (whole_tree ? n_merges != (n ? n - 1 : 0) : n_merges >= (n ? n : 1)) return false;
    std::vector<uint32_t> size(n, 1);
    for (uint32_t e = 0; e < n_merges; ++e) {
        if (a[e] >= b[e] || b[e] >= n || size[a[e]] != sa[e] || size[b[e]] != sb[e] || sa[e] == 0 || sb[e] == 0) return false;
        if (millionths && !lnk_millionths_fit(kind, num[e], sa[e], sb[e])) return false;
        size[a[e]] += size[b[e]];
        size[b[e]] = 0;
    }
    return true;
}

// cluster numbers at every threshold from a merge list lnk_merges_ok accepts, in ascending key order: the merges within T are a
// prefix (heights are monotone); numbers 1, 2, ... in the order of the smallest sample
static inline void lnk_cut(int kind, uint32_t n, const uint32_t *a, const uint32_t *b, const uint32_t *sa, const uint32_t *sb, const uint64_t *num,
                           uint32_t n_merges, const int32_t *thresholds, uint32_t n_thresholds, uint32_t *out_numbers, uint32_t *out_n_clusters) {
    std::vector<uint32_t> parent(n);
    for (uint32_t t = 0; t < n_thresholds; ++t) {
        for (uint32_t i = 0; i < n; ++i) parent[i] = i;
        for (uint32_t e = 0; e < n_merges && lnk_within(kind, num[e], sa[e], sb[e], thresholds[t]); ++e) parent[b[e]] = a[e];   // b is a cluster's smallest sample: a root
        uint32_t count = 0;
        uint32_t *numbers = out_numbers + (size_t)t * n;
        for (uint32_t i = 0; i < n; ++i) {
            uint32_t r = i;
            while (parent[r] != r) r = parent[r];                    // r <= i: numbered already, or i itself
            parent[i] = r;
            numbers[i] = r == i ? ++count : numbers[r];
        }
        if (out_n_clusters) out_n_clusters[t] = count;
    }
}
