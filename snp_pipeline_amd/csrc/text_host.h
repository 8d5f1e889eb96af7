// The text pieces every host writer of the distance step shares (csrc/tsv_out.hip, csrc/nj_host.h): names, numbers, the Newick
// line.  No device code and no other header of the library, so a stand-alone program can include it.
//
// Sink.  Everything here is a template over its sink, which needs put(char) and put(const char *, size_t) and nothing else: the
// library writes a file through one (the buffered sinks of csrc/tsv_out.hip), measures a text with one that only counts, and a
// check program collects a string.
//
// Numbers.  Always integers: txt_put_u64 is str(int); a value in millionths is written short (the integer part and, when the
// fraction is not zero, "." and its digits without trailing zeros: 1500000 is "1.5", 2000000 is "2") or fixed (exactly six
// decimals).  A value is a sign and a 64-bit magnitude, which holds every caller's range: half an int32 distance, a difference of
// lnk_height, |nj_millionths|.
//
// Newick grammar, one line per tree:
//   tree  = node ";" "\n"          node = leaf | "(" node "," node ")"        (neighbour joining: three nodes at the top, two for n = 2)
//   leaf  = the id as it is when it is [A-Za-z0-9.|-]+, else in single quotes with every ' doubled
// and behind every leaf and every ")" but the root's what the tree's writer puts there: ":" and the length of the branch above the
// node, short millionths; neighbour joining with bootstrap support puts the percent between ")" and ":".  Inside a node the child
// with the smaller smallest sample comes first.  A tree of n leaves is an array child[]: node k < n is leaf k, node n + e has the
// children child[2 e] and child[2 e + 1].  It is walked with an explicit stack: a chain of 100 000 nested joins is an ordinary tree.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

// the ids of a table: sample i is the bytes off[i] ... off[i + 1] of ids
struct TxtNames {
    const char *ids;
    const uint64_t *off;
    size_t len(uint32_t i) const { return (size_t)(off[i + 1] - off[i]); }
    template <typename Sink>
    void put(Sink &o, uint32_t i) const { o.put(ids + off[i], len(i)); }
};

template <typename Sink>
static inline void txt_put_u64(Sink &o, uint64_t u) {
    char tmp[20];
    size_t at = sizeof(tmp);
    do { tmp[--at] = (char)('0' + u % 10); u /= 10; } while (u);
    o.put(tmp + at, sizeof(tmp) - at);
}

// (-) v / 10^6 with `decimals` digits of the fraction, which must hold all of it that is not zero
template <typename Sink>
static inline void txt_put_millionths(Sink &o, uint64_t v, bool negative, size_t decimals) {
    char tmp[32];
    size_t at = sizeof(tmp);
    uint32_t frac = (uint32_t)(v % 1000000u);
    for (size_t k = 6; k > decimals; --k) frac /= 10;
    for (size_t k = 0; k < decimals; ++k) { tmp[--at] = (char)('0' + frac % 10); frac /= 10; }
    if (decimals) tmp[--at] = '.';
    v /= 1000000u;
    do { tmp[--at] = (char)('0' + v % 10); v /= 10; } while (v);
    if (negative) tmp[--at] = '-';
    o.put(tmp + at, sizeof(tmp) - at);
}
template <typename Sink>
static inline void txt_put_millionths_short(Sink &o, uint64_t v, bool negative = false) {
    size_t decimals = v % 1000000u ? 6 : 0;
    for (uint32_t frac = (uint32_t)(v % 1000000u); decimals && frac % 10 == 0; frac /= 10) --decimals;
    txt_put_millionths(o, v, negative, decimals);
}
template <typename Sink>
static inline void txt_put_millionths_fixed(Sink &o, uint64_t v) { txt_put_millionths(o, v, false, 6); }

template <typename Sink>
static inline void txt_put_newick_label(Sink &o, const char *s, size_t len) {
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

// The subtree under `root` of the tree child[] over the leaves of `names`: behind(node) writes what follows a leaf's label or a
// join's ")".
template <typename Sink, typename Behind>
static inline void txt_put_newick(Sink &o, const TxtNames &names, uint32_t n, const uint32_t *child, uint32_t root, Behind behind) {
    struct Frame { uint32_t node, state; };                          // state: children written
    std::vector<Frame> stack;
    stack.push_back({root, 0u});
    while (!stack.empty()) {
        Frame &f = stack.back();
        const uint32_t node = f.node;
        if (node >= n && f.state < 2) {
            o.put(f.state ? ',' : '(');
            const uint32_t c = child[2 * (size_t)(node - n) + f.state];
            ++f.state;
            stack.push_back({c, 0u});                                // (f is not used behind this)
            continue;
        }
        if (node < n) txt_put_newick_label(o, names.ids + names.off[node], names.len(node));
        else o.put(')');
        behind(node);
        stack.pop_back();
    }
}
