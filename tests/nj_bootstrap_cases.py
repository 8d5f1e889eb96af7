"""What the bootstrap support values of the neighbour-joining tree must be, stated in plain Python and NumPy: the GPU tests compare
the kernels of csrc/nj_bootstrap.hip and the files of the commands against this; tests/test_nj_bootstrap_cpu.py pins the statement.

Samples are the sorted rows 0 ... n-1, s the column count, B >= 1 the number of replicates, seed a 64-bit unsigned integer (default
1).  All arithmetic modulo 2^64:

  G       = 0x9E3779B97F4A7C15
  mix(z)  : z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  return z ^ (z >> 31)
  draw(seed, b, k) = mix(mix(seed + G (b + 1)) + G (k + 1))          replicate b = 0 ... B-1, position k = 0 ... s-1
  c(b, k)          = floor(draw(seed, b, k) s / 2^64)                the high half of the 64 x 64-bit product

Replicate b: its matrix is the project's distance over the multiset of columns {c(b, k)} (the order of the columns does not enter),
its tree the NJ tree of that matrix exactly as tests/nj_cases.py states it.

Bipartitions: a tree of n >= 4 samples has n - 3 join records (a_t, b_t); record t defines the leaf set under the new node.  Its
canonical form is the side that does NOT hold sample 0 (the complement within the n samples when the leaf set holds sample 0): n - 3
distinct non-trivial bipartitions per tree, each a bitset of W = ceil(n / 64) 64-bit words, bit i of word i / 64 sample i, bits >= n 0.

Support(t) of the main tree (of the unresampled matrix): the number of replicates whose tree holds main bipartition t, 0 ... B.
Percent(t) = floor((200 Support(t) + B) / (2 B)): half up, in integers.  With n <= 3 there is nothing to count."""
import collections
import functools

import numpy as np

from tests import nj_cases as nc
from tests.mst_cases import label

MASK = 2 ** 64 - 1
G = 0x9E3779B97F4A7C15
TABLE_HEADER = "Seq1\tSeq2\tSize\tSupport\tReplicates\n"


def mix(z):
    z &= MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def draw(seed, b, k):
    return mix(mix(seed + G * (b + 1)) + G * (k + 1))


def column(seed, b, k, s):
    return (draw(seed, b, k) * s) >> 64


def _mix_np(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def columns(seed, b, s):
    """c(b, 0 ... s-1) as a uint32 array, in draw order (s < 2^32); the same numbers as ``column``, with wrapping uint64 arrays."""
    assert 0 <= s < 2 ** 32 and 0 <= seed <= MASK
    with np.errstate(over="ignore"):
        base = np.uint64(mix(seed + G * (b + 1)))
        d = _mix_np(base + np.uint64(G) * np.arange(1, s + 1, dtype=np.uint64))
        hi, lo = d >> np.uint64(32), d & np.uint64(0xFFFFFFFF)         # (hi 2^32 + lo) s >> 64, s below 2^32: no product wraps
        out = (hi * np.uint64(s) + ((lo * np.uint64(s)) >> np.uint64(32))) >> np.uint64(32)
    return out.astype(np.uint32)


def distance_matrix(sym):
    """The project's distance: columns where both bytes are in ACGT after upper-casing and differ."""
    sym = np.asarray(sym, dtype=np.uint8)
    n = sym.shape[0]
    upper = np.where((sym >= 97) & (sym <= 122), sym - 32, sym).astype(np.uint8)
    acgt = np.isin(upper, np.frombuffer(b"ACGT", dtype=np.uint8))
    mat = np.zeros((n, n), dtype=np.int32)
    for i in range(n):
        mat[i] = ((upper[i][None, :] != upper) & acgt[i][None, :] & acgt).sum(axis=1)
    return mat


def words(n):
    return (n + 63) // 64


def splits(n, merges):
    """The canonical bipartitions of the join records, in round order, as Python integers (bit i = sample i)."""
    below = {i: 1 << i for i in range(n)}
    everyone = (1 << n) - 1
    out = []
    for m in merges:
        a, b = m[0], m[1]
        below[a] |= below.pop(b)
        out.append(everyone ^ below[a] if below[a] & 1 else below[a])
    return out


def split_words(n, sets):
    """(len(sets), W) uint64: the bitsets as the device lays them out."""
    w = words(n)
    return np.asarray([[(x >> (64 * k)) & MASK for k in range(w)] for x in sets], dtype=np.uint64).reshape(len(sets), w)


def support(n, main_merges, replicate_merges):
    """Per main join: how many of the replicate trees hold its bipartition."""
    have = collections.Counter(x for merges in replicate_merges for x in splits(n, merges))
    return [have[x] for x in splits(n, main_merges)]


def percent(count, replicates):
    return (200 * count + replicates) // (2 * replicates)


def replicate_tree(sym, b, seed):
    sym = np.asarray(sym, dtype=np.uint8)
    return nc.nj_numpy(distance_matrix(sym[:, columns(seed, b, sym.shape[1])]))


def bootstrap(sym, replicates, seed=1):
    """(the main tree as nj_cases gives it, the support counts of its joins)."""
    sym = np.asarray(sym, dtype=np.uint8)
    n = sym.shape[0]
    assert replicates >= 1
    main = nc.nj_numpy(distance_matrix(sym))
    if n <= 3:
        return main, []
    return main, support(n, main[0], [replicate_tree(sym, b, seed)[0] for b in range(replicates)])


# ---- the two inputs that separate strong from weak data --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted():
    sym = nc.planted_symbols(97, 1000, 6, seed=5)
    sym.setflags(write=False)
    return sym


@functools.lru_cache(maxsize=None)
def additive_symbols(n=65, seed=7, copies=20):
    """Symbols grown on additive_tree(n, seed): every edge of length l becomes copies * l identical columns, C under the edge and A
    elsewhere.  The tree is rebuilt from its matrix: the bipartitions of its NJ tree, with the lengths of their edges, and the leaves."""
    mat = nc.additive_tree(n, seed)
    merges, star, star_len = nc.nj(mat)
    cols = []
    below = {i: 1 << i for i in range(n)}
    edges = []                                                       # (leaf set, length in fixed point)
    for a, b, la, lb in merges:
        edges += [(below[a], la), (below[b], lb)]
        below[a] |= below.pop(b)
    edges += [(below[s], x) for s, x in zip(star, star_len)]
    for leaves, x in edges:
        assert x > 0 and x % nc.ONE == 0
        col = np.asarray([ord("C") if (leaves >> i) & 1 else ord("A") for i in range(n)], dtype=np.uint8)
        cols += [col] * (copies * (x >> nc.F))
    sym = np.ascontiguousarray(np.stack(cols, axis=1))
    assert np.array_equal(distance_matrix(sym), copies * mat)
    sym.setflags(write=False)
    return sym


@functools.lru_cache(maxsize=None)
def planted_bootstrap(seed=1, replicates=8):
    return bootstrap(planted(), replicates, seed)


@functools.lru_cache(maxsize=None)
def additive_bootstrap(seed=1, replicates=8):
    return bootstrap(additive_symbols(), replicates, seed)


@functools.lru_cache(maxsize=None)
def differing_seed():
    """The first seed after 1 whose support counts of the planted input differ from those of seed 1."""
    first = planted_bootstrap(1)[1]
    for seed in range(2, 10):
        if planted_bootstrap(seed)[1] != first:
            return seed
    raise AssertionError("no seed of 2 ... 9 moves a count")


# ---- text ------------------------------------------------------------------------------------------------------------------------
def newick_support_text(ids, tree, counts, replicates):
    """nj_cases.newick_text with every join node's Percent between its ')' and its ':'; the top trifurcation carries none."""
    merges, star, star_len = tree
    n = len(ids)
    if n <= 3:
        return nc.newick_text(ids, tree)
    assert len(merges) == len(counts) == n - 3
    text = {i: collections.deque([label(ids[i])]) for i in range(n)}
    mark = {}                                                        # what stands behind a slot's own text before its ':'
    for (a, b, la, lb), c in zip(merges, counts):
        ta, tb = text[a], text.pop(b)
        mid, end = "%s:%s," % (mark.get(a, ""), nc.length(la)), "%s:%s)" % (mark.pop(b, ""), nc.length(lb))
        if len(ta) >= len(tb):
            ta.appendleft("(")
            ta.append(mid)
            ta.extend(tb)
            ta.append(end)
        else:
            tb.appendleft(mid)
            tb.extendleft(reversed(ta))
            tb.appendleft("(")
            tb.append(end)
            text[a] = tb
        mark[a] = "%d" % percent(c, replicates)
    return "(" + ",".join("".join(text[s]) + mark.get(s, "") + ":" + nc.length(x) for s, x in zip(star, star_len) if s is not None) + ");\n"


def support_table_text(ids, merges, counts, replicates):
    size = {i: 1 for i in range(len(ids))}
    rows = []
    for m, c in zip(merges, counts):
        a, b = m[0], m[1]
        size[a] += size.pop(b)
        rows.append("%s\t%s\t%d\t%d\t%d\n" % (ids[a], ids[b], size[a], c, replicates))
    return TABLE_HEADER + "".join(rows)
