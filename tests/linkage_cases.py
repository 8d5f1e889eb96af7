"""What the complete- and average-linkage trees of the distance step must be, stated in plain Python and NumPy: the GPU tests
compare the kernels of csrc/linkage.hip and the files of the commands against these; tests/test_linkage_cpu.py pins the statements
themselves.

Samples are 0 ... n-1.  A cluster is a set of samples, its id its smallest sample.  complete: d(A,B) = max d(a,b); average:
d(A,B) = S(A,B) / (|A| |B|), S the sum of d(a,b), an exact rational.  Pairs of live clusters are totally ordered by the key
(d(A,B), min id, max id); THE tree merges the least pair n - 1 times (``greedy``).  A merge is the tuple (a, b, size_a, size_b,
num), a = idA < b = idB, num = d for complete linkage and S for average linkage."""
import collections
from fractions import Fraction

import numpy as np

from tests import clusters_cases as cc
from tests.mst_cases import label, random_matrix, seeded_matrix, xor_matrix          # noqa: F401  (the matrices of the tree tests)

KINDS = ("complete", "average")
HEADER = "Seq1\tSeq2\tSize1\tSize2\tDistance\n"
MILLION = 10 ** 6


def _check(mat):
    mat = np.asarray(mat)
    n = mat.shape[0]
    assert mat.shape == (n, n) and np.array_equal(mat, mat.T)
    off = mat[~np.eye(n, dtype=bool)]
    assert (off >= 0).all()
    return n, int(off.max()) if off.size else 0


def _work(mat, n, most):
    """The working matrix: int64 while every cross product num * size * size stays below 2^63, Python integers beyond."""
    safe = most * (max(n, 2) // 2 * ((max(n, 2) + 1) // 2)) ** 2 < 2 ** 62
    return np.asarray(mat).astype(np.int64 if safe else object)      # (astype(object) gives Python integers)


def _least(num, pairs, first, second):
    """Index of the least (num / pairs, first, second) among candidates that come in ascending (first, second): exact, by
    cross-multiplication.  A float picks the few that can be least; integers decide among them."""
    ratio = num.astype(np.float64) / pairs.astype(np.float64)
    near = np.flatnonzero(ratio <= ratio.min() * (1 + 1e-9) + 1e-300)
    best = near[0]
    while True:
        below = near[num[near] * pairs[best] < num[best] * pairs[near]]
        if len(below) == 0:
            break
        best = below[0]
    return near[num[near] * pairs[best] == num[best] * pairs[near]][0]


def _combine(kind, x, y):
    return x + y if kind == "average" else np.maximum(x, y)


def greedy(mat, kind):
    """The definition: n - 1 times the pair of live clusters with the least key, in the order they merge."""
    assert kind in KINDS
    n, most = _check(mat)
    w = _work(mat, n, most)
    size = np.ones(n, dtype=w.dtype)
    live = np.ones(n, dtype=bool)
    out = []
    for _ in range(max(n - 1, 0)):
        ids = np.flatnonzero(live)
        i, j = np.triu_indices(len(ids), 1)                         # ascending (i, j): ties fall to the first
        i, j = ids[i], ids[j]
        pairs = size[i] * size[j] if kind == "average" else np.ones(len(i), dtype=w.dtype)
        at = _least(w[i, j], pairs, i, j)
        a, b = int(i[at]), int(j[at])
        out.append((a, b, int(size[a]), int(size[b]), int(w[a, b])))
        w[a, :] = _combine(kind, w[a, :], w[b, :])
        w[:, a] = w[a, :]
        size[a] += size[b]
        live[b] = False
    return out


def key(kind, merge):
    a, b, sa, sb, num = merge
    return (Fraction(num, sa * sb) if kind == "average" else num, a, b)


def nearest(w, size, live, kind, i):
    """The live k != i with the least (w[i][k] / size[k], k): |i| cancels within a row, and at equal value the smaller k is the
    smaller (min id, max id)."""
    ks = np.flatnonzero(live)
    ks = ks[ks != i]
    weight = size[ks] if kind == "average" else np.ones(len(ks), dtype=w.dtype)
    return int(ks[_least(w[i, ks], weight, ks, ks)])


def rounds(mat, kind):
    """The round form: every round merges ALL reciprocal nearest neighbours.  Returns (merges in ascending key order, rounds)."""
    assert kind in KINDS
    n, most = _check(mat)
    w = _work(mat, n, most)
    size = np.ones(n, dtype=w.dtype)
    live = np.ones(n, dtype=bool)
    out, count = [], 0
    while len(out) < n - 1:
        nn = {int(i): nearest(w, size, live, kind, int(i)) for i in np.flatnonzero(live)}
        picked = [(i, j) for i, j in sorted(nn.items()) if i < j and nn[j] == i]
        assert picked                                                # the least pair of all is reciprocal
        old = w.copy()
        partner = {}
        for i, j in picked:
            partner[i], partner[j] = j, i
            out.append((i, j, int(size[i]), int(size[j]), int(old[i, j])))
        for i, j in picked:                                          # up to four old entries per new one
            for k in np.flatnonzero(live):
                k = int(k)
                if k in (i, j) or (k in partner and partner[k] < k):
                    continue
                v = _combine(kind, old[i, k], old[j, k])
                if k in partner:
                    v = _combine(kind, v, _combine(kind, old[i, partner[k]], old[j, partner[k]]))
                w[i, k] = w[k, i] = v
        for i, j in picked:
            size[i] += size[j]
            live[j] = False
        count += 1
    return sorted(out, key=lambda m: key(kind, m)), count


def within(kind, merge, t):
    a, b, sa, sb, num = merge
    return t >= 0 and (num <= t * sa * sb if kind == "average" else num <= t)


def cut(merges, kind, n, t):
    """Cluster numbers at threshold t: the merges within t (a prefix of the list), numbered 1, 2, ... by smallest sample."""
    parent = list(range(n))
    for m in merges:
        if not within(kind, m, t):
            break
        parent[m[1]] = m[0]
    numbers, count = [0] * n, 0
    for i in range(n):
        r = i
        while parent[r] != r:
            r = parent[r]
        if r == i:
            count += 1
            numbers[i] = count
        else:
            numbers[i] = numbers[r]
    return numbers


def clusters_text(ids, merges, kind, thresholds):
    thresholds = cc.thresholds_in_order(thresholds)
    columns = [cut(merges, kind, len(ids), t) for t in thresholds]
    return "Id\t" + "\t".join(str(t) for t in thresholds) + "\n" + "".join(
        "%s\t%s\n" % (ids[i], "\t".join(str(c[i]) for c in columns)) for i in range(len(ids)))


def half_up(numerator, denominator):
    return (2 * numerator + denominator) // (2 * denominator)


def six_decimals(millionths):
    return "%d.%06d" % divmod(millionths, MILLION)


def merges_text(ids, merges, kind):
    rows = []
    for a, b, sa, sb, num in merges:
        distance = six_decimals(half_up(num * MILLION, sa * sb)) if kind == "average" else "%d" % num
        rows.append("%s\t%s\t%d\t%d\t%s\n" % (ids[a], ids[b], sa, sb, distance))
    return HEADER + "".join(rows)


def height(kind, merge):
    """A join's height in integer millionths: round_half_up(num 10^6 / (2 sa sb))."""
    a, b, sa, sb, num = merge
    return half_up(num * MILLION, 2 * (sa * sb if kind == "average" else 1))


def length(millionths):
    assert millionths >= 0
    whole, fraction = divmod(millionths, MILLION)
    return "%d" % whole if fraction == 0 else ("%d.%06d" % (whole, fraction)).rstrip("0")


def newick_text(ids, merges, kind):
    """The tree: every merge joins the clusters a and b under a node at its height, a (the smaller sample) first."""
    n = len(ids)
    if n == 0:
        return ";\n"
    assert len(merges) == n - 1
    text = {i: collections.deque([label(ids[i])]) for i in range(n)}
    top = {i: 0 for i in range(n)}
    for m in merges:
        a, b, h = m[0], m[1], height(kind, m)
        ta, tb = text[a], text.pop(b)
        mid, end = ":%s," % length(h - top[a]), ":%s)" % length(h - top[b])
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
        top[a] = h
    assert list(text) == [0]
    return "".join(text[0]) + ";\n"


def arrays(merges):
    """(a, b, size_a, size_b uint32, num uint64) as the device gives them."""
    cols = list(zip(*merges)) if merges else [()] * 5
    return tuple(np.asarray(c, dtype=np.uint32) for c in cols[:4]) + (np.asarray(cols[4], dtype=np.uint64),)


def merges_of_arrays(a, b, size_a, size_b, num):
    return [tuple(int(x) for x in m) for m in zip(a, b, size_a, size_b, num)]


def zero_matrix(n):
    """n identical samples: the ids break every tie, one merge per round."""
    return np.zeros((n, n), dtype=np.int32)


def line_matrix(n):
    """d(i, j) = |i - j|."""
    i = np.arange(n, dtype=np.int32)
    return np.abs(i[:, None] - i[None, :]).astype(np.int32)


def planted_symbols(n, s, group, seed=1):
    """Groups of `group` samples a few sites from their centre, the centres s / 20 sites from a common base."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    base = rng.integers(0, 4, size=s, dtype=np.uint8)
    code = np.empty((n, s), dtype=np.uint8)
    for g0 in range(0, n, group):
        centre = base.copy()
        at = rng.choice(s, size=max(1, s // 20), replace=False)
        centre[at] = (centre[at] + rng.integers(1, 4, size=len(at), dtype=np.uint8)) & 3
        code[g0:g0 + group] = centre
        for r in range(g0, min(n, g0 + group)):
            at = rng.integers(0, s, size=int(rng.integers(0, 5)))
            code[r, at] = (code[r, at] + 1) & 3
    return acgt[code]


def hamming_matrix(sym):
    sym = np.asarray(sym)
    return (sym[:, None, :] != sym[None, :, :]).sum(axis=2).astype(np.int32)


def planted_matrix(n=90, s=600, group=7, seed=1):
    return hamming_matrix(planted_symbols(n, s, group, seed))


def tie_matrix(n, high, seed):
    """Entries 0 ... high, symmetric: the smaller `high`, the more ties."""
    return random_matrix(n, seed, high=high + 1)


def diameter(mat, members):
    members = list(members)
    return max([int(mat[i][j]) for i in members for j in members if i != j] or [0])
