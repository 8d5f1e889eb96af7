"""What the minimum spanning tree and the dendrogram of the distance step must be, stated in plain Python and NumPy: the GPU tests
compare the kernels of csrc/mst.hip and the files of the commands against these; tests/test_mst_cpu.py pins the statements
themselves on the reference's own tables.

Samples are 0 ... n-1; edge {i, j}, i < j, weighs d = mat[i][j]; the edges are totally ordered by (d, i, j), and THE tree is the one
Kruskal's algorithm builds in that order.  An edge is the tuple (d, i, j)."""
import collections
import re

import numpy as np

from tests import clusters_cases as cc
from tests.clusters_ranks_worker import seeded_matrix          # noqa: F401  (the tie matrix: seeded_matrix(300, 17))

HEADER = cc.HEADER
INT_MAX = cc.INT_MAX


def band_edges(mat, row_lo=0, row_hi=None, n=None):
    """Every edge the rows [row_lo, row_hi) hold over the columns < n, once each, in ascending (d, i, j): three int64 arrays."""
    mat = np.asarray(mat)
    n = mat.shape[0] if n is None else n
    row_hi = n if row_hi is None else row_hi
    if row_hi <= row_lo or n == 0:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z
    rows, cols = np.nonzero(np.ones((row_hi - row_lo, n), dtype=bool))
    rows = rows + row_lo
    d = np.asarray(mat[row_lo:row_hi, :n], dtype=np.int64).reshape(-1)
    off = rows != cols
    rows, cols, d = rows[off], cols[off], d[off]
    lo, hi = np.minimum(rows, cols), np.maximum(rows, cols)
    order = np.lexsort((hi, lo, d))
    d, lo, hi = d[order], lo[order], hi[order]
    first = np.ones(len(d), dtype=bool)
    first[1:] = (d[1:] != d[:-1]) | (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])        # an edge between two band rows is there twice
    return d[first], lo[first], hi[first]


class _Sets(object):
    def __init__(self, n):
        self.parent = list(range(n))

    def find(self, x):
        p = self.parent
        while p[x] != x:
            p[x] = p[p[x]]
            x = p[x]
        return x

    def join(self, a, b):
        a, b = self.find(a), self.find(b)
        if a == b:
            return False
        self.parent[max(a, b)] = min(a, b)
        return True


def kruskal(n, edges):
    """The minimum spanning forest of an edge list [(d, u, v)] (duplicates, either orientation) under the order (d, min, max)."""
    sets, out = _Sets(n), []
    for d, lo, hi in sorted((int(d), min(int(u), int(v)), max(int(u), int(v))) for d, u, v in edges):
        if len(out) == n - 1:
            break
        if sets.join(lo, hi):
            out.append((d, lo, hi))
    return out


def mst_of_matrix(mat, row_lo=0, row_hi=None, n=None):
    """Kruskal over the edges of band_edges: [(d, i, j)] ascending."""
    mat = np.asarray(mat)
    n = mat.shape[0] if n is None else n
    d, lo, hi = band_edges(mat, row_lo, row_hi, n)
    sets, out = _Sets(n), []
    for k in range(len(d)):
        if len(out) == n - 1:
            break
        if sets.join(int(lo[k]), int(hi[k])):
            out.append((int(d[k]), int(lo[k]), int(hi[k])))
    return out


def boruvka(mat, row_lo=0, row_hi=None, n=None):
    """Boruvka rounds over the same edges with candidates for BOTH ends of every entry: every component takes its least edge
    (d, i, j) to another component, all of them are contracted.  Returns (edges ascending, rounds that took an edge)."""
    mat = np.asarray(mat)
    n = mat.shape[0] if n is None else n
    d, lo, hi = band_edges(mat, row_lo, row_hi, n)                  # ascending: the first edge that touches a component is its least
    sets, out, rounds = _Sets(n), [], 0
    while True:
        comp = np.asarray([sets.find(i) for i in range(n)], dtype=np.int64)
        cl, ch = comp[lo], comp[hi]
        leaving = np.flatnonzero(cl != ch)
        if len(leaving) == 0:
            break
        ends = np.concatenate((cl[leaving], ch[leaving]))
        which = np.concatenate((leaving, leaving))
        order = np.argsort(which, kind="stable")                    # by edge rank, both ends of an edge next to each other
        _, first = np.unique(ends[order], return_index=True)
        picked = np.unique(which[order][first])
        for k in picked:
            assert sets.join(int(lo[k]), int(hi[k]))                # a total order admits no cycle among the picks
            out.append((int(d[k]), int(lo[k]), int(hi[k])))
        rounds += 1
    return sorted(out), rounds


def ceil_log2(n):
    return max(int(n) - 1, 0).bit_length()


def weight(edges):
    return sum(e[0] for e in edges)


def arrays(edges):
    """(u, v, dist) as the device gives them."""
    return (np.asarray([e[1] for e in edges], dtype=np.uint32), np.asarray([e[2] for e in edges], dtype=np.uint32),
            np.asarray([e[0] for e in edges], dtype=np.int32))


def edges_of_arrays(u, v, dist):
    return [(int(d), int(a), int(b)) for a, b, d in zip(u, v, dist)]


def mst_text(ids, edges):
    return HEADER + "".join("%s\t%s\t%d\n" % (ids[i], ids[j], d) for d, i, j in edges)


def label(name):
    if re.fullmatch(r"[A-Za-z0-9.|-]+", name):
        return name
    return "'" + name.replace("'", "''") + "'"


def half(twice):
    """(d_parent - d_child) / 2 from the integer."""
    assert twice >= 0
    return "%d" % (twice // 2) if twice % 2 == 0 else "%d.5" % (twice // 2)


def newick_text(ids, edges):
    """The dendrogram: the edges in order join the groups of their ends under a node of height d / 2; the child with the smaller
    sample first.  Pieces are kept in deques and the smaller group is poured into the larger, so a 10 000-leaf chain is quick."""
    n = len(ids)
    if n == 0:
        return ";\n"
    assert len(edges) == n - 1
    sets = _Sets(n)
    text = {i: collections.deque([label(ids[i])]) for i in range(n)}
    height = {i: 0 for i in range(n)}                                # twice the node height: the d of the group's last join
    for d, i, j in edges:
        a, b = sets.find(i), sets.find(j)
        assert a != b
        if b < a:
            a, b = b, a                                              # (the root of a set is its smallest sample)
        ta, tb = text.pop(a), text.pop(b)
        mid, end = ":%s," % half(d - height[a]), ":%s)" % half(d - height[b])
        if len(ta) >= len(tb):
            ta.appendleft("(")
            ta.append(mid)
            ta.extend(tb)
            ta.append(end)
            joined = ta
        else:
            tb.appendleft(mid)
            tb.extendleft(reversed(ta))
            tb.appendleft("(")
            tb.append(end)
            joined = tb
        sets.join(a, b)
        text[a], height[a] = joined, d
    assert len(text) == 1
    return "".join(text[sets.find(0)]) + ";\n"


def xor_matrix(n):
    """d(i, j) = 1 + the highest set bit of i ^ j: the components pair up round by round."""
    i = np.arange(n, dtype=np.int64)
    x = i[:, None] ^ i[None, :]
    m = np.zeros((n, n), dtype=np.int32)
    for bit in range(32):
        m[(x >> bit) > 0] = bit + 1
    return m


def random_matrix(n, seed, high=1000):
    rng = np.random.default_rng(seed)
    m = rng.integers(0, high, size=(n, n)).astype(np.int32)
    m = np.minimum(m, m.T)
    np.fill_diagonal(m, 0)
    return m


def chain_edges(n):
    """The tree of d(i, j) = |i - j|: n - 1 edges of weight 1, a chain of n - 1 nested joins."""
    return [(1, i, i + 1) for i in range(n - 1)]
