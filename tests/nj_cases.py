"""What the neighbour-joining tree of the distance step must be, stated in plain Python: the GPU tests compare the kernels of
csrc/nj.hip and the files of the commands against this; tests/test_nj_cpu.py pins the statement itself.

Samples are 0 ... n-1; the input is a symmetric matrix of non-negative integers whose diagonal is never read.  F = 20 fractional
bits; working values are w(i,k) = matrix[i][k] << F.  A node lives in a slot; slot i starts as sample i and a joined node keeps
the smaller of its two slots, so a node's slot is its smallest sample.  r is the number of live slots.  While r > 3:

  R(i) = the sum of w(i,k) over live k != i;  Q(i,j) = (r-2) w(i,j) - R(i) - R(j) for live i < j;
  the pair least in the order (Q, i, j) is joined: a < b;
  La = floor(((r-2) w(a,b) + R(a) - R(b)) / (2 (r-2))), Lb = w(a,b) - La;
  the new node takes slot a: for every other live k, w(a,k) = w(k,a) = floor((w(a,k) + w(b,k) - w(a,b)) / 2); b retires;
  the record is (a, b, La, Lb).

Lengths and distances may be negative; nothing is clamped.  The last three live slots a < b < c are the star: La = floor((w(a,b) +
w(a,c) - w(b,c)) / 2), Lb = w(a,b) - La, Lc = w(a,c) - La.  n = 2: the star (0, 1, None) with L0 = floor(w / 2), L1 = w - L0.
n <= 1: nothing.  A tree is (merges, star, star_len): max(n - 3, 0) tuples in round order, three slots (None where there is none)
and three lengths (0 where there is no slot).

Range: with L = floor(2^61 / max(n, 1)) every |Q| stays below 2^63 while every |w| <= L; ``nj`` and ``nj_numpy`` assert that for
every value they ever hold, so a tree that comes back from them is a tree the 64-bit device arithmetic can build."""
import collections

import numpy as np

from tests.linkage_cases import hamming_matrix, line_matrix, planted_matrix, planted_symbols, zero_matrix       # noqa: F401  (the matrices of the tree tests)
from tests.mst_cases import label, random_matrix, xor_matrix                                                    # noqa: F401

F = 20
ONE = 1 << F
MILLION = 10 ** 6
INT_MAX = 2 ** 31 - 1


def limit(n):
    return 2 ** 61 // max(n, 1)


def refused(mat):
    """Does the call refuse the matrix before the first round: a negative entry, or (largest entry) << F above the limit."""
    mat = np.asarray(mat)
    n = mat.shape[0]
    off = mat[~np.eye(n, dtype=bool)]
    return bool(off.size) and (int(off.min()) < 0 or (int(off.max()) << F) > limit(n))


def _star(w, live, n):
    if n <= 1:
        return (None, None, None), (0, 0, 0)
    if n == 2:
        half = w[0][1] >> 1
        return (0, 1, None), (half, w[0][1] - half, 0)
    a, b, c = live
    la = (w[a][b] + w[a][c] - w[b][c]) >> 1                          # (Python's >> and // are floors)
    return (a, b, c), (la, w[a][b] - la, w[a][c] - la)


def nj(mat):
    """The definition, in Python integers."""
    mat = np.asarray(mat)
    n = mat.shape[0]
    assert mat.shape == (n, n) and not refused(mat)
    bound = limit(n)
    w = [[0 if i == k else int(mat[i][k]) << F for k in range(n)] for i in range(n)]
    assert all(w[i][k] == w[k][i] for i in range(n) for k in range(i))
    live = list(range(n))
    merges = []
    while len(live) > 3:
        r = len(live)
        R = {i: sum(w[i][k] for k in live if k != i) for i in live}
        q, a, b = min(((r - 2) * w[i][j] - R[i] - R[j], i, j) for x, i in enumerate(live) for j in live[x + 1:])
        assert abs(q) < 2 ** 63
        la = ((r - 2) * w[a][b] + R[a] - R[b]) // (2 * (r - 2))
        merges.append((a, b, la, w[a][b] - la))
        for k in live:
            if k != a and k != b:
                w[a][k] = w[k][a] = (w[a][k] + w[b][k] - w[a][b]) >> 1
                assert abs(w[a][k]) <= bound
        live.remove(b)
    star, star_len = _star(w, live, n)
    return merges, star, star_len


def nj_numpy(mat, want_lowest=False):
    """The same tree with int64 arrays: the live slots are kept together in their order, so the first least entry of the upper
    triangle in row-major order is the least (Q, i, j).  The asserted bound is what makes int64 enough.  want_lowest adds the
    largest and the lowest working value ever held, in units of 2^-F."""
    mat = np.asarray(mat)
    n = mat.shape[0]
    assert mat.shape == (n, n) and not refused(mat)
    bound = limit(n)
    w = mat.astype(np.int64) << F
    np.fill_diagonal(w, 0)
    assert np.array_equal(w, w.T)
    slots = np.arange(n)
    merges = []
    highest, lowest = (int(w.max()), int(w.min())) if n else (0, 0)
    while len(slots) > 3:
        r = len(slots)
        R = w.sum(axis=1)
        q = (r - 2) * w - R[:, None] - R[None, :]
        q[np.tril_indices(r)] = np.iinfo(np.int64).max
        a, b = divmod(int(np.argmin(q)), r)
        wab = int(w[a, b])
        la = ((r - 2) * wab + int(R[a]) - int(R[b])) // (2 * (r - 2))
        merges.append((int(slots[a]), int(slots[b]), la, wab - la))
        fresh = (w[a] + w[b] - wab) >> 1
        fresh[a] = 0
        w[a, :] = fresh
        w[:, a] = fresh
        keep = np.arange(r) != b
        w = w[np.ix_(keep, keep)]
        slots = slots[keep]
        assert int(np.abs(w).max()) <= bound
        highest, lowest = max(highest, int(w.max())), min(lowest, int(w.min()))
    star, star_len = _star([[int(x) for x in row] for row in w], list(range(len(slots))), n)
    star = tuple(None if s is None else int(slots[s]) for s in star)
    return (merges, star, star_len) + ((highest, lowest) if want_lowest else ())


def negative_lengths(tree):
    merges, star, star_len = tree
    return sum(1 for m in merges for x in m[2:] if x < 0) + sum(1 for s, x in zip(star, star_len) if s is not None and x < 0)


def all_lengths(tree):
    merges, star, star_len = tree
    return [x for m in merges for x in m[2:]] + [x for s, x in zip(star, star_len) if s is not None]


# ---- matrices -----------------------------------------------------------------------------------------------------------------
def equal_matrix(n, value=2):
    """Every pair `value` apart.  With 2: a star with unit leaves."""
    return (np.full((n, n), value, dtype=np.int64) - value * np.eye(n, dtype=np.int64)).astype(np.int32)


def star_of_equal(n, value=2):
    """The tree of equal_matrix(n, 2 u), n >= 4, known without building it: every Q is equal in every round, so the ids break every
    tie: (0, 1) join with a leaf's length each, then 0 takes up 2, 3, ... at length 0, and 0, n - 2, n - 1 are left."""
    assert n >= 4 and value % 2 == 0
    u = (value // 2) << F
    return [(0, 1, u, u)] + [(0, j, 0, u) for j in range(2, n - 2)], (0, n - 2, n - 1), (0, u, u)


def additive_tree(n, seed, longest=9):
    """A random unrooted binary tree over n >= 3 leaves by leaf insertion, with positive integer edge lengths, as its matrix of
    path sums.  An edge is split only when its length is at least 2, so both parts stay positive; a new leaf's edge is at least 2
    long, so there always is such an edge."""
    assert n >= 3
    rng = np.random.default_rng(seed)
    # nodes 0 ... n-1 are the leaves, the inner nodes follow; an edge is [u, v, length]
    inner = n
    edges = [[i, inner, int(rng.integers(1, longest + 1))] for i in range(3)]
    edges[int(rng.integers(0, 3))][2] = int(rng.integers(2, longest + 1))
    for leaf in range(3, n):
        long_enough = [e for e in edges if e[2] >= 2]
        e = long_enough[int(rng.integers(0, len(long_enough)))]
        first = int(rng.integers(1, e[2]))                           # 1 ... length - 1
        inner += 1
        u, v, length = e
        e[1], e[2] = inner, first
        edges.append([inner, v, length - first])
        edges.append([leaf, inner, int(rng.integers(2, longest + 1))])
    assert all(e[2] >= 1 for e in edges) and len(edges) == 2 * n - 3
    near = collections.defaultdict(list)
    for u, v, length in edges:
        near[u].append((v, length))
        near[v].append((u, length))
    mat = np.zeros((n, n), dtype=np.int32)
    for leaf in range(n):
        seen, stack = {leaf: 0}, [leaf]
        while stack:
            u = stack.pop()
            for v, length in near[u]:
                if v not in seen:
                    seen[v] = seen[u] + length
                    stack.append(v)
        mat[leaf] = [seen[k] for k in range(n)]
    assert np.array_equal(mat, mat.T)
    return mat


# the matrices the GPU tests give to the device, by name; tests/test_nj_cpu.py asserts the range bound on every one of them
MATRICES = {
    "random": lambda n: random_matrix(n, n, high=40),
    "ties3": lambda n: random_matrix(n, 5, high=3),
    "wide": lambda n: random_matrix(n, 6, high=1000),
    "line": line_matrix,
    "xor": xor_matrix,
    "planted": lambda n: planted_matrix(n, 600, 7),
    "zero": zero_matrix,
    "equal2": equal_matrix,
    "largest": lambda n: equal_matrix(n, INT_MAX),
    "additive": lambda n: additive_tree(n, 7),
}


def path_sums(n, tree):
    """The leaf-to-leaf path sums of a tree as an (n, n) array of Python integers, in units of 2^-F."""
    merges, star, star_len = tree
    out = np.zeros((n, n), dtype=object)
    below = {i: ([i], [0]) for i in range(n)}                        # per slot: the leaves under its node and their depths

    def join(x, y, lx, ly):
        for p, dp in zip(*x):
            for q, dq in zip(*y):
                out[p][q] = out[q][p] = dp + lx + ly + dq

    for a, b, la, lb in merges:
        x, y = below[a], below.pop(b)
        join(x, y, la, lb)
        below[a] = (x[0] + y[0], [d + la for d in x[1]] + [d + lb for d in y[1]])
    left = [(below[s], length) for s, length in zip(star, star_len) if s is not None]
    for i in range(len(left)):
        for j in range(i + 1, len(left)):
            join(left[i][0], left[j][0], left[i][1], left[j][1])
    return out


# ---- text ---------------------------------------------------------------------------------------------------------------------
def millionths(x):
    """A length in integer millionths, half up: floor((2 x 10^6 + 2^F) / 2^(F+1))."""
    return (2 * x * MILLION + (1 << F)) >> (F + 1)


def length(x):
    m = millionths(x)
    whole, fraction = divmod(abs(m), MILLION)
    return ("-" if m < 0 else "") + ("%d" % whole if fraction == 0 else ("%d.%06d" % (whole, fraction)).rstrip("0"))


def newick_text(ids, tree):
    """One line: inside a node the child with the smaller smallest sample (slot a) first; the star a trifurcation at the top."""
    merges, star, star_len = tree
    n = len(ids)
    if n == 0:
        return ";\n"
    if n == 1:
        return label(ids[0]) + ";\n"
    assert len(merges) == max(n - 3, 0)
    text = {i: collections.deque([label(ids[i])]) for i in range(n)}
    for a, b, la, lb in merges:
        ta, tb = text[a], text.pop(b)
        mid, end = ":%s," % length(la), ":%s)" % length(lb)
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
    left = [s for s in star if s is not None]
    assert sorted(text) == left
    return "(" + ",".join("".join(text[s]) + ":" + length(x) for s, x in zip(star, star_len) if s is not None) + ");\n"


def arrays(tree):
    """(a, b uint32, len_a, len_b int64, star, star_len) as Device.nj gives them."""
    merges, star, star_len = tree
    cols = list(zip(*merges)) if merges else [()] * 4
    return tuple(np.asarray(c, dtype=np.uint32) for c in cols[:2]) + tuple(np.asarray(c, dtype=np.int64) for c in cols[2:]) + (tuple(star), tuple(star_len))


def tree_of_arrays(a, b, len_a, len_b, star, star_len):
    return [tuple(int(x) for x in m) for m in zip(a, b, len_a, len_b)], tuple(star), tuple(int(x) for x in star_len)
