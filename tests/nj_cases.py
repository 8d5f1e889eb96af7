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


def nj_numpy(mat, want_lowest=False, rounds=None):
    """The same tree with int64 arrays: the live slots are kept together in their order, so the first least entry of the upper
    triangle in row-major order is the least (Q, i, j).  The asserted bound is what makes int64 enough.  want_lowest adds the
    largest and the lowest working value ever held, in units of 2^-F.  With `rounds` it stops after that many joins and returns
    their records alone (nj_prefix)."""
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
    while len(slots) > 3 and (rounds is None or len(merges) < rounds):
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
    if rounds is not None:
        return merges
    star, star_len = _star([[int(x) for x in row] for row in w], list(range(len(slots))), n)
    star = tuple(None if s is None else int(slots[s]) for s in star)
    return (merges, star, star_len) + ((highest, lowest) if want_lowest else ())


def nj_prefix(mat, rounds):
    """The first `rounds` join records of nj_numpy(mat): the same code, stopping there."""
    return nj_numpy(mat, rounds=rounds)


# ---- checking a tree without building it --------------------------------------------------------------------------------------
class Replay(object):
    """The state of the statement while given joins are applied to it: the full n x n working matrix (rows and columns of retired
    slots stay and are never read), the live mask, and R kept incrementally: a join moves R(k) by new - w(a,k) - w(b,k) for every
    other live k and gives R(a) the sum of the new values.  tests/test_nj_cpu.py shows that this R is the statement's sum over the
    live k in every round.  A join costs O(n); ``ranked`` is the r^2 pass that finds the least pairs."""

    def __init__(self, mat):
        mat = np.asarray(mat)
        self.n = n = mat.shape[0]
        assert mat.shape == (n, n) and not refused(mat)
        self.bound = limit(n)
        self.w = mat.astype(np.int64) << F
        np.fill_diagonal(self.w, 0)
        assert np.array_equal(self.w, self.w.T)
        self.live = np.ones(n, dtype=bool)
        self.R = self.w.sum(axis=1)
        self.r = n

    def summed_R(self):
        """R as the statement has it: the sum of w(i,k) over live k != i, for the live i (0 elsewhere)."""
        return np.where(self.live, (self.w * self.live[None, :]).sum(axis=1), 0)

    def ranked(self, count=1):
        """The first `count` live pairs i < j in the order (Q, i, j)."""
        idx = np.flatnonzero(self.live)
        r = len(idx)
        assert r == self.r and count <= r * (r - 1) // 2
        q = self.w[idx][:, idx]
        q *= r - 2
        q -= self.R[idx][:, None]
        q -= self.R[idx][None, :]
        q[np.tri(r, dtype=bool)] = np.iinfo(np.int64).max           # the diagonal and below: row-major argmin is then the order
        out = []
        for _ in range(count):
            i, j = divmod(int(np.argmin(q)), r)
            out.append((int(idx[i]), int(idx[j])))
            q[i, j] = np.iinfo(np.int64).max
        return out

    def lengths(self, a, b):
        wab = int(self.w[a, b])
        la = ((self.r - 2) * wab + int(self.R[a]) - int(self.R[b])) // (2 * (self.r - 2))
        return la, wab - la

    def join(self, a, b):
        w, R = self.w, self.R
        others = self.live.copy()
        others[a] = others[b] = False
        fresh = np.where(others, (w[a] + w[b] - w[a, b]) >> 1, 0)
        assert int(np.abs(fresh).max()) <= self.bound
        R += np.where(others, fresh - w[a] - w[b], 0)
        R[a] = fresh.sum()
        R[b] = 0
        w[a, :] = fresh
        w[:, a] = fresh
        self.live[b] = False
        self.r -= 1

    def star(self):
        slots = [int(i) for i in np.flatnonzero(self.live)]
        sub = [[int(self.w[i, k]) for k in slots] for i in slots]
        star, star_len = _star(sub, list(range(len(slots))), self.n)
        return tuple(None if s is None else slots[s] for s in star), star_len


def check_tree(mat, tree, argmin_rounds=(), summed_R=False):
    """Is `tree` the tree of the statement?  The recorded joins are replayed: every round must name two live slots a < b with the
    lengths the statement gives that pair in the replayed state, the star and its lengths must be the statement's, and in the rounds
    of `argmin_rounds` the pair must be the least (Q, i, j) of all live pairs.  A wrong state after any round shows in the lengths of
    the rounds behind it; a wrong choice from a right state shows only in an argmin round.  With summed_R the incremental R is
    compared with the sum over the live slots in every round.  Raises AssertionError naming the round."""
    merges, star, star_len = tree
    mat = np.asarray(mat)
    n = mat.shape[0]
    assert len(merges) == max(n - 3, 0), "the tree has %d joins, not %d" % (len(merges), max(n - 3, 0))
    argmin_rounds = set(argmin_rounds)
    assert all(0 <= t < len(merges) for t in argmin_rounds), "an argmin round that is no round"
    state = Replay(mat)
    for t, (a, b, la, lb) in enumerate(merges):
        assert 0 <= a < b < n and state.live[a] and state.live[b], "round %d: (%d, %d) are not two live slots a < b" % (t, a, b)
        if summed_R:
            assert np.array_equal(state.R, state.summed_R()), "round %d: the incremental R is not the sum over the live slots" % t
        if t in argmin_rounds:
            least = state.ranked(1)[0]
            assert least == (a, b), "round %d: (%d, %d) joined, the least (Q, i, j) is (%d, %d)" % ((t, a, b) + least)
        want = state.lengths(a, b)
        assert (la, lb) == want, "round %d: the lengths of (%d, %d) are (%d, %d), not (%d, %d)" % ((t, a, b, la, lb) + want)
        state.join(a, b)
    want = state.star()
    assert (tuple(star), tuple(star_len)) == want, "the star: %r %r, not %r %r" % ((tuple(star), tuple(star_len)) + want)


def far_cherries(n, seed, pairs):
    """Symmetric random entries in 40 ... 60 with a 1 planted at each of the disjoint `pairs`.  A row sum is about 50 r (r live slots;
    it scatters by some 6 sqrt(r)), so Q of a planted pair is about (r - 2) - 100 r = -99 r and that of any other pair 40 r - 100 r =
    -60 r at best: the first len(pairs) rounds join exactly the planted pairs, in an order their row sums decide, and the new node's
    distances are floor((w(a,k) + w(b,k) - 1) / 2), ordinary again.  tests/test_nj_cpu.py asserts that for the lists the GPU tests
    use (tests/nj_geometry.py).  Where a pair lies decides which loop turn of a kernel finds it."""
    pairs = [(int(i), int(j)) for i, j in pairs]
    assert all(0 <= i < j < n for i, j in pairs) and len({x for p in pairs for x in p}) == 2 * len(pairs)
    rng = np.random.default_rng(seed)
    m = np.triu(rng.integers(40, 61, size=(n, n)), 1).astype(np.int32)
    m = m + m.T
    for i, j in pairs:
        m[i, j] = m[j, i] = 1
    assert not refused(m) and (60 << F) <= limit(n)                  # (the update never grows an entry: test_nj_cpu.py)
    return m


def compaction_rounds(n, num, den):
    """[(round, m before, m after)]: the rounds before which the device moves the live columns together, by the arithmetic of
    nj_run's loop: when r den <= m num."""
    out, m, r, t = [], n, n, 0
    while r > 3:
        if r * den <= m * num:
            out.append((t, m, r))
            m = r
        r -= 1
        t += 1
    return out


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


def additive_tree_by_rows(n, seed, longest=9):
    """The matrix of additive_tree(n, seed, longest), drawn with the same calls, from a node-to-node table kept while the tree grows
    instead of a walk per leaf: a node on the edge (u, v) is min(d(u, .) + first, d(v, .) + rest) from everything, a leaf its node's
    row plus its edge.  Fast enough for 2 100 leaves."""
    assert n >= 3
    rng = np.random.default_rng(seed)
    d = np.zeros((2 * n - 2, 2 * n - 2), dtype=np.int64)             # rows and columns of nodes that do not exist yet are rewritten when they appear

    def place(x, row):
        d[x, :] = row
        d[:, x] = row
        d[x, x] = 0

    inner = n
    edges = [[i, inner, int(rng.integers(1, longest + 1))] for i in range(3)]
    edges[int(rng.integers(0, 3))][2] = int(rng.integers(2, longest + 1))
    for i in range(3):
        place(i, np.zeros(2 * n - 2, dtype=np.int64))
    for i, _, length in edges:
        d[i, inner] = d[inner, i] = length
    for i in range(3):
        for k in range(i):
            d[i, k] = d[k, i] = edges[i][2] + edges[k][2]
    for leaf in range(3, n):
        long_enough = [e for e in edges if e[2] >= 2]
        e = long_enough[int(rng.integers(0, len(long_enough)))]
        first = int(rng.integers(1, e[2]))
        inner += 1
        u, v, length = e
        e[1], e[2] = inner, first
        edges.append([inner, v, length - first])
        place(inner, np.minimum(d[u] + first, d[v] + (length - first)))
        d[u, inner] = d[inner, u] = first                            # (u's own row holds 0 for itself: the minimum is right there too; written for clarity)
        hang = int(rng.integers(2, longest + 1))
        edges.append([leaf, inner, hang])
        place(leaf, d[inner] + hang)
        d[leaf, inner] = d[inner, leaf] = hang
    return np.ascontiguousarray(d[:n, :n]).astype(np.int32)


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
