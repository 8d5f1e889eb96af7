"""What the close-pairs and clusters outputs of the distance step must be, stated in NumPy and plain Python: the GPU tests compare
the kernels of csrc/clusters.hip and the files of the commands against these; tests/test_clusters_cpu.py pins the statements
themselves on the reference's own tables."""
import itertools

import numpy as np

HEADER = "Seq1\tSeq2\tDistance\n"
INT_MAX = 2 ** 31 - 1

# the listeria fixture (48 samples, distances 0 ... 10 033): T -> (pairs i < j with d <= T, clusters)
LISTERIA_COUNTS = {0: (98, 23), 2: (246, 9), 5: (290, 6), 10: (512, 3), 20: (531, 3), 50: (841, 2)}


def filter_rows(mat, threshold, row_lo=0, row_hi=None, n=None):
    """The CSR of the entries <= threshold of the rows [row_lo, row_hi) over the columns < n: (row_off, col, dist)."""
    mat = np.asarray(mat)
    n = mat.shape[0] if n is None else n
    row_hi = n if row_hi is None else row_hi
    part = mat[row_lo:row_hi, :n]
    keep = part <= threshold
    row_off = np.zeros(row_hi - row_lo + 1, dtype=np.uint64)
    np.cumsum(keep.sum(axis=1), out=row_off[1:])
    rows, cols = np.nonzero(keep)                                   # row-major: rows in order, columns ascending inside a row
    return row_off, cols.astype(np.uint32), part[rows, cols].astype(np.int32)


def adjacency(n, row_off, col, dist, threshold):
    a = np.eye(n, dtype=bool)
    for i in range(n):
        for e in range(int(row_off[i]), int(row_off[i + 1])):
            if dist[e] <= threshold:
                a[i, col[e]] = a[col[e], i] = True
    return a


def reach(adj):
    """Boolean reachability by repeated squaring of the adjacency matrix (with its diagonal) until it stops changing; n <= 300."""
    r = np.asarray(adj, dtype=bool) | np.eye(len(adj), dtype=bool)
    assert len(r) <= 300
    while True:
        nxt = (r.astype(np.uint32) @ r.astype(np.uint32)) > 0
        if np.array_equal(nxt, r):
            return r
        r = nxt


def labels_of_reach(r):
    """Smallest index of every node's component."""
    return np.argmax(r, axis=1).astype(np.int64) if len(r) else np.zeros(0, np.int64)


def numbers_of_labels(labels):
    """Clusters numbered 1, 2, ... in the order of their smallest member; labels[i] = smallest index of i's component."""
    labels = np.asarray(labels, dtype=np.int64)
    roots = np.flatnonzero(labels == np.arange(len(labels)))
    rank = np.zeros(len(labels), dtype=np.int64)
    rank[roots] = np.arange(1, len(roots) + 1)
    return rank[labels]


def cluster_numbers(mat, threshold):
    mat = np.asarray(mat)
    return numbers_of_labels(labels_of_reach(reach(mat <= threshold)))


def union_find_labels(n, edges):
    """Smallest index of every node's component, for graphs too large for reach()."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for u, v in edges:
        a, b = find(int(u)), find(int(v))
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.asarray([find(i) for i in range(n)], dtype=np.int64)


def thresholds_in_order(values):
    return sorted(set(int(v) for v in values))


def pairwise_text(ids, mat):
    """The pairwise file of distance.py:100-106."""
    index = range(len(ids))
    return HEADER + "".join("%s\t%s\t%i\n" % (ids[i], ids[j], mat[i][j]) for i, j in itertools.product(index, index))


def close_pairs_text_of_pairwise(pairwise, threshold):
    """The contract, literally: the header and the rows of the pairwise file with Distance <= T."""
    rows = pairwise.split("\n")[1:-1] if pairwise.endswith("\n") else pairwise.split("\n")[1:]
    return HEADER + "".join(row + "\n" for row in rows if int(row.split("\t")[2]) <= threshold)


def close_pairs_text(ids, mat, threshold):
    row_off, col, dist = filter_rows(mat, threshold)
    out = [HEADER]
    for i in range(len(ids)):
        for e in range(int(row_off[i]), int(row_off[i + 1])):
            out.append("%s\t%s\t%i\n" % (ids[i], ids[col[e]], dist[e]))
    return "".join(out)


def clusters_text(ids, mat, thresholds):
    thresholds = thresholds_in_order(thresholds)
    numbers = [cluster_numbers(mat, t) if len(ids) else [] for t in thresholds]
    out = ["Id\t" + "\t".join(str(t) for t in thresholds) + "\n"]
    for i, name in enumerate(ids):
        out.append(name + "".join("\t%d" % num[i] for num in numbers) + "\n")
    return "".join(out)


def read_matrix_tsv(path):
    """(ids, matrix) of a snp_distance_matrix.tsv."""
    with open(path) as f:
        lines = f.read().split("\n")
    ids = lines[0].split("\t")[1:]
    rows = [line.split("\t") for line in lines[1:] if line]
    assert [r[0] for r in rows] == ids
    return ids, np.asarray([[int(v) for v in r[1:]] for r in rows], dtype=np.int32).reshape(len(ids), len(ids))


def read_pairwise_text(text):
    """(ids in the file's order, matrix) of a pairwise file."""
    rows = [ln.split("\t") for ln in text.split("\n")[1:] if ln]
    ids = []
    for r in rows:
        if r[0] not in ids:
            ids.append(r[0])
    n = len(ids)
    assert len(rows) == n * n
    return ids, np.asarray([int(r[2]) for r in rows], dtype=np.int64).reshape(n, n)
