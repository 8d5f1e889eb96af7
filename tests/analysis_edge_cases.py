"""Inputs that take the component, linkage and cluster-SNP kernels (csrc/clusters.hip, linkage.hip, cluster_snps.hip) past the
first turn of their grid-stride loops and the first block of the prims.h scans under them, and the plain restatements their
results are compared with.  tests/test_analysis_edges_cpu.py pins what is stated here against tests/clusters_cases.py,
tests/linkage_cases.py and tests/cluster_snps_cases.py; tests/test_gpu_analysis_edges.py runs the kernels on it.  No GPU, and
nothing here shares code with the package: the kernels' constants are read from the text of their sources."""
import os
import re

import numpy as np

from tests import cluster_snps_cases as sc
from tests import clusters_cases as cc
from tests import linkage_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def define(source, name):
    """The integer a `#define name value` of csrc/<source> gives."""
    with open(os.path.join(ROOT, "snp_pipeline_amd", "csrc", source)) as f:
        return int(re.search(r"^#define %s (\d+)\b" % re.escape(name), f.read(), re.M).group(1))


# ---- A. components ------------------------------------------------------------------------------------------------------------

def csr_of_edges(n, u, v, w):
    """Every edge in both directions, the rows in order, the columns ascending inside a row: (row_off, col, dist)."""
    rows = np.concatenate([u, v]).astype(np.int64)
    cols = np.concatenate([v, u]).astype(np.int64)
    dist = np.concatenate([w, w]).astype(np.int64)
    order = np.lexsort((dist, cols, rows))
    row_off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(np.bincount(rows, minlength=n), out=row_off[1:])
    return row_off, cols[order].astype(np.uint32), dist[order].astype(np.int32)


def forest(n, path, seed, gaps, gap_half, hub, hub_degree=80, long_every=50):
    """Paths of `path` nodes whose order along the path is a seeded permutation of the node indices; about one link in
    `long_every` has d = 9, the others d = 1.  The nodes within `gap_half` of every index of `gaps` have no edge at all.  Node
    `hub` has `hub_degree` more links (d = 1 and 9 in turn) to nodes of other paths.  Returns (u, v, w, lonely)."""
    rng = np.random.default_rng(seed)
    lonely = np.concatenate([np.arange(g - gap_half, g + gap_half) for g in gaps]).astype(np.int64)
    assert lonely.min() >= 0 and lonely.max() < n and hub not in lonely.tolist()
    keep = np.ones(n, dtype=bool)
    keep[lonely] = False
    order = rng.permutation(n)
    order = order[keep[order]]
    link = (np.arange(len(order) - 1) + 1) % path != 0               # no link from the last node of a path to the first of the next
    u, v = order[:-1][link], order[1:][link]
    w = np.where(rng.integers(0, long_every, size=len(u)) == 0, 9, 1)
    far = rng.choice(order[order != hub], size=hub_degree, replace=False)
    u = np.concatenate([u, np.full(hub_degree, hub)])
    v = np.concatenate([v, far])
    w = np.concatenate([w, np.where(np.arange(hub_degree) % 2 == 0, 1, 9)])
    return u.astype(np.int64), v.astype(np.int64), w.astype(np.int64), lonely


def random_edges(n, m, seed, high=10):
    rng = np.random.default_rng(seed)
    u, v = rng.integers(0, n, size=m), rng.integers(0, n, size=m)
    off = u != v
    return u[off].astype(np.int64), v[off].astype(np.int64), rng.integers(0, high, size=m)[off].astype(np.int64)


def numbers_by_union_find(n, u, v, w, threshold):
    """Cluster numbers of the edges with d <= threshold: union-find, then numbered by smallest member."""
    keep = w <= threshold
    return cc.numbers_of_labels(cc.union_find_labels(n, zip(u[keep].tolist(), v[keep].tolist())))


def numbers_by_reach(n, csr, threshold):
    return cc.numbers_of_labels(cc.labels_of_reach(cc.reach(cc.adjacency(n, csr[0], csr[1], csr[2], threshold))))


def extreme_edges(n, seed):
    """Edges whose distances are mostly small and of either sign, some of them the two ends of int32."""
    rng = np.random.default_rng(seed)
    u, v, w = random_edges(n, 2 * n, seed, high=7)
    w = w - 3
    at = rng.permutation(len(w))
    w[at[:n // 5]] = INT_MIN
    w[at[n // 5:2 * n // 5]] = INT_MAX
    return u, v, w


# ---- B. linkage ---------------------------------------------------------------------------------------------------------------

def planted_far_column(mat, rows):
    """Every entry off the diagonal one larger — so that no row holds a 0 — and then the entries (r, n - 1) and (n - 1, r) set to 0
    for the rows given: the nearest neighbour of each of them is the last column, and of the last column the first of them."""
    out = np.array(mat, dtype=np.int32) + 1
    np.fill_diagonal(out, 0)
    last = out.shape[0] - 1
    for r in rows:
        out[r, last] = out[last, r] = 0
    return out


def xor_with_outliers(block, outliers, seed, first, between=48):
    """d(i, j) = i xor j among `block` samples, and `outliers` more whose distance to everything is 5 000 + a seeded value below
    50, symmetric.  first: the outliers are samples 0 ... outliers - 1 and the block follows; otherwise they come last.  Against
    the block the value is seeded and below 48, but for the one largest entry of outlier k, 5 049, against block sample
    block - 1 - 2 k — an odd one, which retires into its neighbour in the first round, among the last merges of that round —;
    between two outliers it is `between`.  At 48, under complete linkage, an outlier is 5 049 from the block once that is one
    cluster and 5 048 from the other outliers; at 10, under average linkage, it is about 5 023 from the block and 5 010 from the
    others.  Either way the outliers join each other first, and only a row that has lost some of its entries against the block
    takes the block for its nearest neighbour."""
    n = block + outliers
    rng = np.random.default_rng(seed)
    mat = 5000 + rng.integers(0, 48, size=(n, n))
    mat = np.minimum(mat, mat.T)
    lo = outliers if first else 0
    far = np.arange(outliers) + (0 if first else block)
    mat[np.ix_(far, far)] = 5000 + between
    for k in range(outliers):
        o = k if first else block + k
        mat[o, lo + block - 1 - 2 * k] = mat[lo + block - 1 - 2 * k, o] = 5049
    i = np.arange(block, dtype=np.int64)
    mat[lo:lo + block, lo:lo + block] = i[:, None] ^ i[None, :]
    np.fill_diagonal(mat, 0)
    return mat.astype(np.int32)


def first_round(mat, kind):
    """The reciprocal nearest neighbours of the matrix as it stands: the pairs (i, j), i < j, that the first round of lc.rounds picks."""
    mat = np.asarray(mat)
    n = mat.shape[0]
    w = mat.astype(np.int64)
    size, live = np.ones(n, dtype=np.int64), np.ones(n, dtype=bool)
    nn = [lc.nearest(w, size, live, kind, i) for i in range(n)]
    return [(i, j) for i, j in enumerate(nn) if i < j and nn[j] == i]


BETWEEN = {"complete": 48, "average": 10}                           # xor_with_outliers: between two outliers, by linkage


# ---- C. cluster SNPs ----------------------------------------------------------------------------------------------------------

def cluster_snps_fast(sym, labels, n_clusters, block=512):
    """sc.cluster_snps without its loop over the clusters: the rows in stable order of their labels, the members per base, cluster
    and column by np.add.reduceat (inside[4][C + 1][columns]; index 0 and a number without rows stay 0), everywhere = inside.sum(1),
    and an entry where exactly one base is held inside and inside == everywhere.  `block` columns at a time, to bound memory."""
    code = sc.base_codes(sym)
    labels = np.asarray(labels, dtype=np.int64)
    n, s = code.shape
    c_total = int(n_clusters)
    assert labels.shape == (n,) and (n == 0 or (labels.min() >= 1 and labels.max() <= c_total))
    order = np.argsort(labels, kind="stable")
    code, labels = code[order], labels[order]
    starts = np.flatnonzero(np.concatenate([[True], labels[1:] != labels[:-1]])) if n else np.zeros(0, dtype=np.int64)
    present = labels[starts]                                        # the numbers that have rows, ascending
    found = [np.zeros(0, dtype=np.int64)] * 4                       # cluster (0-based), column, base, members
    for lo in range(0, s, block if n else s):
        part = code[:, lo:lo + block]
        inside = np.zeros((4, c_total + 1, part.shape[1]), dtype=np.int32)
        for b in range(4):
            inside[b, present] = np.add.reduceat(part == b, starts, axis=0, dtype=np.int32)
        everywhere = inside.sum(axis=1)
        held = inside > 0
        entry = held & (held.sum(axis=0) == 1)[None] & (inside == everywhere[:, None, :])
        b, c, col = np.nonzero(entry)
        found = [np.concatenate([x, y]) for x, y in zip(found, (c - 1, col + lo, b, inside[b, c, col]))]
    by = np.lexsort((found[1], found[0]))                            # by cluster, then column
    c, col, b, members = (x[by] for x in found)
    off = np.zeros(c_total + 1, dtype=np.uint64)
    np.cumsum(np.bincount(c, minlength=c_total), out=off[1:])
    return off, col.astype(np.uint32), b.astype(np.uint8), members.astype(np.uint32)


def labels_of_sizes(sizes, seed=None):
    """Cluster c (from 1) has sizes[c - 1] rows; with a seed the rows are shuffled, so that no cluster is contiguous."""
    labels = np.repeat(np.arange(1, len(sizes) + 1), sizes).astype(np.uint32)
    return labels if seed is None else labels[np.random.default_rng(seed).permutation(len(labels))]


def mixed_sizes(c, seed):
    """One to three rows per cluster, and none for the cluster number c - 1."""
    sizes = np.random.default_rng(seed).integers(1, 4, size=c)
    sizes[c - 2] = 0
    return sizes


def _stride(s):
    """A step of about 0.38 s that is coprime to s: q -> q * step % s visits every column once and neighbours land far apart."""
    step = max(1, int(0.381966 * s))
    while np.gcd(step, s) != 1:
        step += 1
    return step


def background(n, s, seed):
    """No base but A anywhere: A, a, - or N."""
    return np.frombuffer(b"Aa-N", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, size=(n, s))].copy()


def private_plants(n_clusters, s, every=3, repeat=50):
    """[(cluster from 1, column, base 1 ... 3)]: every `every`-th cluster, the q-th of them at column q * step % s (all word tiles,
    neighbours far apart) with base 1 + q // s % 3 — injective in q — but every `repeat`-th repeats its predecessor's pair."""
    step = _stride(s)
    plants = []
    for q, c in enumerate(range(0, n_clusters, every)):
        assert q < 3 * s
        pair = (q * step % s, 1 + q // s % 3)
        if q % repeat == repeat - 1:
            pair = plants[-1][1:]
        plants.append((c + 1,) + pair)
    return plants


def planted_private(labels, n_clusters, s, seed, every=3, repeat=50, gap_every=5):
    """The background with, for every plant of private_plants, ALL members of the cluster holding the base at the column (either
    case); in every `gap_every`-th planted cluster of more than one row, one member holds '-' there instead."""
    labels = np.asarray(labels, dtype=np.int64)
    n = len(labels)
    rng = np.random.default_rng(seed)
    sym = background(n, s, seed + 1)
    order = np.argsort(labels, kind="stable")
    first = np.searchsorted(labels[order], np.arange(1, n_clusters + 2))
    letters = np.frombuffer(b"CGTcgt", dtype=np.uint8)
    several = 0
    for c, col, base in private_plants(n_clusters, s, every, repeat):
        rows = order[first[c - 1]:first[c]]
        sym[rows, col] = letters[base - 1 + 3 * rng.integers(0, 2, size=len(rows))]
        if len(rows) > 1:
            several += 1
            if several % gap_every == 0:
                sym[rows[rng.integers(0, len(rows))], col] = 0x2D
    return sym


def plant(sym, labels, clusters, col, letter):
    """Column `col` back to '-' everywhere, then `letter` in every member of the clusters given."""
    sym[:, col] = 0x2D
    sym[np.isin(labels, clusters), col] = letter


def entries_of(want):
    """{(cluster from 1, column): (base, members)} of a (cluster_off, site, base, members) result."""
    off, site, base, members = want
    cluster = np.repeat(np.arange(1, len(off)), np.diff(off.astype(np.int64)))
    return {(int(c), int(x)): (int(b), int(m)) for c, x, b, m in zip(cluster, site, base, members)}


def per_tile(want, tile_sites, n_tiles):
    return np.bincount(want[1].astype(np.int64) // tile_sites, minlength=n_tiles)


def check_large(want, sizes, s, tile, mixed):
    """What the expected entries of the large inputs must be like for a comparison with them to say anything: many, in every word
    tile, among the last clusters, and — when the clusters have several rows — held by several members and by fewer than all."""
    off = want[0].astype(np.int64)
    c = len(off) - 1
    of_entry = np.repeat(np.asarray(sizes, dtype=np.int64), np.diff(off))
    assert len(want[1]) >= 1000
    assert (per_tile(want, tile, -(-s // tile)) >= 100).all()
    assert off[-1] - off[3 * c // 4] >= 100
    assert (want[3] >= 1).all() and (want[3] <= of_entry).all()
    if mixed:
        assert (want[3] > 1).any() and (want[3] < of_entry).any()


COL_TWICE, COL_ONCE = 7, 150


def chunk_edge_case(c, chunk, across, n=400, s=200):
    """n shuffled rows in c clusters on the constructed input, and two columns of their own: at COL_TWICE exactly two clusters hold G
    — the first cluster of the first and of the last chunk of `chunk` clusters when `across` (the last cluster when there is one
    chunk), else two clusters of the first chunk —, at COL_ONCE a cluster of the last chunk alone holds t.  Returns (labels, sym,
    the two clusters, the one cluster)."""
    labels = (np.random.default_rng(c).permutation(n) % c + 1).astype(np.uint32)
    sym = planted_private(labels, c, s, 40 + c)
    last_first = (c - 1) // chunk * chunk + 1
    pair = (1, last_first if last_first > 1 else c) if across else (2, min(chunk, c) - 1)
    last = c if c - last_first < 2 else last_first + 1
    plant(sym, labels, pair, COL_TWICE, 0x47)
    plant(sym, labels, (last,), COL_ONCE, 0x74)
    return labels, sym, pair, last
