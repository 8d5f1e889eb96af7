"""The component kernels of csrc/clusters.hip, the linkage kernels of csrc/linkage.hip and the cluster-SNP kernels of
csrc/cluster_snps.hip past the first turn of their grid-stride loops and past the first block of the prims.h scans under them, on
the inputs of tests/analysis_edge_cases.py.  The expected values are the plain statements of tests/clusters_cases.py,
tests/linkage_cases.py and tests/cluster_snps_cases.py, or a restatement that tests/test_analysis_edges_cpu.py pins against them.
Everything is compared exactly, every output keeps a mark behind its last element, and every cap or block size a shape is meant
to pass is read from the kernel's source and asserted to be passed: a cap that changes fails the test that leaned on it.

NOT exercised here, because each needs an input no test can hold:
  - the second turn of k_sweep and of k_unique_part (cluster_snps.hip): tiles x row chunks, or parts x tiles, beyond 64 waves per
    CU — gigabytes of symbols;
  - the chunk loop of k_mst_cols (mst.hip): 65 536 band rows;
  - the second turn of the per-slot kernels of mst.hip and linkage.hip: more than 524 288 samples, an n x n matrix;
  - average linkage's refusal of a sum that could reach 2^64: about 185 000 samples.
"""
import functools

import numpy as np
import pytest

from tests import analysis_edge_cases as ae
from tests import cluster_snps_cases as sc
from tests import linkage_cases as lc
from tests.gpu_util import get_device

pytestmark = pytest.mark.gpu

MARK = 0x5A5A5A5A
BYTE = 0xA5


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- A. components ------------------------------------------------------------------------------------------------------------

def _cc_sizes():
    """(items of one turn of the edge and label kernels, rows of one turn of k_cc_rows, elements of one block of the u32 scan)"""
    threads, cap = ae.define("clusters.hip", "CLUSTERS_THREADS"), ae.define("clusters.hip", "CLUSTERS_EDGE_GRID_CAP")
    return cap * threads, cap * (threads // 64), ae.define("prims.h", "PRIM_SCAN_THREADS") * ae.define("prims.h", "PRIM_SCAN_ITEMS")


def _clusters_dev(d, n, csr, thresholds):
    import torch
    off, col, dist = torch.from_numpy(csr[0].view(np.int64)).cuda(), torch.from_numpy(csr[1].view(np.int32)).cuda(), torch.from_numpy(csr[2]).cuda()
    k = len(thresholds)
    out = torch.full((k * n + 8,), MARK, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    counts = d.clusters_dev(n, off.data_ptr(), col.data_ptr(), dist.data_ptr(), len(csr[1]), thresholds, out.data_ptr())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[k * n:] == MARK).all()
    assert np.array_equal(off.cpu().numpy(), csr[0].view(np.int64)) and np.array_equal(col.cpu().numpy(), csr[1].view(np.int32)) and np.array_equal(dist.cpu().numpy(), csr[2])
    return got[:k * n].reshape(k, n).astype(np.int64), counts.astype(np.int64)


def test_a_forest_past_every_grid_and_scan_block_of_the_components():
    """600 000 nodes in scrambled paths of 1 000, a fiftieth of the links too long for the smaller threshold, two thresholds in
    one call: every k_cc_* kernel goes round its grid-stride loop, k_cc_rows writes a row of more than 64 entries in its second
    turn, nodes on both sides of every turn and block edge have no edge at all, and the numbering scans 74 blocks."""
    d = get_device()
    per_turn, rows_per_turn, scan_block = _cc_sizes()
    n, thresholds = 600000, [5, 9]
    hub = n // 2
    u, v, w, lonely = ae.forest(n, 1000, 24, gaps=sorted({rows_per_turn, scan_block, per_turn}), gap_half=75, hub=hub)
    csr = ae.csr_of_edges(n, u, v, w)
    assert n > per_turn and len(csr[1]) > 2 * per_turn and n * len(thresholds) > 2 * per_turn
    assert n > rows_per_turn and hub >= rows_per_turn and csr[0][hub + 1] - csr[0][hub] > 64
    assert n > 2 * scan_block
    for edge in (rows_per_turn, scan_block, per_turn):
        assert (lonely < edge).any() and (lonely >= edge).any()
    want = [ae.numbers_by_union_find(n, u, v, w, t) for t in thresholds]
    assert n > want[0].max() > want[1].max() > len(lonely) and all((np.bincount(x)[x[lonely]] == 1).all() for x in want)
    numbers, counts = _clusters_dev(d, n, csr, thresholds)
    for k in range(len(thresholds)):
        assert counts[k] == want[k].max() and np.array_equal(numbers[k], want[k]), thresholds[k]
    numbers, counts = d.clusters(n, csr[0], csr[1], csr[2], thresholds)                        # the host form, once, on the same CSR
    for k in range(len(thresholds)):
        assert counts[k] == want[k].max() and np.array_equal(numbers[k], want[k]), (thresholds[k], "host form")


@pytest.mark.parametrize("n", [8193, 8191])
def test_the_first_and_last_node_beside_a_scan_block(n):
    """The last node has no edge: it is a root and its number is the count, which at n = block + 1 crosses from one scan block
    into the next; it is also the first row of k_cc_rows's second turn."""
    d = get_device()
    _, rows_per_turn, scan_block = _cc_sizes()
    assert rows_per_turn == scan_block and n in (scan_block + 1, scan_block - 1)
    u, v, w = ae.random_edges(n, n // 2, n)
    keep = (u != n - 1) & (v != n - 1)
    u, v, w = u[keep], v[keep], w[keep]
    csr = ae.csr_of_edges(n, u, v, w)
    want = ae.numbers_by_union_find(n, u, v, w, 4)
    assert want[n - 1] == want.max() and n // 2 < want.max() < n
    numbers, counts = _clusters_dev(d, n, csr, [4])
    assert counts[0] == want.max() and np.array_equal(numbers[0], want)


def test_thresholds_at_the_ends_of_int32():
    d = get_device()
    n, thresholds = 300, [ae.INT_MIN, -1, ae.INT_MAX]
    u, v, w = ae.extreme_edges(n, 11)
    csr = ae.csr_of_edges(n, u, v, w)
    want = [ae.numbers_by_reach(n, csr, t) for t in thresholds]
    assert n > want[0].max() > want[1].max() > want[2].max()
    for numbers, counts in (_clusters_dev(d, n, csr, thresholds), d.clusters(n, csr[0], csr[1], csr[2], thresholds)):
        for k in range(3):
            assert counts[k] == want[k].max() and np.array_equal(numbers[k], want[k]), thresholds[k]


# ---- B. linkage ---------------------------------------------------------------------------------------------------------------

def _tree(d, mat, kind, stride=None, garbage=False):
    """(merges, rounds) of the matrix at a row pitch of `stride`; with `garbage`, INT32_MIN / INT32_MAX fill the padding columns
    and the diagonal.  The matrix must come back untouched, and so must what lies behind the n - 1 merges."""
    import torch
    n = mat.shape[0]
    stride = n if stride is None else stride
    host = np.zeros((n, stride), dtype=np.int32)
    if garbage:
        host[:] = np.where((np.arange(host.size).reshape(host.shape) % 3) == 0, ae.INT_MIN, ae.INT_MAX)
    host[:n, :n] = mat
    if garbage:
        host[np.arange(n), np.arange(n)] = np.where(np.arange(n) % 2 == 0, ae.INT_MIN, ae.INT_MAX)
    t = torch.from_numpy(host).cuda()
    room = n - 1 + 8
    out = [torch.full((room,), MARK, dtype=torch.int32, device="cuda") for _ in range(4)] + [torch.full((room,), MARK, dtype=torch.int64, device="cuda")]
    torch.cuda.synchronize()
    k, rounds = d.linkage_dev(t.data_ptr(), n, stride, kind, *(o.data_ptr() for o in out))
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), host)
    got = [o.cpu().numpy() for o in out]
    assert k == n - 1
    assert all((g[k:] == MARK).all() for g in got)
    return lc.merges_of_arrays(*(g[:k].view(np.uint32) for g in got[:4]), got[4][:k].view(np.uint64)), rounds


MATRICES = {
    "ties": lambda n: lc.random_matrix(n, n, high=40),
    "wide": lambda n: lc.random_matrix(n, 6, high=1000),
    "outliers last complete": lambda n: ae.xor_with_outliers(n - 5, 5, 1, False, ae.BETWEEN["complete"]),
    "outliers first complete": lambda n: ae.xor_with_outliers(n - 5, 5, 1, True, ae.BETWEEN["complete"]),
    "outliers last average": lambda n: ae.xor_with_outliers(n - 5, 5, 1, False, ae.BETWEEN["average"]),
    "outliers first average": lambda n: ae.xor_with_outliers(n - 5, 5, 1, True, ae.BETWEEN["average"]),
    "far column": lambda n: ae.planted_far_column(lc.random_matrix(n, n, high=40), (3, 100, 255)),
}


@functools.lru_cache(maxsize=None)
def _want(name, n, kind):
    mat = np.ascontiguousarray(MATRICES[name](n), dtype=np.int32)
    assert np.array_equal(mat, mat.T)
    mat.setflags(write=False)
    return mat, lc.greedy(mat, kind)


def _lnk_step():
    threads = ae.define("linkage.hip", "LNK_THREADS")
    return ae.define("linkage.hip", "LNK_UNROLL") * threads, threads


@pytest.mark.parametrize("kind", lc.KINDS)
@pytest.mark.parametrize("name,n", [("ties", 1023), ("ties", 1024), ("ties", 1025), ("ties", 1281), ("wide", 1025)])
def test_rows_at_and_past_one_step_of_the_row_loops(name, n, kind):
    """One step of k_lnk_rows and k_lnk_contract is LNK_UNROLL x LNK_THREADS columns: n one below, at and one above it, and in
    the second load of the second step.  At step + 1 also at a row pitch of n + 3 with INT32_MIN / INT32_MAX behind the rows and
    on the diagonal: the loads past the last column of the first step lie next to them."""
    d = get_device()
    step, threads = _lnk_step()
    assert n in (step - 1, step, step + 1, step + threads + 1)
    mat, want = _want(name, n, kind)
    count = lc.rounds(mat, kind)[1]
    assert 1 < count < n - 1
    assert _tree(d, mat, kind) == (want, count)
    if n == step + 1:
        assert _tree(d, mat, kind, stride=n + 3, garbage=True) == (want, count)


@pytest.mark.parametrize("kind", lc.KINDS)
@pytest.mark.parametrize("name", ["outliers last", "outliers first"])
def test_a_round_of_512_merges_with_five_bystanders(name, kind):
    """d = i xor j on 1 024 samples and five far outliers: the first round merges every i with i xor 1 — more merges than
    k_lnk_contract has threads, so that the five rows that do not merge go twice round its list loop — and every block row
    combines four entries.  With the outliers first they are the smallest ids and the block's ids shift.  The largest entry of
    every outlier is against a sample that retires in one of the last merges of the round, and the outliers are just nearer to
    each other than to the whole block (tests/analysis_edge_cases.py: xor_with_outliers): a row that the second turn of the list
    loop left as it was takes the block for its nearest neighbour, and the tree shows it, whichever side of W the records read."""
    d = get_device()
    step, threads = _lnk_step()
    n = 1029
    mat, want = _want("%s %s" % (name, kind), n, kind)
    picked = ae.first_round(mat, kind)
    lonely = set(range(n)) - set(x for p in picked for x in p)
    assert 2 * threads >= len(picked) == 512 > threads and lonely == (set(range(5)) if name == "outliers first" else set(range(1024, n))) and n > step
    for o in lonely:
        (far,) = np.flatnonzero(mat[o] == mat[o].max())
        assert [p[1] for p in picked].index(far) >= threads
    got, rounds = _tree(d, mat, kind)
    assert got == want
    assert sorted(m[:2] for m in got if m[2:4] == (1, 1) and m[4] == 1) == picked
    assert [m[:4] for m in want[-5:-1]] == [(min(lonely), o, k + 1, 1) for k, o in enumerate(sorted(lonely)[1:])]      # the outliers join each other first
    assert 11 <= rounds < n - 1                                      # a cluster at most doubles in a round: 2^10 < 1 029


@pytest.mark.parametrize("kind", lc.KINDS)
def test_a_nearest_neighbour_in_the_last_partial_step(kind):
    """Three rows below 256 whose only 0 is in column 1 280: the second load of the second step, taken by one lane alone."""
    d = get_device()
    step, threads = _lnk_step()
    n = 1281
    assert n - 1 == step + threads
    mat, want = _want("far column", n, kind)
    assert want[0] == (3, n - 1, 1, 1, 0)
    assert _tree(d, mat, kind)[0] == want


# ---- C. cluster SNPs ----------------------------------------------------------------------------------------------------------

def _cs_sizes():
    """(sites of a word tile, rows of a chunk, clusters of a part, waves of a full grid per CU, elements of one block of the cell scan)"""
    src = "cluster_snps.hip"
    waves = ae.define(src, "CS_GRID_CAP_PER_CU") * (ae.define(src, "CS_THREADS") // 64)
    return (ae.define(src, "CS_TILE_WORDS") * 32, ae.define(src, "CS_ROW_CHUNK"), ae.define(src, "CS_CLUSTER_CHUNK"), waves,
            ae.define("prims.h", "PRIM_GSCAN_THREADS") * ae.define("prims.h", "PRIM_GSCAN_ITEMS"))


def _pack(d, sym):
    import torch
    sym_t = torch.from_numpy(np.array(sym, dtype=np.uint8, order="C")).cuda()
    n, s = sym.shape
    pk = torch.full((n, d.packed_row_bytes(s)), BYTE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    d.pack_matrix_dev(sym_t.data_ptr(), n, s, s, pk.data_ptr())
    d.sync()
    return pk


def _counts_dev(d, pk, n, s):
    import torch
    out = torch.full((s * 16 + 64,), BYTE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    d.site_counts_dev(pk.data_ptr(), n, s, out.data_ptr())
    d.sync()
    host = out.cpu().numpy()
    assert (host[s * 16:] == BYTE).all()
    return host[:s * 16].copy().view("<i4").reshape(s, 4)


def _snps_dev(d, pk, n, s, labels, n_clusters):
    """Count, then emit into exactly enough room: (cluster_off, site, base, members); everything behind them keeps the mark."""
    import torch
    lab = torch.from_numpy(np.asarray(labels, dtype=np.int64).astype(np.int32)).cuda()
    torch.cuda.synchronize()
    total = d.cluster_snps_dev(pk.data_ptr(), n, s, lab.data_ptr(), n_clusters, 0)
    c = n_clusters + 1
    off = torch.full((c * 8 + 64,), BYTE, dtype=torch.uint8, device="cuda")
    site, members = (torch.full(((total + 8) * 4,), BYTE, dtype=torch.uint8, device="cuda") for _ in range(2))
    base = torch.full((total + 8,), BYTE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert d.cluster_snps_dev(pk.data_ptr(), n, s, lab.data_ptr(), n_clusters, max(total, 1), off.data_ptr(), site.data_ptr(), base.data_ptr(), members.data_ptr()) == total
    d.sync()
    off, site, base, members = (x.cpu().numpy() for x in (off, site, base, members))
    assert (off[c * 8:] == BYTE).all() and (site[total * 4:] == BYTE).all() and (base[total:] == BYTE).all() and (members[total * 4:] == BYTE).all()
    return off[:c * 8].copy().view("<u8"), site[:total * 4].copy().view("<u4"), base[:total].copy(), members[:total * 4].copy().view("<u4")


def _same(got, want, where):
    for g, w, name in zip(got, want, ("cluster_off", "site", "base", "members")):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (where, name)


def _check(sym, labels, n_clusters, want, where, host_form=False):
    d = get_device()
    n, s = sym.shape
    counts = sc.site_counts(sym)
    assert np.array_equal(want[3], counts[want[1], want[2]])          # every holder of an entry's base is a member
    pk = _pack(d, sym)
    assert np.array_equal(_counts_dev(d, pk, n, s), counts), where
    _same(_snps_dev(d, pk, n, s, labels, n_clusters), want, where)
    if host_form:
        offs, site, base, members = d.cluster_snps(sym, labels, n_clusters=n_clusters, expect=len(want[1]))
        _same((offs[0], site, base, members), want, (where, "host form"))


@pytest.mark.parametrize("mixed", [False, True])
def test_cells_past_the_grid_and_past_the_block_of_the_cell_scan(mixed):
    """33 x CUs + 100 clusters on two word tiles: more (cluster, tile) cells than a full grid has waves — k_presence_zero and both
    forms of k_rows go round their loops — and than one block of the scan that places them.  Once as singletons, once with one
    to three rows per cluster and the rows shuffled — and one of the last cluster numbers without a row, whose presence words
    k_presence_zero alone writes, in its second turn; the rows fill more than 32 chunks of k_sweep, for the site counts too."""
    cus = _cus()
    tile, chunk, _, waves_per_cu, scan_block = _cs_sizes()
    c, s = 33 * cus + 100, 2 * 2048 + 1 - 1497
    assert tile < s <= 2 * tile and waves_per_cu == 64
    assert 2 * c > waves_per_cu * cus and 2 * c > scan_block
    sizes = ae.mixed_sizes(c, 9) if mixed else np.ones(c, dtype=np.int64)
    labels = ae.labels_of_sizes(sizes, seed=5 if mixed else None)
    assert len(labels) > 32 * chunk and (not mixed or (sizes[c - 2] == 0 and 2 * (c - 2) >= waves_per_cu * cus))
    sym = ae.planted_private(labels, c, s, 3)
    want = ae.cluster_snps_fast(sym, labels, c)
    ae.check_large(want, sizes, s, tile, mixed)
    assert want[0][1] >= 1 and (want[1][0], want[2][0]) == (0, 1)      # C at column 0 is cluster 1's: a stray bit in another cluster's presence there takes it away
    _check(sym, labels, c, want, mixed, host_form=not mixed)


@pytest.mark.parametrize("c", [683, 684])
def test_the_block_edge_of_the_cell_scan_alone(c):
    """Three word tiles: 2 049 and 2 052 cells, one and four past a block of the scan."""
    tile, _, _, _, scan_block = _cs_sizes()
    n, s = 700, 2 * 2048 + 700
    assert 2 * tile < s <= 3 * tile and 3 * c in (scan_block + 1, scan_block + 4)
    rng = np.random.default_rng(c)
    labels = np.concatenate([np.arange(1, c + 1), rng.integers(1, c + 1, size=n - c)])[rng.permutation(n)].astype(np.uint32)
    sym = ae.planted_private(labels, c, s, 12)
    want = ae.cluster_snps_fast(sym, labels, c)
    assert len(want[1]) >= 200 and (ae.per_tile(want, tile, 3) >= 20).all() and want[0][-1] > want[0][3 * c // 4]
    _check(sym, labels, c, want, c)


@pytest.mark.parametrize("across", [True, False])
@pytest.mark.parametrize("c", [63, 64, 65, 128, 129])
def test_cluster_counts_at_the_edges_of_the_parts_of_the_unique_pass(c, across):
    """A base that exactly two clusters hold — in the first and the last part (parts 0 and 2 of three at 129 clusters), then in
    one part — defines neither; a base that one cluster of the last, partial part holds alone defines it."""
    _, _, part, _, _ = _cs_sizes()
    assert c in (part - 1, part, part + 1, 2 * part, 2 * part + 1)
    labels, sym, pair, last = ae.chunk_edge_case(c, part, across)
    assert ((pair[0] - 1) // part != (pair[1] - 1) // part) == (across and c > part) and (last - 1) // part == (c - 1) // part
    want = sc.cluster_snps(sym, labels, c)
    found = ae.entries_of(want)
    assert (pair[0], ae.COL_TWICE) not in found and (pair[1], ae.COL_TWICE) not in found
    assert found[(last, ae.COL_ONCE)] == (3, int((labels == last).sum())) and len(found) > 10
    _check(sym, labels, c, want, (c, across))


def test_one_cluster_across_two_chunk_edges():
    """600 of 700 shuffled rows in one cluster: its presence is OR-ed together by the waves of three row chunks, and the 600
    holders of its base carry the counters of two chunks into the ninth plane."""
    _, chunk, _, _, _ = _cs_sizes()
    sizes = [600] + [5] * 20
    assert sizes[0] > 2 * chunk and sum(sizes) <= 3 * chunk
    labels = ae.labels_of_sizes(sizes, seed=21)
    sym = ae.planted_private(labels, len(sizes), 100, 22)
    ae.plant(sym, labels, (1,), 33, 0x47)
    sym[labels != 1, 34] = 0x63                                      # c in everybody else: the A of the background is cluster 1's own, and not all of it hold one
    want = sc.cluster_snps(sym, labels, len(sizes))
    found = ae.entries_of(want)
    assert found[(1, 33)] == (2, 600) and found[(1, 34)][0] == 0 and 256 < found[(1, 34)][1] < 600 and sc.site_counts(sym)[33].tolist() == [0, 0, 600, 0]
    _check(sym, labels, len(sizes), want, "600", host_form=True)
