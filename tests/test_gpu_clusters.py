"""Kernel (b) of csrc/clusters.hip — connected components of a thresholded CSR at several thresholds in one call, and the
numbering of the clusters — against the reachability statement of tests/clusters_cases.py (small graphs) and a union-find or
SciPy (large ones)."""
import os

import numpy as np
import pytest

from tests import clusters_cases as cc
from tests.gpu_util import get_device

pytestmark = pytest.mark.gpu


def _csr_of_edges(n, edges, both=True, diagonal=False):
    """edges: (u, v, d).  Row u lists v (and row v lists u when `both`), columns ascending, as kernel (a) writes them."""
    rows = [[] for _ in range(n)]
    for u, v, w in edges:
        rows[u].append((v, w))
        if both:
            rows[v].append((u, w))
    if diagonal:
        for i in range(n):
            rows[i].append((i, 0))
    row_off = np.zeros(n + 1, dtype=np.uint64)
    col, dist = [], []
    for i, r in enumerate(rows):
        r.sort()
        row_off[i + 1] = row_off[i] + len(r)
        col += [c for c, _ in r]
        dist += [w for _, w in r]
    return row_off, np.asarray(col, dtype=np.uint32), np.asarray(dist, dtype=np.int32)


def _want_small(n, csr, threshold):
    return cc.numbers_of_labels(cc.labels_of_reach(cc.reach(cc.adjacency(n, csr[0], csr[1], csr[2], threshold))))


def _want_large(n, edges, threshold):
    return cc.numbers_of_labels(cc.union_find_labels(n, [(u, v) for u, v, w in edges if w <= threshold]))


def _run(d, n, csr, thresholds):
    numbers, counts = d.clusters(n, csr[0], csr[1], csr[2], thresholds)
    assert numbers.shape == (len(thresholds), n) and counts.shape == (len(thresholds),)
    for t in range(len(thresholds)):
        assert counts[t] == (numbers[t].max() if n else 0)
    return numbers.astype(np.int64), counts


def test_nothing_one_node_and_no_edges():
    d = get_device()
    empty = (np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.int32))
    numbers, counts = _run(d, 0, empty, [0, 5])
    assert numbers.shape == (2, 0) and counts.tolist() == [0, 0]
    numbers, counts = _run(d, 1, (np.zeros(2, np.uint64), empty[1], empty[2]), [3])
    assert numbers.tolist() == [[1]] and counts.tolist() == [1]
    numbers, counts = _run(d, 1, (np.array([0, 1], np.uint64), np.zeros(1, np.uint32), np.zeros(1, np.int32)), [0])
    assert numbers.tolist() == [[1]] and counts.tolist() == [1]
    n = 300
    numbers, counts = _run(d, n, (np.zeros(n + 1, np.uint64), empty[1], empty[2]), [0, 9])
    assert counts.tolist() == [n, n] and np.array_equal(numbers[0], np.arange(1, n + 1)) and np.array_equal(numbers[1], numbers[0])
    numbers, counts = _run(d, n, _csr_of_edges(n, [], diagonal=True), [0])           # only the diagonal
    assert counts.tolist() == [n] and np.array_equal(numbers[0], np.arange(1, n + 1))
    numbers, counts = _run(d, 5, (np.zeros(6, np.uint64), empty[1], empty[2]), [])
    assert numbers.shape == (0, 5) and counts.shape == (0,)


def test_complete_graph_and_star():
    d = get_device()
    n = 150
    full = _csr_of_edges(n, [(u, v, 4) for u in range(n) for v in range(u + 1, n)], diagonal=True)
    numbers, counts = _run(d, n, full, [3, 4])
    assert counts.tolist() == [n, 1] and (numbers[1] == 1).all() and np.array_equal(numbers[0], np.arange(1, n + 1))
    for centre in (0, 77, n - 1):
        star = _csr_of_edges(n, [(centre, v, 2) for v in range(n) if v != centre])
        numbers, counts = _run(d, n, star, [1, 2])
        assert counts.tolist() == [n, 1] and (numbers[1] == 1).all()
        assert np.array_equal(numbers[1], _want_small(n, star, 2)) and np.array_equal(numbers[0], _want_small(n, star, 1))


def test_a_long_path_with_scrambled_numbering():
    """5 000 nodes in a chain whose order along the chain is a seeded permutation of their indices: no fixed number of rounds and
    no single pass over the edges gets every label down to the smallest index of its piece.  Three links are too long for the
    smaller threshold: four pieces there, one at the larger."""
    d = get_device()
    n = 5000
    perm = np.random.default_rng(2024).permutation(n)
    edges = [(int(perm[i]), int(perm[i + 1]), 9 if i in (700, 2500, 4100) else 1) for i in range(n - 1)]
    for both in (True, False):
        csr = _csr_of_edges(n, edges, both=both)
        numbers, counts = _run(d, n, csr, [5, 9])
        assert counts.tolist() == [4, 1]
        assert np.array_equal(numbers[0], _want_large(n, edges, 5)) and (numbers[1] == 1).all()
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        return
    short = [(u, v) for u, v, w in edges if w <= 5]
    g = coo_matrix((np.ones(len(short)), ([u for u, _ in short], [v for _, v in short])), shape=(n, n))
    n_comp, lab = connected_components(g, directed=False)
    assert n_comp == 4 and len(set(zip(lab.tolist(), numbers[0].tolist()))) == 4


def test_two_cliques_joined_by_one_edge_at_the_threshold():
    d = get_device()
    a, b, t = 40, 55, 17
    n = a + b
    edges = [(u, v, 2) for u in range(a) for v in range(u + 1, a)] + [(u, v, 3) for u in range(a, n) for v in range(u + 1, n)]
    edges.append((a - 1, a + 7, t))
    csr = _csr_of_edges(n, edges, diagonal=True)
    numbers, counts = _run(d, n, csr, [t - 1, t, t + 1])
    assert counts.tolist() == [2, 1, 1]
    assert numbers[0].tolist() == [1] * a + [2] * b and (numbers[1] == 1).all() and (numbers[2] == 1).all()
    for k, thr in enumerate((t - 1, t, t + 1)):
        assert np.array_equal(numbers[k], _want_small(n, csr, thr))


def test_six_thresholds_in_one_call_coarsen():
    d = get_device()
    n = 280
    rng = np.random.default_rng(6)
    edges = [(int(u), int(v), int(w)) for u, v, w in zip(rng.integers(0, n, 420), rng.integers(0, n, 420), rng.integers(0, 60, 420)) if u != v]
    thresholds = [0, 5, 10, 20, 40, 59]
    for both, diagonal in ((True, True), (True, False), (False, False)):          # what kernel (a) writes; no diagonal; one direction only
        csr = _csr_of_edges(n, edges, both=both, diagonal=diagonal)
        numbers, counts = _run(d, n, csr, thresholds)
        for k, t in enumerate(thresholds):
            assert np.array_equal(numbers[k], _want_small(n, csr, t)), (both, diagonal, t)
        assert counts.tolist() == sorted(counts.tolist(), reverse=True) and counts[0] > counts[-1]
        for k in range(1, len(thresholds)):                                 # every cluster of the finer threshold lies inside one of the coarser
            assert len(set(zip(numbers[k - 1].tolist(), numbers[k].tolist()))) == counts[k - 1]
    # thresholds in any order and repeated: each column answers its own threshold
    csr = _csr_of_edges(n, edges)
    numbers, _ = _run(d, n, csr, [40, 0, 40])
    assert np.array_equal(numbers[0], numbers[2]) and np.array_equal(numbers[0], _want_small(n, csr, 40)) and np.array_equal(numbers[1], _want_small(n, csr, 0))


def test_device_form_on_what_kernel_a_writes():
    import torch
    d = get_device()
    n = 200
    rng = np.random.default_rng(8)
    mat = rng.integers(0, 400, size=(n, n)).astype(np.int32)
    mat = np.minimum(mat, mat.T)
    np.fill_diagonal(mat, 0)
    t_mat = torch.from_numpy(mat).cuda()
    torch.cuda.synchronize()
    total = d.close_pairs_dev(t_mat.data_ptr(), n, n, 0, n, 6)
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    col = torch.zeros(total, dtype=torch.int32, device="cuda")
    dist = torch.zeros(total, dtype=torch.int32, device="cuda")
    out = torch.zeros((3, n), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    d.close_pairs_dev(t_mat.data_ptr(), n, n, 0, n, 6, total, off.data_ptr(), col.data_ptr(), dist.data_ptr())
    counts = d.clusters_dev(n, off.data_ptr(), col.data_ptr(), dist.data_ptr(), total, [1, 3, 6], out.data_ptr())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for k, t in enumerate((1, 3, 6)):
        want = cc.cluster_numbers(mat, t)
        assert np.array_equal(got[k], want) and counts[k] == want.max()
    assert 1 < counts[2] < counts[0] < n


def test_listeria_end_to_end(fixture_trees):
    from snp_pipeline_amd import distance, snp_matrix
    d = get_device()
    tree = fixture_trees["listeria"][0]
    file_ids, sym, lens = snp_matrix.load_matrix(os.path.join(tree, "snpma.fasta"))
    thresholds = sorted(cc.LISTERIA_COUNTS)
    ids, row_off, col, dist = distance.close_pairs_of_matrix(d, file_ids, sym, lens, max(thresholds))
    want_ids, mat = cc.read_matrix_tsv(os.path.join(tree, "snp_distance_matrix.tsv"))
    assert ids == want_ids and len(ids) == 48
    want = cc.filter_rows(mat, max(thresholds))
    assert np.array_equal(row_off, want[0]) and np.array_equal(col, want[1]) and np.array_equal(dist, want[2])
    numbers, counts = d.clusters(len(ids), row_off, col, dist, thresholds)
    got = {}
    for k, t in enumerate(thresholds):
        pairs = (int((dist <= t).sum()) - len(ids)) // 2
        got[t] = (pairs, int(counts[k]))
        assert np.array_equal(numbers[k], cc.cluster_numbers(mat, t)), t
    assert got == {0: (98, 23), 2: (246, 9), 5: (290, 6), 10: (512, 3), 20: (531, 3), 50: (841, 2)}
