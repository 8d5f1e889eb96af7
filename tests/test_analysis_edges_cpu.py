"""The generators and restatements of tests/analysis_edge_cases.py pinned against the plain statements they stand in for
(tests/clusters_cases.py, tests/linkage_cases.py, tests/cluster_snps_cases.py), and the properties the GPU tests rely on: that the
restatement of the cluster SNPs is sc.cluster_snps, that the wide linkage round has 512 merges and five bystanders, and that the
constructed cluster-SNP inputs have entries where the kernels' later turns look.  No GPU."""
import numpy as np
import pytest

from tests import analysis_edge_cases as ae
from tests import cluster_snps_cases as sc
from tests import linkage_cases as lc

CUS = 256                                                           # an MI355X, as an example: the GPU test asks the device


def _same(got, want, where):
    for g, w, name in zip(got, want, ("cluster_off", "site", "base", "members")):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (where, name)


# ---- A ------------------------------------------------------------------------------------------------------------------------

def test_a_small_forest_is_what_it_says_and_union_find_is_reachability():
    n, hub = 300, 150
    u, v, w, lonely = ae.forest(n, 20, 3, gaps=(100, 200), gap_half=5, hub=hub, hub_degree=70, long_every=6)
    row_off, col, dist = csr = ae.csr_of_edges(n, u, v, w)
    assert len(col) == len(dist) == 2 * len(u) == row_off[-1] and set(w.tolist()) == {1, 9}
    assert len(lonely) == 20 and all(row_off[i] == row_off[i + 1] for i in lonely)
    assert row_off[hub + 1] - row_off[hub] > 64                      # more entries than a wave has lanes
    dense = np.full((n, n), -1, dtype=np.int64)
    for i in range(n):
        cols = col[int(row_off[i]):int(row_off[i + 1])].astype(np.int64)
        assert (np.diff(cols) >= 0).all() and i not in cols.tolist()
        dense[i, cols] = dist[int(row_off[i]):int(row_off[i + 1])]
    assert np.array_equal(dense, dense.T)                            # both directions of every edge
    for t in (0, 5, 9):
        numbers = ae.numbers_by_union_find(n, u, v, w, t)
        assert np.array_equal(numbers, ae.numbers_by_reach(n, csr, t)), t
    few, all_of = ae.numbers_by_union_find(n, u, v, w, 5), ae.numbers_by_union_find(n, u, v, w, 9)
    assert all_of.max() < few.max() < n and (np.bincount(all_of)[all_of[lonely]] == 1).all()


def test_the_large_forest_passes_what_the_gpu_test_says_it_passes():
    n = 600000
    u, v, w, lonely = ae.forest(n, 1000, 24, gaps=(8192, 524288), gap_half=75, hub=n // 2)
    row_off, col, dist = ae.csr_of_edges(n, u, v, w)
    assert len(col) > 2 * 524288 and 200 <= len(lonely) <= 400
    assert lonely.min() < 8192 < lonely.max() and (lonely < 524288).any() and (lonely > 524288).any()
    assert row_off[n // 2 + 1] - row_off[n // 2] > 64
    assert 0.01 < (w == 9).mean() < 0.03
    assert np.bincount(np.concatenate([u, v]), minlength=n).max() == row_off[n // 2 + 1] - row_off[n // 2]


def test_extreme_edges_hold_both_ends_of_int32_and_both_signs():
    u, v, w = ae.extreme_edges(300, 11)
    assert (w == ae.INT_MIN).sum() >= 50 and (w == ae.INT_MAX).sum() >= 50 and ((w < 0) & (w > ae.INT_MIN)).any() and (w == 0).any()
    csr = ae.csr_of_edges(300, u, v, w)
    counts = [int(ae.numbers_by_reach(300, csr, t).max()) for t in (ae.INT_MIN, -1, ae.INT_MAX)]
    assert 300 > counts[0] > counts[1] > counts[2] >= 1
    for t in (ae.INT_MIN, -1, ae.INT_MAX):
        assert np.array_equal(ae.numbers_by_reach(300, csr, t), ae.numbers_by_union_find(300, u, v, w, t))


# ---- B ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("kind", lc.KINDS)
def test_the_wide_round_has_512_merges_and_five_bystanders(kind, first):
    mat = ae.xor_with_outliers(1024, 5, 1, first, ae.BETWEEN[kind])
    assert mat.shape == (1029, 1029) and np.array_equal(mat, mat.T)
    lo = 5 if first else 0
    outliers = list(range(5)) if first else list(range(1024, 1029))
    picked = ae.first_round(mat, kind)
    assert len(picked) == 512 and picked == [(lo + i, lo + i + 1) for i in range(0, 1024, 2)]
    assert not set(outliers) & set(x for p in picked for x in p)
    assert all(5000 <= mat[o, k] < 5050 for o in outliers for k in range(1029) if k != o)
    threads = ae.define("linkage.hip", "LNK_THREADS")
    for k, o in enumerate(outliers):                                 # the one largest entry: against the sample that retires in merge 511 - k
        assert np.flatnonzero(mat[o] == mat[o].max()).tolist() == [lo + 1023 - 2 * k] and picked[511 - k][1] == lo + 1023 - 2 * k and 511 - k >= threads
    # once the block is one cluster, every outlier is nearer to the other outliers than to it — and would not be without the
    # entries against the samples that retire in the merges past the first LNK_THREADS of the round
    block = [k for k in range(1029) if k not in outliers]
    late = [j for _, j in picked[threads:]]
    for o in outliers:
        whole, rest = mat[o, block].astype(np.int64), np.delete(mat[o].astype(np.int64), outliers + late)
        to_block, without = (whole.max(), rest.max()) if kind == "complete" else (whole.sum() / 1024.0, rest.sum() / 1024.0)
        assert without < 5000 + ae.BETWEEN[kind] < to_block


@pytest.mark.parametrize("kind", lc.KINDS)
def test_first_round_is_the_first_round_of_the_round_form(kind):
    """On a matrix small enough to follow: the picked pairs are the merges of singletons that lc.rounds reports when it is stopped
    after one round — here a matrix whose first round is its only one."""
    mat = ae.xor_with_outliers(2, 0, 1, False)
    assert ae.first_round(mat, kind) == [(0, 1)] and lc.rounds(mat, kind) == ([(0, 1, 1, 1, 1)], 1)
    mat = ae.xor_with_outliers(16, 3, 2, True)
    picked = ae.first_round(mat, kind)
    merges, _ = lc.rounds(mat, kind)
    assert [(a, b) for a, b, sa, sb, _ in merges if sa == sb == 1 and mat[a, b] == 1] == picked == [(3 + i, 4 + i) for i in range(0, 16, 2)]
    assert merges == lc.greedy(mat, kind)


def test_a_column_planted_past_the_first_step():
    mat = lc.random_matrix(1281, 1281, high=40)
    far = ae.planted_far_column(mat, (3, 100, 255))
    assert np.array_equal(far, far.T) and (far[:1280, :1280] == mat[:1280, :1280] + 1 - np.eye(1280, dtype=np.int32)).all()
    size, live = np.ones(1281, dtype=np.int64), np.ones(1281, dtype=bool)
    for kind in lc.KINDS:                                            # (a 0 at a smaller column would come first: no row has one)
        assert [lc.nearest(far.astype(np.int64), size, live, kind, r) for r in (3, 100, 255, 1280)] == [1280, 1280, 1280, 3]
        assert (3, 1280) in ae.first_round(far, kind)


# ---- C ------------------------------------------------------------------------------------------------------------------------

def test_the_restatement_is_the_statement_on_every_labelling():
    n, s = 300, 2100
    labs = sc.labellings(n, 5)
    sym = sc.planted_symbols(n, s, labs["planted"], 77)
    total = 0
    for name, labels in labs.items():
        c = int(labels.max())
        want = sc.cluster_snps(sym, labels, c)
        _same(ae.cluster_snps_fast(sym, labels, c), want, name)
        _same(ae.cluster_snps_fast(sym, labels, c, block=s + 9), want, (name, "one block"))
        total += len(want[1])
    assert total > 1000
    # cluster numbers that no row carries: in the middle and at the end
    labels = labs["planted"].copy()
    gone = int(labels[0])
    labels[labels == gone] = gone + 1 if gone < labels.max() else gone - 1
    c = int(labs["planted"].max()) + 2
    want = sc.cluster_snps(sym, labels, c)
    assert want[0][gone] == want[0][gone - 1] and want[0][-1] == want[0][-3] and len(want[1]) > 0
    _same(ae.cluster_snps_fast(sym, labels, c), want, "empty numbers")
    _same(ae.cluster_snps_fast(sym[:0], labels[:0], 3), sc.cluster_snps(sym[:0], labels[:0], 3), "no rows")


def test_the_restatement_is_the_statement_on_the_constructed_input():
    rng = np.random.default_rng(4)
    c = 90
    labels = ae.labels_of_sizes(rng.integers(1, 4, size=c), seed=6)
    sym = ae.planted_private(labels, c, 150, 8)
    assert set(np.unique(sym).tolist()) <= set(b"AaCcGgTt-N")
    want = sc.cluster_snps(sym, labels, c)
    _same(ae.cluster_snps_fast(sym, labels, c), want, "constructed")
    found = ae.entries_of(want)
    sizes = sc.sizes_of(labels, c)
    plants = ae.private_plants(c, 150)
    assert len(plants) == 30 and plants[0][0] == 1 and plants[-1][0] == 88
    repeated = set(plants[k][1:] for k in range(len(plants)) if k % 50 == 49)
    for cluster, col, base in plants:                               # every plant is an entry of its cluster alone, but for the repeated pairs
        if (col, base) in repeated:
            assert (cluster, col) not in found
        else:
            got = found.pop((cluster, col))
            assert got[0] == base and got[1] in (sizes[cluster - 1], sizes[cluster - 1] - 1) and got[1] >= 1
    assert not found                                                 # and nothing else is: the background holds A alone, everywhere


@pytest.mark.parametrize("mixed", [False, True])
def test_the_large_input_has_entries_where_the_later_turns_look(mixed):
    c, s, tile = 33 * CUS + 100, 2600, 2048
    sizes = ae.mixed_sizes(c, 9) if mixed else np.ones(c, dtype=np.int64)
    labels = ae.labels_of_sizes(sizes, seed=5 if mixed else None)
    sym = ae.planted_private(labels, c, s, 3)
    want = ae.cluster_snps_fast(sym, labels, c)
    assert np.array_equal(sc.sizes_of(labels, c), sizes) and (sizes[c - 2] == 0) == mixed
    ae.check_large(want, sizes, s, tile, mixed)
    assert want[0][1] >= 1 and (want[1][0], want[2][0]) == (0, 1) and want[0][c - 1] == want[0][c - 2]
    plants = ae.private_plants(c, s)
    assert len(set(p[1:] for p in plants)) == len(plants) - len(plants) // 50        # injective but for the repeats
    # the statement itself on two of the clusters that have entries, the last planted one among them: everybody else as a third
    one, other = 4, int(np.flatnonzero(np.diff(want[0].astype(np.int64)))[-1]) + 1
    assert other > c - 9
    three = np.where(labels == one, 1, np.where(labels == other, 2, 3)).astype(np.uint32)
    lone = sc.cluster_snps(sym, three, 3)
    for k, cluster in enumerate((one, other)):
        mine, its = slice(int(lone[0][k]), int(lone[0][k + 1])), slice(int(want[0][cluster - 1]), int(want[0][cluster]))
        assert lone[0][k + 1] > lone[0][k] and all(lone[x][mine].tolist() == want[x][its].tolist() for x in (1, 2, 3)), cluster


@pytest.mark.parametrize("c", [63, 64, 65, 128, 129])
def test_a_base_held_by_two_clusters_and_one_held_by_the_last(c):
    for across in (True, False):
        labels, sym, pair, last = ae.chunk_edge_case(c, 64, across)
        assert ((pair[0] - 1) // 64 != (pair[1] - 1) // 64) == (across and c > 64) and (last - 1) // 64 == (c - 1) // 64
        if c == 129 and across:
            assert ((pair[0] - 1) // 64, (pair[1] - 1) // 64) == (0, 2)
        want = sc.cluster_snps(sym, labels, c)
        _same(ae.cluster_snps_fast(sym, labels, c), want, (c, across))
        found = ae.entries_of(want)
        assert (pair[0], ae.COL_TWICE) not in found and (pair[1], ae.COL_TWICE) not in found
        assert found[(last, ae.COL_ONCE)] == (3, int((labels == last).sum())) and len(found) > 10
