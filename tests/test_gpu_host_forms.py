"""Every host form of the distance step — the entry points of ``Device`` that take the symbol matrix from host memory — at the
shapes where the preamble they share (upload, pack, matrix, valid plane: ``DevSymbols`` of csrc/distance.hip) can go wrong: no
row; no column, so that nothing is uploaded and the matrix is still zero-filled; one packed group of 128 sites exactly and one
column past it; one row past a 128-row distance tile.  Each answer against the restatements of tests/*_cases.py, each form twice
in a row on one Device: nothing of the first call is left enqueued or kept."""
import numpy as np
import pytest

from tests import clusters_cases as cc
from tests import cluster_snps_cases as sc
from tests import compared_cases as pc
from tests import linkage_cases as lc
from tests import mst_cases as mc
from tests import nearest_cases as nc
from tests import nj_cases as jc
from tests import pair_sites_cases as ps
from tests.gpu_util import get_device

pytestmark = pytest.mark.gpu

SHAPES = ((0, 0), (0, 5), (1, 0), (1, 7), (2, 0), (3, 128), (3, 129), (129, 33))
LETTERS = np.frombuffer(b"ACGTACGTacgt-N", dtype=np.uint8)


def symbols(n, s, seed):
    """Rows a few sites from a common base, so that thresholds and trees have something to tell apart."""
    rng = np.random.default_rng(seed)
    sym = np.tile(rng.choice(LETTERS[:4], size=s), (n, 1)).reshape(n, s)
    flips = rng.random((n, s)) < 0.2
    sym[flips] = rng.choice(LETTERS, size=int(flips.sum()))
    return np.ascontiguousarray(sym)


def expected(sym, query):
    """What every form has to return for these symbols, from the restatements alone."""
    n, s = sym.shape
    mat = nc.rect_distance(sym, sym)
    t = int(np.median(mat)) if n else 0
    a = np.asarray([0, n - 1, n // 2, 0][:4 if n else 0], dtype=np.uint32)
    b = np.asarray([n - 1, 0, n // 2, n // 2][:4 if n else 0], dtype=np.uint32)
    labels = (np.arange(n, dtype=np.uint32) * 7 % 3 % max(n, 1)) + 1
    labels = np.unique(labels, return_inverse=True)[1].astype(np.uint32) + 1       # every number from 1 to the largest is used
    want = {"mat": mat, "t": t, "a": a, "b": b, "labels": labels}
    want["csr"] = cc.filter_rows(mat, t)
    want["tree"] = mc.arrays(mc.mst_of_matrix(mat) if n > 1 else [])
    for kind in ("complete", "average"):
        want[kind] = lc.arrays(lc.rounds(mat, kind)[0] if n > 1 else [])
    want["nj"] = jc.nj_numpy(mat)
    want["sites"] = ps.pair_sites(sym, a, b)
    want["compared"] = pc.compared_rect(sym, sym)
    want["compared_pairs"] = pc.compared_pairs(sym, a, b)
    qa = np.asarray([0, len(query) - 1][:2 if n else 0], dtype=np.uint32)
    want["qa"], want["qb"] = qa, b[:len(qa)]
    want["compared_two"] = pc.compared_pairs(query, qa, b[:len(qa)], sym)
    want["counts"] = sc.site_counts(sym)
    want["snps"] = sc.cluster_snps(sym, labels, int(labels.max()) if n else 0)
    want["nearest"] = nc.nearest_of_matrix(nc.rect_distance(query, sym), 2, None)
    return want


def same(got, want):
    return len(got) == len(want) and all(np.array_equal(g, w) and np.asarray(g).dtype == np.asarray(w).dtype for g, w in zip(got, want))


@pytest.mark.parametrize("n,s", SHAPES)
def test_every_host_form(n, s):
    from snp_pipeline_amd.device import SnpGpuError
    d = get_device()
    sym, other, query = symbols(n, s, 100 * n + s), symbols(n, s, 100 * n + s + 1), symbols(2, s, 100 * n + s + 2)
    w = expected(sym, query)
    mat, t, a, b = w["mat"], w["t"], w["a"], w["b"]
    for again in range(2):
        where = (n, s, again)
        assert same([d.distance(sym)], [mat]), where
        assert same(d.close_pairs(sym, t), w["csr"]) and same(d.close_pairs(sym, t, want_matrix=True), w["csr"] + (mat,)), where
        assert same(d.mst(sym), w["tree"]) and same(d.mst(sym, want_matrix=True), w["tree"] + (mat,)), where
        got = d.mst(sym, pairs_within=t)
        assert same(got[:3], w["tree"]) and same(got[3], w["csr"]), where
        tree, csr, m = d.distance_outputs(sym, want_tree=True, want_matrix=True, pairs_within=t)
        assert same(tree, w["tree"]) and same(csr, w["csr"]) and same([m], [mat]), where
        assert d.distance_outputs(sym) == (None, None, None), where
        for kind in ("complete", "average"):
            assert same(d.linkage(sym, kind), w[kind]) and same(d.linkage(sym, kind, want_matrix=True), w[kind] + (mat,)), where
            assert same(d.linkage_of_matrix(mat, kind), w[kind]), where
        assert jc.tree_of_arrays(*d.nj(sym)) == w["nj"], where
        got = d.nj(sym, want_matrix=True)
        assert jc.tree_of_arrays(*got[:6]) == w["nj"] and same(got[6:], [mat]), where
        assert same(d.pair_sites(sym, a, b), w["sites"]) and same(d.pair_sites(sym, a, b, expect=len(w["sites"][1])), w["sites"]), where
        assert same([d.compared(sym)], [w["compared"]]) and same([d.compared_pairs(sym, a, b)], [w["compared_pairs"]]), where
        assert same([d.compared_pairs(query, w["qa"], w["qb"], sym)], [w["compared_two"]]), where
        assert same([d.site_counts(sym)], [w["counts"]]), where
        off, site, base, members = d.cluster_snps(sym, w["labels"])
        assert len(off) == 1 and same((off[0], site, base, members), w["snps"]), where
        assert same(d.nearest(query, sym, k=2), w["nearest"]), where
        # the packed matrix a call keeps is the one of THAT call, and it goes with packed_drop
        with pytest.raises(SnpGpuError):
            d.pair_sites_kept(a, b)
        tree, csr, m = d.distance_outputs(other, want_tree=True, pairs_within=t, keep_packed=True)
        assert m is None and same(tree, mc.arrays(mc.mst_of_matrix(nc.rect_distance(other, other)) if n > 1 else [])), where
        if n:
            assert same(d.pair_sites_kept(a, b), ps.pair_sites(other, a, b)), where
            tree, csr, m = d.distance_outputs(sym, want_matrix=True, keep_packed=True)
            assert tree is None and csr is None and same([m], [mat]), where
            assert same(d.pair_sites_kept(a, b), w["sites"]) and same(d.pair_sites_kept(a, b, expect=len(w["sites"][1])), w["sites"]), where
        d.packed_drop()
        d.packed_drop()
        with pytest.raises(SnpGpuError):
            d.pair_sites_kept(a, b)
