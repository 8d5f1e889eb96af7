"""The kernels of csrc/mst.hip — the minimum spanning forest of a row range of a device distance matrix — through snpgpu_mst_dev
against the Kruskal and Boruvka statements of tests/mst_cases.py: edges, their order and the round count must be equal."""
import functools
import os
import re

import numpy as np
import pytest

from tests import mst_cases as mc
from tests.gpu_util import get_device

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARK = 0x5A5A5A5A


def _on_device(mat, stride, lo=0, hi=None, pad=0, shift=0):
    """Rows [lo, hi) of the matrix with a row pitch of `stride` (`pad` in the padding), `shift` int32 elements into an allocation
    that holds nothing else: (tensor, where row 0 WOULD lie)."""
    import torch
    n = mat.shape[0]
    hi = n if hi is None else hi
    host = np.full(shift + (hi - lo) * stride + 4, pad, dtype=np.int32)
    if hi > lo:
        host[shift:shift + (hi - lo) * stride].reshape(hi - lo, stride)[:, :n] = mat[lo:hi]
    t = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    return t, t.data_ptr() + 4 * shift - 4 * lo * stride


def _forest(d, mat, stride=None, lo=0, hi=None, pad=0, shift=0):
    """(edges [(d, u, v)], rounds, raw bytes of the three arrays) of rows [lo, hi); what lies behind the edges must stay untouched."""
    import torch
    n = mat.shape[0]
    hi = n if hi is None else hi
    stride = n if stride is None else stride
    keep, ptr = _on_device(mat, stride, lo, hi, pad, shift)
    out = [torch.full((max(n - 1, 0) + 8,), MARK, dtype=torch.int32, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    k, rounds = d.mst_dev(ptr, n, stride, lo, hi, *(o.data_ptr() for o in out))
    torch.cuda.synchronize()
    u, v, dist = (o.cpu().numpy() for o in out)
    assert k <= max(n - 1, 0)
    assert (u[k:] == MARK).all() and (v[k:] == MARK).all() and (dist[k:] == MARK).all()
    del keep
    return mc.edges_of_arrays(u[:k].view(np.uint32), v[:k].view(np.uint32), dist[:k]), rounds, b"".join(a.tobytes() for a in (u, v, dist))


@functools.lru_cache(maxsize=None)
def _want(kind, n, lo=0, hi=None):
    """(matrix, Kruskal's forest, Boruvka's round count) of rows [lo, hi), computed once."""
    mat = {"random": lambda: mc.random_matrix(n, n), "xor": lambda: mc.xor_matrix(n), "tie": lambda: mc.seeded_matrix(n, 17),
           "zero": lambda: np.zeros((n, n), dtype=np.int32)}[kind]()
    mat.setflags(write=False)
    forest, rounds = mc.boruvka(mat, lo, hi)
    assert forest == mc.mst_of_matrix(mat, lo, hi)
    return mat, forest, rounds


@pytest.mark.parametrize("n", [0, 1, 2, 3, 63, 64, 65, 129, 300, 1100])
def test_sizes(n):
    src = open(os.path.join(ROOT, "snp_pipeline_amd", "csrc", "mst.hip")).read()
    assert int(re.search(r"#define MST_ROW_GRID_CAP (\d+)", src).group(1)) == 1024          # 1100 rows go round the grid-stride loop
    d = get_device()
    mat, want, want_rounds = _want("random", n)
    got, rounds, _ = _forest(d, mat)
    assert got == want and len(got) == max(n - 1, 0)
    assert rounds == want_rounds <= mc.ceil_log2(n)
    if 2 < n <= 300:                                                 # a pitch of the next multiple of 128, a base off the 16-byte grid
        for stride, shift in (((n + 127) // 128 * 128, 0), (n, 1), (n + 1, 3)):
            assert _forest(d, mat, stride=stride, shift=shift)[:2] == (want, want_rounds), (stride, shift)


def test_xor_matrix_pairs_components_up_round_by_round():
    d = get_device()
    mat, want, want_rounds = _want("xor", 300)
    got, rounds, _ = _forest(d, mat)
    assert got == want and mc.weight(got) == 593 and rounds == want_rounds == 8
    _, band, band_rounds = _want("xor", 300, 128, 256)
    got, rounds, _ = _forest(d, mat, lo=128, hi=256)
    assert got == band and rounds == band_rounds == 7


def test_ties_are_decided_by_the_sample_indices():
    d = get_device()
    mat, want, want_rounds = _want("tie", 300)
    assert [e[0] for e in want] == [1] * 299
    got, rounds, _ = _forest(d, mat)
    assert got == want and rounds == want_rounds <= 9
    zero, star, _ = _want("zero", 300)
    got, rounds, _ = _forest(d, zero)
    assert got == star == [(0, 0, j) for j in range(1, 300)] and rounds == 1


def test_the_largest_distance_is_an_edge_like_any_other():
    d = get_device()
    n = 65
    mat = np.full((n, n), mc.INT_MAX, dtype=np.int32)               # every edge at 2^31 - 1: the empty slot must not be mistaken for one
    np.fill_diagonal(mat, 0)
    got, rounds, _ = _forest(d, mat)
    assert got == [(mc.INT_MAX, 0, j) for j in range(1, n)] and rounds == 1
    mat = mc.random_matrix(n, 5, high=50)
    mat[40:, :40] = mat[:40, 40:] = mc.INT_MAX                      # two groups that only such edges join
    mat[7, 50] = mat[50, 7] = mc.INT_MAX - 1
    mat[0, :] = mat[:, 0] = mc.INT_MAX                               # and a sample that has nothing else
    mat[0, 0] = 0
    want, want_rounds = mc.boruvka(mat)
    assert want == mc.mst_of_matrix(mat) and want[-2:] == [(mc.INT_MAX - 1, 7, 50), (mc.INT_MAX, 0, 1)]
    got, rounds, _ = _forest(d, mat)
    assert got == want and rounds == want_rounds


def test_padding_and_diagonal_never_win():
    d = get_device()
    for n in (65, 129):
        mat = np.array(_want("random", n)[0])
        want, want_rounds = _want("random", n)[1:]
        np.fill_diagonal(mat, -5)
        for stride in (n + 1, (n + 127) // 128 * 128 + 128):
            got, rounds, _ = _forest(d, mat, stride=stride, pad=-1)
            assert got == want and rounds == want_rounds, (n, stride)
            got, rounds, _ = _forest(d, mat, stride=stride, pad=-1, lo=n // 2, hi=n - 1)
            assert got == mc.mst_of_matrix(mat, n // 2, n - 1), (n, stride)


@pytest.mark.parametrize("kind", ["random", "xor", "tie"])
def test_bands(kind):
    d = get_device()
    n = 300
    mat, tree, _ = _want(kind, n)
    merged = []
    for lo, hi in ((0, n), (128, 256), (256, 300), (7, 8), (5, 5)):
        _, want, want_rounds = _want(kind, n, lo, hi)
        for stride in (n, 384):
            got, rounds, _ = _forest(d, mat, stride=stride, lo=lo, hi=hi)
            assert got == want and len(got) == (n - 1 if hi > lo else 0), (lo, hi, stride)
            assert rounds == want_rounds <= mc.ceil_log2(n), (lo, hi, stride)
        if (lo, hi) != (0, n):
            merged += got
    first, _, _ = _forest(d, mat, lo=0, hi=128)
    from snp_pipeline_amd import distance
    assert mc.edges_of_arrays(*distance.mst_of_edges(n, *mc.arrays(first + merged))) == tree


def test_two_runs_give_the_same_bytes():
    d = get_device()
    for kind, lo, hi in (("tie", 0, 300), ("random", 0, 300), ("tie", 128, 256)):
        mat = _want(kind, 300)[0]
        a = _forest(d, mat, lo=lo, hi=hi)
        b = _forest(d, mat, lo=lo, hi=hi)
        assert a[0] and a[2] == b[2] and a[1] == b[1]


def test_bad_arguments_are_refused_before_anything_runs():
    import torch
    from snp_pipeline_amd.device import SnpGpuError
    d = get_device()
    n = 65
    keep, ptr = _on_device(_want("random", n)[0], n)
    out = torch.zeros(3 * n, dtype=torch.int32, device="cuda")
    o = [out.data_ptr() + 4 * n * k for k in range(3)]
    for args in ((n, n - 1, 0, n), (n, n, 5, 4), (n, n, 0, n + 1)):
        with pytest.raises(SnpGpuError):
            d.mst_dev(ptr, args[0], args[1], args[2], args[3], *o)
    with pytest.raises(SnpGpuError):
        d.mst_dev(ptr + 2, n, n, 0, n, *o)
    with pytest.raises(SnpGpuError):
        d.mst_dev(ptr, n, n, 0, n)
    assert d.mst_dev(0, n, n, 3, 3) == (0, 0) and d.mst_dev(ptr, 1, 1, 0, 1) == (0, 0)
    torch.cuda.synchronize()
    del keep


def test_host_form_on_the_listeria_matrix(fixture_trees):
    from snp_pipeline_amd import distance, snp_matrix
    from tests import clusters_cases as cc
    d = get_device()
    tree_dir = fixture_trees["listeria"][0]
    ids, mat = cc.read_matrix_tsv(os.path.join(tree_dir, "snp_distance_matrix.tsv"))
    want = mc.mst_of_matrix(mat)
    assert mc.weight(want) == 9986
    loaded = snp_matrix.load_matrix(os.path.join(tree_dir, "snpma.fasta"))
    got = distance.mst_of_matrix(d, *loaded)
    assert len(got) == 4 and got[0] == ids and mc.edges_of_arrays(*got[1:4]) == want
    both = distance.mst_of_matrix(d, *loaded, want_matrix=True)
    assert len(both) == 5 and mc.edges_of_arrays(*both[1:4]) == want and np.array_equal(both[4], mat)
    # ... and with the close pairs of the same computation
    three = distance.mst_of_matrix(d, *loaded, want_matrix=True, pairs_within=20)
    assert len(three) == 6 and mc.edges_of_arrays(*three[1:4]) == want and np.array_equal(three[5], mat)
    assert all(np.array_equal(g, w) for g, w in zip(three[4], cc.filter_rows(mat, 20)))
    two = distance.mst_of_matrix(d, *loaded, pairs_within=0)
    assert len(two) == 5 and all(np.array_equal(g, w) for g, w in zip(two[4], cc.filter_rows(mat, 0)))
    for n in (0, 1):
        sym = np.frombuffer(b"ACGT" * n, dtype=np.uint8).reshape(n, 4)
        u, v, dist = d.mst(sym)
        assert len(u) == len(v) == len(dist) == 0
        assert d.mst(sym, want_matrix=True)[3].shape == (n, n)
