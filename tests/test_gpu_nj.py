"""The kernels of csrc/nj.hip — the neighbour-joining tree of a device distance matrix, in fixed point — through snpgpu_nj_dev
against the statement of tests/nj_cases.py: the merges in round order, their branch lengths and the star."""
import functools
import os
import re

import numpy as np
import pytest

from tests import nj_cases as nc
from tests.gpu_util import get_device

pytestmark = pytest.mark.gpu

MARK = 0x5A5A5A5A
MARK64 = 0x5A5A5A5A5A5A5A5A
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def _tree(d, mat, stride=None, garbage=False):
    """The tree of the matrix at a row pitch of `stride`; with `garbage`, INT32_MIN / INT32_MAX fill the padding columns and the
    diagonal.  The matrix must come back untouched, and so must what lies behind the n - 3 merges — also when the call refuses."""
    import torch
    n = mat.shape[0]
    stride = n if stride is None else stride
    host = np.zeros((max(n, 1), max(stride, 1)), dtype=np.int32)
    if garbage:
        host[:] = np.where((np.arange(host.size).reshape(host.shape) % 3) == 0, INT_MIN, INT_MAX)
    host[:n, :n] = mat
    if garbage:
        host[np.arange(n), np.arange(n)] = np.where(np.arange(n) % 2 == 0, INT_MIN, INT_MAX)
    t = torch.from_numpy(host).cuda()
    room = max(n - 3, 0) + 8
    out = [torch.full((room,), MARK, dtype=torch.int32, device="cuda") for _ in range(2)] + [torch.full((room,), MARK64, dtype=torch.int64, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    try:
        k, star, star_len = d.nj_dev(t.data_ptr(), n, stride, *(o.data_ptr() for o in out))
    except Exception:
        torch.cuda.synchronize()
        assert all((o.cpu().numpy() == (MARK if o.dtype == torch.int32 else MARK64)).all() for o in out)      # refused before any record is written
        assert np.array_equal(t.cpu().numpy(), host)
        raise
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), host)                     # the input is not modified
    got = [o.cpu().numpy() for o in out]
    assert k == max(n - 3, 0)
    assert all((g[k:] == (MARK if g.dtype == np.int32 else MARK64)).all() for g in got)
    return nc.tree_of_arrays(got[0][:k].view(np.uint32), got[1][:k].view(np.uint32), got[2][:k], got[3][:k], star, star_len)


@functools.lru_cache(maxsize=None)
def _want(name, n):
    """(matrix, the tree of the statement), computed once."""
    mat = np.ascontiguousarray(nc.MATRICES[name](n), dtype=np.int32)
    mat.setflags(write=False)
    return mat, nc.nj_numpy(mat)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257])
def test_sizes_at_the_wave_and_workgroup_edges(n):
    d = get_device()
    mat, want = _want("random", n)
    got = _tree(d, mat)
    assert got == want and len(got[0]) == max(n - 3, 0)
    assert [s is not None for s in got[1]] == [n >= 2, n >= 2, n >= 3]


@pytest.mark.parametrize("n,stride", [(3, 4), (65, 128), (130, 131), (257, 300)])
def test_a_row_pitch_beyond_n_and_garbage_in_padding_and_diagonal(n, stride):
    d = get_device()
    mat, want = _want("ties3", n)
    assert _tree(d, mat, stride=stride, garbage=True) == want
    assert _tree(d, mat, garbage=True) == want


@pytest.mark.parametrize("name,n", [("line", 130), ("xor", 64), ("ties3", 257), ("wide", 257), ("planted", 90), ("zero", 65)])
def test_matrices_with_structure_and_ties(name, n):
    d = get_device()
    mat, want = _want(name, n)
    assert _tree(d, mat) == want
    if name == "zero":
        assert want == ([(0, j, 0, 0) for j in range(1, n - 2)], (0, n - 2, n - 1), (0, 0, 0))     # the ids break every tie


@pytest.mark.parametrize("name,n", [("random", 64), ("ties3", 257)])
def test_negative_branch_lengths_come_back_as_they_are(name, n):
    """Matrices that are no trees give negative lengths; the signed floor division and the arithmetic shifts are on that path."""
    d = get_device()
    mat, want = _want(name, n)
    assert nc.negative_lengths(want) >= 1 and len(nc.all_lengths(want)) == 2 * n - 3
    got = _tree(d, mat)
    assert got == want and nc.negative_lengths(got) == nc.negative_lengths(want)


@pytest.mark.parametrize("n", [65, 257])
def test_an_additive_tree_is_recovered_exactly(n):
    d = get_device()
    mat, want = _want("additive", n)
    got = _tree(d, mat)
    assert got == want
    assert np.array_equal(nc.path_sums(n, got), mat.astype(object) * nc.ONE) and nc.negative_lengths(got) == 0


def test_more_rows_than_the_grid_of_the_row_kernels_and_through_the_compactions():
    """2 100 rows go round the grid-stride loops of k_nj_init, k_nj_rows and k_nj_compact, k_nj_update takes nine workgroups, and the
    live columns move together every time an eighth of the stored slots have retired.  With every entry 2 the tree is known without
    building it: the ids break every tie.  What this does not show: the winning row is always 0 and the winning column among the first
    few, so the later sub-steps and turns of k_nj_rows' column loop and the later rows of k_nj_pick never decide a join, and every value
    a compaction moves is a 2 beside another 2.  tests/test_gpu_nj_edges.py sends matrices whose values differ everywhere."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "snp_pipeline_amd", "csrc", "nj.hip")).read()
    cap = int(re.search(r"#define NJ_ROW_GRID_CAP (\d+)", src).group(1))
    n = 2100
    num, den = (int(re.search(r"#define NJ_COMPACT_%s (\d+)" % w, src).group(1)) for w in ("NUM", "DEN"))
    assert n > cap and 0 < num < den and n * num * num // (den * den) > 3      # at least two compactions before the star
    d = get_device()
    assert _tree(d, nc.equal_matrix(n)) == nc.star_of_equal(n)


def test_refusals_come_before_any_record():
    from snp_pipeline_amd import _lib as L
    from snp_pipeline_amd.device import SnpGpuError
    d = get_device()
    mat = nc.random_matrix(70, 3, high=9)
    mat[69, 68] = mat[68, 69] = -1
    with pytest.raises(SnpGpuError) as ei:
        _tree(d, mat)
    assert ei.value.code == L.E_ARG and "negative" in str(ei.value)
    mat[69, 68] = mat[68, 69] = 0
    mat[5, 5] = -9                                                   # the diagonal is not an entry
    assert _tree(d, mat) == nc.nj_numpy(np.where(np.eye(70, dtype=bool), 0, mat))
    with pytest.raises(SnpGpuError) as ei:                           # (2^31 - 1) << 20 exceeds 2^61 / 2100
        _tree(d, nc.equal_matrix(2100, INT_MAX))
    assert ei.value.code == L.E_ARG and "2^61" in str(ei.value)
    mat, want = _want("largest", 4)                                  # ... and fits 2^61 / 4
    assert _tree(d, mat) == want == ([(0, 1, INT_MAX << 19, INT_MAX * nc.ONE - (INT_MAX << 19))], (0, 2, 3), (0, INT_MAX << 19, INT_MAX * nc.ONE - (INT_MAX << 19)))
    with pytest.raises(SnpGpuError):
        d.nj_dev(0, 5, 5)
    assert d.nj_dev(0, 0, 0) == d.nj_dev(0, 1, 1) == (0, (None, None, None), (0, 0, 0))


def test_host_forms_on_symbols_and_on_the_matrix_agree_with_the_statement():
    d = get_device()
    sym = nc.planted_symbols(97, 1000, 6, seed=5)
    rng = np.random.default_rng(11)
    sym = sym.copy()
    lower = rng.random(sym.shape) < 0.3
    sym[lower] |= 0x20                                               # lower case counts as its upper case
    sym[rng.random(sym.shape) < 0.05] = ord("N")                     # N and - are never compared
    sym[rng.random(sym.shape) < 0.05] = ord("-")
    sym[:, 900:][rng.random((97, 100)) < 0.5] = ord("-")             # a tenth of the columns half missing
    upper = sym & 0xDF
    acgt = np.isin(upper, np.frombuffer(b"ACGT", dtype=np.uint8))
    mat = ((upper[:, None, :] != upper[None, :, :]) & acgt[:, None, :] & acgt[None, :, :]).sum(axis=2).astype(np.int32)
    want = nc.nj_numpy(mat)
    got = d.nj(sym, want_matrix=True)
    assert np.array_equal(got[6], mat)
    assert nc.tree_of_arrays(*got[:6]) == want
    assert nc.tree_of_arrays(*d.nj(sym)) == want
    assert nc.tree_of_arrays(*d.nj_of_matrix(mat)) == want
    assert [x.dtype for x in got[:4]] == [np.uint32] * 2 + [np.int64] * 2
    for n in (0, 1, 2, 3):
        assert nc.tree_of_arrays(*d.nj(sym[:n])) == nc.tree_of_arrays(*d.nj_of_matrix(mat[:n, :n])) == nc.nj_numpy(mat[:n, :n])
