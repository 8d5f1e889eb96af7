"""The kernels of csrc/linkage.hip — the complete- and average-linkage trees of a device distance matrix — through
snpgpu_linkage_dev against the greedy definition of tests/linkage_cases.py: the merges, their order and the round count."""
import functools

import numpy as np
import pytest

from tests import linkage_cases as lc
from tests.gpu_util import get_device

pytestmark = pytest.mark.gpu

MARK = 0x5A5A5A5A
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def _tree(d, mat, kind, stride=None, garbage=False):
    """(merges, rounds) of the matrix at a row pitch of `stride`; with `garbage`, INT32_MIN / INT32_MAX fill the padding columns
    and the diagonal.  The matrix must come back untouched, and so must what lies behind the n - 1 merges."""
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
    room = max(n - 1, 0) + 8
    out = [torch.full((room,), MARK, dtype=torch.int32, device="cuda") for _ in range(4)] + [torch.full((room,), MARK, dtype=torch.int64, device="cuda")]
    torch.cuda.synchronize()
    k, rounds = d.linkage_dev(t.data_ptr(), n, stride, kind, *(o.data_ptr() for o in out))
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), host)                     # the input is not modified
    got = [o.cpu().numpy() for o in out]
    assert k == max(n - 1, 0)
    assert all((g[k:] == MARK).all() for g in got)
    return lc.merges_of_arrays(*(g[:k].view(np.uint32) for g in got[:4]), got[4][:k].view(np.uint64)), rounds


MATRICES = {
    "random": lambda n: lc.random_matrix(n, n, high=40),
    "zero": lc.zero_matrix,
    "equal": lambda n: np.full((n, n), 7, dtype=np.int32) - 7 * np.eye(n, dtype=np.int32),
    "line": lc.line_matrix,
    "xor": lc.xor_matrix,
    "tie": lambda n: lc.seeded_matrix(n, 17),
    "ties3": lambda n: lc.random_matrix(n, 5, high=3),
    "wide": lambda n: lc.random_matrix(n, 6, high=1000),
    "planted": lambda n: lc.planted_matrix(n, 600, 7),
    "largest": lambda n: np.full((n, n), INT_MAX, dtype=np.int32) - INT_MAX * np.eye(n, dtype=np.int32),
}


@functools.lru_cache(maxsize=None)
def _want(name, n, kind):
    """(matrix, the greedy tree), computed once."""
    mat = np.ascontiguousarray(MATRICES[name](n), dtype=np.int32)
    mat = np.minimum(mat, mat.T)
    mat.setflags(write=False)
    return mat, lc.greedy(mat, kind)


@pytest.mark.parametrize("kind", lc.KINDS)
@pytest.mark.parametrize("n", [0, 1, 2, 3, 63, 64, 65, 255, 256, 257])
def test_sizes_at_the_wave_and_workgroup_edges(n, kind):
    d = get_device()
    mat, want = _want("random", n, kind)
    got, rounds = _tree(d, mat, kind)
    assert got == want and len(got) == max(n - 1, 0)
    assert rounds <= max(n - 1, 0) and (rounds > 0) == (n > 1)
    assert rounds == (lc.rounds(mat, kind)[1] if n > 1 else 0)        # every reciprocal pair of a round merges


@pytest.mark.parametrize("kind", lc.KINDS)
@pytest.mark.parametrize("n,stride", [(3, 4), (65, 128), (130, 131), (257, 300)])
def test_a_row_pitch_beyond_n_and_garbage_in_padding_and_diagonal(n, stride, kind):
    d = get_device()
    mat, want = _want("ties3", n, kind)
    count = lc.rounds(mat, kind)[1]
    assert _tree(d, mat, kind, stride=stride, garbage=True) == (want, count)
    assert _tree(d, mat, kind, garbage=True) == (want, count)


@pytest.mark.parametrize("kind", lc.KINDS)
def test_identical_samples_take_one_round_per_merge(kind):
    d = get_device()
    mat, want = _want("zero", 65, kind)
    got, rounds = _tree(d, mat, kind)
    assert got == want == [(0, j, j, 1, 0) for j in range(1, 65)] and rounds == 64
    mat, want = _want("equal", 66, kind)
    got, rounds = _tree(d, mat, kind)
    assert got == want and [m[:2] for m in got] == [(0, j) for j in range(1, 66)] and rounds == 65


@pytest.mark.parametrize("kind", lc.KINDS)
def test_more_rows_than_the_grid_of_the_row_kernels(kind):
    """2 100 rows go round the grid-stride loops of k_lnk_init, k_lnk_rows and k_lnk_contract.  With every entry 7 the tree is known
    without building it: the ids break every tie, sample j joins the cluster of 0 at 7 (complete) or at a sum of 7 j (average)."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "snp_pipeline_amd", "csrc", "linkage.hip")).read()
    assert int(re.search(r"#define LNK_ROW_GRID_CAP (\d+)", src).group(1)) == 2048
    d = get_device()
    n = 2100
    mat = MATRICES["equal"](n)
    got, rounds = _tree(d, mat, kind)
    assert got == [(0, j, j, 1, 7 * j if kind == "average" else 7) for j in range(1, n)] and rounds == n - 1


@pytest.mark.parametrize("kind", lc.KINDS)
@pytest.mark.parametrize("name,n", [("line", 130), ("xor", 64), ("tie", 300), ("ties3", 257), ("wide", 257), ("planted", 90)])
def test_matrices_with_structure_and_ties(name, n, kind):
    d = get_device()
    mat, want = _want(name, n, kind)
    got, rounds = _tree(d, mat, kind)
    assert got == want
    keys = [lc.key(kind, m) for m in got]
    assert keys == sorted(keys)
    assert 1 <= rounds <= n - 1
    by_rounds, count = lc.rounds(mat, kind)
    assert by_rounds == want and rounds == count
    if name == "xor":
        assert rounds == 6                                           # the clusters pair up round by round


@pytest.mark.parametrize("kind", lc.KINDS)
def test_sums_of_the_largest_entries_do_not_wrap(kind):
    d = get_device()
    mat, want = _want("largest", 5, kind)
    got, rounds = _tree(d, mat, kind)
    assert got == want and rounds == 4
    assert got[-1] == ((0, 4, 4, 1, 4 * INT_MAX) if kind == "average" else (0, 4, 4, 1, INT_MAX))
    mat = lc.random_matrix(40, 9, high=50).astype(np.int64) + (INT_MAX - 50)
    np.fill_diagonal(mat, 0)
    mat = mat.astype(np.int32)
    assert _tree(d, mat, kind)[0] == lc.greedy(mat, kind)            # sums near 400 x 2^31, products beyond 2^64: compared in 128 bits


@pytest.mark.parametrize("kind", lc.KINDS)
def test_a_negative_entry_is_refused(kind):
    from snp_pipeline_amd import _lib as L
    from snp_pipeline_amd.device import SnpGpuError
    d = get_device()
    mat = lc.random_matrix(70, 3, high=9)
    mat[69, 68] = mat[68, 69] = -1
    with pytest.raises(SnpGpuError) as ei:
        _tree(d, mat, kind)
    assert ei.value.code == L.E_ARG and "negative" in str(ei.value)
    mat[69, 68] = mat[68, 69] = 0
    mat[5, 5] = -9                                                   # the diagonal is not an entry
    assert _tree(d, mat, kind)[0] == lc.greedy(np.where(np.eye(70, dtype=bool), 0, mat), kind)
    with pytest.raises(SnpGpuError):
        d.linkage_dev(0, 5, 5, kind)
    with pytest.raises(ValueError):
        d.linkage_dev(0, 0, 0, "single")
    assert d.linkage_dev(0, 0, 0, kind) == (0, 0) and d.linkage_dev(0, 1, 1, kind) == (0, 0)


@pytest.mark.parametrize("kind", lc.KINDS)
def test_host_forms_on_symbols_and_on_the_matrix_agree_with_the_statement(kind):
    d = get_device()
    sym = lc.planted_symbols(97, 1000, 6, seed=5)
    mat = lc.hamming_matrix(sym)
    want = lc.greedy(mat, kind)
    got = d.linkage(sym, kind, want_matrix=True, want_rounds=True)
    assert np.array_equal(got[5], mat)
    assert lc.merges_of_arrays(*got[:5]) == want
    assert lc.merges_of_arrays(*d.linkage(sym, kind)) == want
    of_matrix = d.linkage_of_matrix(got[5], kind, want_rounds=True)
    assert lc.merges_of_arrays(*of_matrix[:5]) == want and of_matrix[5] == got[6] == lc.rounds(mat, kind)[1]
    assert [x.dtype for x in got[:5]] == [np.uint32] * 4 + [np.uint64]
    for n in (0, 1):
        assert all(len(x) == 0 for x in d.linkage(sym[:n], kind)) and all(len(x) == 0 for x in d.linkage_of_matrix(mat[:n, :n], kind))
