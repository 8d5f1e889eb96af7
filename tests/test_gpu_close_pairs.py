"""Kernel (a) of csrc/clusters.hip — the rows of a device distance matrix as a CSR of their entries <= T — through
snpgpu_close_pairs_dev against the NumPy filter of tests/clusters_cases.py: the arrays must be equal, element order included."""
import os
import re

import numpy as np
import pytest

from tests import clusters_cases as cc
from tests.gpu_util import get_device

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARK = 0x5A5A5A5A
BIG = 1000                                                             # the largest value of the test matrices


def _matrix(n, seed):
    """Any int32 matrix will do (the kernel knows nothing of symmetry): values 1 .. BIG off the diagonal, one row with only its
    diagonal within reach of small thresholds, one row with everything."""
    rng = np.random.default_rng(seed)
    m = rng.integers(1, BIG + 1, size=(n, n)).astype(np.int32)
    if n:
        m[rng.integers(0, n), rng.integers(0, n)] = BIG                 # the maximum is there
        np.fill_diagonal(m, 0)
    if n > 2:
        m[1, :] = BIG
        m[1, 1] = 0
        m[2, :] = 0
    return m


def _on_device(mat, stride, shift=0):
    """The matrix with a row pitch of `stride` (zeros in the padding), `shift` int32 elements into an allocation: (tensor, pointer)."""
    import torch
    n = mat.shape[0]
    host = np.zeros(shift + n * stride + 4, dtype=np.int32)
    if n:
        host[shift:shift + n * stride].reshape(n, stride)[:, :n] = mat
    t = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + 4 * shift


def _csr(d, ptr, n, stride, lo, hi, threshold, capacity=None):
    """(count, row_off, col, dist, slack) with the outputs pre-filled with MARK and `slack` words of room behind them."""
    import torch
    total = d.close_pairs_dev(ptr, n, stride, lo, hi, threshold)
    cap = total if capacity is None else capacity
    off = torch.full((hi - lo + 1 + 2,), -1, dtype=torch.int64, device="cuda")
    col = torch.full((max(total, cap) + 8,), MARK, dtype=torch.int32, device="cuda")
    dist = torch.full((max(total, cap) + 8,), MARK, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    got = d.close_pairs_dev(ptr, n, stride, lo, hi, threshold, cap, off.data_ptr(), col.data_ptr(), dist.data_ptr())
    torch.cuda.synchronize()
    assert got == total
    return total, off.cpu().numpy(), col.cpu().numpy(), dist.cpu().numpy()


def _check(d, mat, stride, lo, hi, threshold, shift=0):
    n = mat.shape[0]
    keep, ptr = _on_device(mat, stride, shift)
    total, off, col, dist = _csr(d, ptr, n, stride, lo, hi, threshold)
    w_off, w_col, w_dist = cc.filter_rows(mat, threshold, lo, hi, n)
    where = (n, stride, lo, hi, threshold, shift)
    assert total == len(w_col), where
    if total == 0:                                                      # capacity 0: the call only counts
        assert (off == -1).all() and (col == MARK).all(), where
        return
    assert np.array_equal(off[:hi - lo + 1].astype(np.uint64), w_off) and (off[hi - lo + 1:] == -1).all(), where
    assert np.array_equal(col[:total].view(np.uint32), w_col), where
    assert np.array_equal(dist[:total], w_dist), where
    assert (col[total:] == MARK).all() and (dist[total:] == MARK).all(), where
    del keep


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 127, 128, 129, 257])
def test_sizes_pitches_and_thresholds(n):
    d = get_device()
    mat = _matrix(n, n)
    top = int(mat.max()) if n else 0
    for stride in sorted({n, (n + 127) // 128 * 128}):
        for t in (0, top - 1, top, top + 1, cc.INT_MAX):
            _check(d, mat, stride, 0, n, t)


@pytest.mark.parametrize("n", [129, 257])
def test_matches_at_chosen_columns(n):
    d = get_device()
    mat = np.full((n, n), BIG, dtype=np.int32)
    spots = (0, 63, 64, n - 1)
    for r, c in enumerate(spots):                                       # one match per row, then pairs, then all four
        mat[r, c] = 3
    mat[4, [0, 63]] = 3
    mat[5, [63, 64]] = 3
    mat[6, [64, n - 1]] = 3
    mat[7, list(spots)] = 3
    for stride in (n, (n + 127) // 128 * 128):
        for shift in (0, 1):
            _check(d, mat, stride, 0, n, 3, shift)
    _, ptr = keep = _on_device(mat, n)
    total, off, col, _ = _csr(d, ptr, n, n, 0, 8, 3)
    assert total == 14 and col[:total].tolist() == [0, 63, 64, n - 1, 0, 63, 63, 64, 64, n - 1, 0, 63, 64, n - 1]
    del keep


def test_bands():
    d = get_device()
    n = 129
    mat = _matrix(n, 3)
    for stride in (n, 256):
        for lo, hi in ((0, 0), (0, n), (40, 97), (77, 78), (n - 1, n), (n, n)):
            for t in (0, 400):
                _check(d, mat, stride, lo, hi, t)


def test_a_base_that_is_not_16_byte_aligned():
    d = get_device()
    for n in (3, 65, 129):
        mat = _matrix(n, 40 + n)
        for stride in (n, (n + 127) // 128 * 128, n + 1, n + 2):
            for shift in (1, 2, 3):
                _check(d, mat, stride, 0, n, 500, shift)


def test_capacity_protocol():
    import torch
    d = get_device()
    n = 65
    mat = _matrix(n, 9)
    keep, ptr = _on_device(mat, n)
    want = cc.filter_rows(mat, 300)
    total = len(want[1])
    assert total > n
    for cap, written in ((0, False), (total - 1, False), (total, True), (total + 5, True)):
        got, off, col, dist = _csr(d, ptr, n, n, 0, n, 300, capacity=cap)
        assert got == total                                             # *out_n is always set
        if not written:
            assert (off == -1).all() and (col == MARK).all() and (dist == MARK).all(), cap
        else:
            assert np.array_equal(off[:n + 1].astype(np.uint64), want[0]) and np.array_equal(col[:total].view(np.uint32), want[1]), cap
            assert np.array_equal(dist[:total], want[2]) and (col[total:] == MARK).all() and (dist[total:] == MARK).all(), cap
    # bad arguments are refused before anything runs
    from snp_pipeline_amd.device import SnpGpuError
    for args in ((n, n - 1, 0, n), (n, n, 5, 4), (n, n, 0, n + 1)):
        with pytest.raises(SnpGpuError):
            d.close_pairs_dev(ptr, args[0], args[1], args[2], args[3], 1)
    with pytest.raises(SnpGpuError):
        d.close_pairs_dev(ptr + 2, n, n, 0, n, 1)
    torch.cuda.synchronize()
    del keep


def test_more_rows_than_the_grid_holds():
    src = open(os.path.join(ROOT, "snp_pipeline_amd", "csrc", "clusters.hip")).read()
    cap = int(re.search(r"#define CLUSTERS_ROW_GRID_CAP (\d+)", src).group(1))
    d = get_device()
    n = cap + 1
    rng = np.random.default_rng(1)
    mat = np.full((n, n), BIG, dtype=np.int32)
    np.fill_diagonal(mat, 0)
    r, c = rng.integers(0, n, size=3 * n), rng.integers(0, n, size=3 * n)
    mat[r, c] = rng.integers(0, 20, size=3 * n)
    mat[n - 1, [0, n - 1]] = 1                                          # the row past the cap has something to say
    _check(d, mat, n, 0, n, 10)
    _check(d, mat, (n + 127) // 128 * 128, 0, n, 10)


def test_two_runs_give_the_same_bytes():
    d = get_device()
    n = 257
    mat = _matrix(n, 77)
    keep, ptr = _on_device(mat, n)
    a = _csr(d, ptr, n, n, 0, n, 500)
    b = _csr(d, ptr, n, n, 0, n, 500)
    assert a[0] == b[0] > n
    for x, y in zip(a[1:], b[1:]):
        assert x.tobytes() == y.tobytes()
    del keep


def test_host_form_equals_the_filter_of_the_distance_matrix():
    d = get_device()
    rng = np.random.default_rng(4)
    for n, s in ((1, 10), (130, 300), (67, 0)):
        base = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=s)
        sym = np.tile(base, (n, 1))
        flips = rng.random((n, s)) < rng.random((n, 1)) * 0.2           # rows at every distance from the base sequence
        sym[flips] = rng.choice(np.frombuffer(b"ACGTacgt-N", dtype=np.uint8), size=int(flips.sum()))
        mat = d.distance(sym) if s else np.zeros((n, n), dtype=np.int32)
        for t in (0, int(np.median(mat)), int(mat.max()), cc.INT_MAX):
            want = cc.filter_rows(mat, t)
            for capacity in (None, 1):                                  # 1: the first call only learns the count, the second fetches
                got = d.close_pairs(sym, t, capacity=capacity)
                assert all(np.array_equal(g, w) for g, w in zip(got, want)), (n, s, t, capacity)
                # ... and with the matrix of the same computation, for a caller that writes the two tables as well
                both = d.close_pairs(sym, t, capacity=capacity, want_matrix=True)
                assert len(both) == 4 and all(np.array_equal(g, w) for g, w in zip(both, want)) and np.array_equal(both[3], mat), (n, s, t, capacity)
    got = d.close_pairs(np.zeros((0, 5), dtype=np.uint8), 3)
    assert got[0].tolist() == [0] and len(got[1]) == 0 and len(got[2]) == 0
