"""The kernel of csrc/pair_sites.hip — the columns at which pairs of rows of the packed matrix differ — through
snpgpu_pair_sites_dev against the NumPy statement of tests/pair_sites_cases.py: the three arrays are compared whole."""
import functools
import os
import re

import numpy as np
import pytest

from tests import pair_sites_cases as pc
from tests.gpu_util import get_device

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARK32, MARK8 = 0x5A5A5A5A, 0x5A


def _packed(d, sym):
    """The byte matrix packed on the device: (tensor that owns the memory, pointer)."""
    import torch
    n, s = sym.shape
    t = torch.zeros(max(n * d.packed_row_bytes(s), 16), dtype=torch.uint8, device="cuda")
    if n and s:
        src = torch.from_numpy(np.array(sym, dtype=np.uint8, order="C")).cuda()
        d.pack_matrix_dev(src.data_ptr(), n, s, s, t.data_ptr())
        torch.cuda.synchronize()
        del src
    return t, t.data_ptr()


def _lists(a, b):
    import torch
    a = np.ascontiguousarray(a, dtype=np.uint32)
    b = np.ascontiguousarray(b, dtype=np.uint32)
    pad = np.zeros(4, dtype=np.uint32)                                   # (an empty list still has an address)
    return torch.from_numpy(np.concatenate((a, pad)).view(np.int32)).cuda(), torch.from_numpy(np.concatenate((b, pad)).view(np.int32)).cuda()


def _sites(d, ptr, n, s, a, b, capacity=None, n_rows=None):
    """(count, pair_off, site, bases) with the outputs pre-filled with marks and room behind them; capacity None: what the count
    call says (at least 1, so that the offsets are written)."""
    import torch
    m = len(a)
    n_rows = n if n_rows is None else n_rows
    d_a, d_b = _lists(a, b)
    total = d.pair_sites_dev(ptr, n_rows, s, d_a.data_ptr(), d_b.data_ptr(), m)
    cap = max(total, 1) if capacity is None else capacity
    off = torch.full((m + 1 + 2,), -1, dtype=torch.int64, device="cuda")
    site = torch.full((max(total, cap) + 8,), MARK32, dtype=torch.int32, device="cuda")
    bases = torch.full((max(total, cap) + 8,), MARK8, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    got = d.pair_sites_dev(ptr, n_rows, s, d_a.data_ptr(), d_b.data_ptr(), m, cap, off.data_ptr(), site.data_ptr(), bases.data_ptr())
    torch.cuda.synchronize()
    assert got == total
    return total, off.cpu().numpy(), site.cpu().numpy(), bases.cpu().numpy()


def _check(d, sym, a, b, want=None, where=None):
    n, s = sym.shape
    keep, ptr = _packed(d, sym)
    total, off, site, bases = _sites(d, ptr, n, s, a, b)
    w_off, w_site, w_bases = pc.pair_sites(sym, a, b) if want is None else want
    m = len(a)
    assert total == len(w_site), where
    assert np.array_equal(off[:m + 1].astype(np.uint64), w_off) and (off[m + 1:] == -1).all(), where
    assert np.array_equal(site[:total].view(np.uint32), w_site), where
    assert np.array_equal(bases[:total], w_bases), where
    assert (site[total:] == MARK32).all() and (bases[total:] == MARK8).all(), where
    del keep
    return total


def _all_pairs(n):
    a, b = np.triu_indices(n, 1)
    return np.concatenate((a, b)).astype(np.uint32), np.concatenate((b, a)).astype(np.uint32)      # ... and reversed: the nibbles swap


@pytest.mark.parametrize("s", [1, 31, 32, 33, 127, 128, 129, 2047, 2048, 2049, 4097])
def test_sizes(s):
    """Bit, word, padding-word and 64-lane-step edges: 5 rows, all 10 pairs and the 10 reversed ones."""
    d = get_device()
    rng = np.random.default_rng(s)
    sym = np.frombuffer(b"ACGTACGTacgtN-nX", dtype=np.uint8)[rng.integers(0, 16, size=(5, s))]
    sym[:, -1] = np.frombuffer(b"ACGTa", dtype=np.uint8)                 # the last column always counts
    a, b = _all_pairs(5)
    total = _check(d, sym, a, b, where=s)
    assert total >= 16
    fwd, rev = pc.pair_sites(sym, a[:10], b[:10]), pc.pair_sites(sym, b[:10], a[:10])
    assert np.array_equal(fwd[1], rev[1]) and np.array_equal(fwd[2] >> 4 | (fwd[2] & 15) << 4, rev[2])


def test_differences_at_chosen_columns():
    d = get_device()
    s = 4097
    sym = np.full((4, s), ord("A"), dtype=np.uint8)
    spots = [0, 31, 32, 63, 2047, 2048, s - 1]
    sym[1, spots] = ord("c")
    sym[2] = sym[0]                                                      # a pair that differs nowhere
    sym[3, :] = np.frombuffer(b"-N", dtype=np.uint8)[np.arange(s) % 2]  # nothing counts against it
    a, b = np.asarray([0, 1, 0, 3, 1, 2, 3], np.uint32), np.asarray([1, 0, 2, 1, 2, 0, 3], np.uint32)
    keep, ptr = _packed(d, sym)
    total, off, site, bases = _sites(d, ptr, 4, s, a, b)
    assert total == 21 and off[:8].tolist() == [0, 7, 14, 14, 14, 21, 21, 21]
    assert site[:21].tolist() == spots * 3
    assert bases[:7].tolist() == [0x50] * 7 and bases[7:14].tolist() == [0x05] * 7 and bases[14:21].tolist() == [0x05] * 7     # A/c, c/A, c/A
    del keep
    _check(d, sym, a, b)
    # a pair that differs everywhere, with a count above 65 535
    s = 70000
    far = np.stack((np.frombuffer(b"ACGT", dtype=np.uint8)[np.arange(s) % 4], np.frombuffer(b"cgta", dtype=np.uint8)[np.arange(s) % 4]))
    want = (np.asarray([0, s, 2 * s], np.uint64), np.tile(np.arange(s, dtype=np.uint32), 2),
            np.concatenate((pc.nibble(far[0]) | pc.nibble(far[1]) << 4, pc.nibble(far[1]) | pc.nibble(far[0]) << 4)).astype(np.uint8))
    assert _check(d, far, [0, 1], [1, 0], want=want) == 2 * s
    assert all(np.array_equal(x, y) for x, y in zip(want, pc.pair_sites(far, [0, 1], [1, 0])))


def test_every_byte_value_opposite_every_letter():
    """All 256 byte values opposite each of ACGTacgt: only valid, unequal-after-upper-casing columns appear, and the letters come
    back with their case."""
    d = get_device()
    sym = np.zeros((2, 2048), dtype=np.uint8)
    sym[0] = np.repeat(np.arange(256, dtype=np.uint8), 8)
    sym[1] = np.tile(np.frombuffer(b"ACGTacgt", dtype=np.uint8), 256)
    keep, ptr = _packed(d, sym)
    total, off, site, bases = _sites(d, ptr, 2, 2048, [0, 1], [1, 0])
    del keep
    letters = np.frombuffer(pc.LETTERS.encode(), dtype=np.uint8)
    want_cols = [c for c in range(2048) if chr(sym[0, c]) in "ACGTacgt" and chr(sym[0, c]).upper() != chr(sym[1, c]).upper()]
    assert len(want_cols) == 8 * 6 and total == 2 * len(want_cols)
    assert site[:total].tolist() == want_cols * 2
    half = total // 2
    assert np.array_equal(letters[bases[:half] & 7], sym[0, want_cols]) and np.array_equal(letters[bases[:half] >> 4], sym[1, want_cols])
    assert np.array_equal(letters[bases[half:total] & 7], sym[1, want_cols]) and np.array_equal(letters[bases[half:total] >> 4], sym[0, want_cols])
    _check(d, sym, [0, 1], [1, 0])


def test_pair_lists():
    src = open(os.path.join(ROOT, "snp_pipeline_amd", "csrc", "pair_sites.hip")).read()
    cap = int(re.search(r"#define PAIR_SITES_GRID_CAP (\d+)", src).group(1))
    threads = int(re.search(r"#define PAIR_SITES_THREADS (\d+)", src).group(1))
    d = get_device()
    sym = pc.planted(7, 33, 3, 11)
    sym[6] = np.frombuffer(b"ACGT", dtype=np.uint8)[(np.arange(33) + 1) % 4]
    none = np.zeros(0, dtype=np.uint32)
    assert _check(d, sym, none, none) == 0                               # m = 0
    assert _check(d, sym, [6], [0]) > 0                                  # m = 1
    assert _check(d, sym, [3, 0, 6], [3, 0, 6]) == 0                     # a == b
    assert _check(d, sym, [6, 2, 6, 6, 2], [0, 5, 0, 0, 5]) > 0          # duplicates
    m = 5000                                                             # more pairs than the grid holds: some waves take a second one
    assert m > cap * (threads // 64)
    rng = np.random.default_rng(2)
    a, b = rng.integers(0, 7, size=m).astype(np.uint32), rng.integers(0, 7, size=m).astype(np.uint32)
    a[-1], b[-1] = 6, 0                                                  # the last pair has something to say
    assert _check(d, sym, a, b) > m


def test_a_row_outside_the_matrix_is_refused_and_nothing_is_written():
    import torch
    from snp_pipeline_amd.device import SnpGpuError
    d = get_device()
    sym = pc.planted(5, 129, 2, 4)
    keep, ptr = _packed(d, sym)
    for a, b in (([0, 5, 1], [1, 2, 3]), ([0, 1], [1, 5]), ([0xFFFFFFFF], [0])):
        d_a, d_b = _lists(a, b)
        off = torch.full((len(a) + 3,), -1, dtype=torch.int64, device="cuda")
        site = torch.full((600,), MARK32, dtype=torch.int32, device="cuda")
        bases = torch.full((600,), MARK8, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for cap in (0, 600):
            with pytest.raises(SnpGpuError) as ei:
                d.pair_sites_dev(ptr, 5, 129, d_a.data_ptr(), d_b.data_ptr(), len(a), cap, off.data_ptr(), site.data_ptr(), bases.data_ptr())
            assert ei.value.code == -2
        torch.cuda.synchronize()
        assert (off.cpu().numpy() == -1).all() and (site.cpu().numpy() == MARK32).all() and (bases.cpu().numpy() == MARK8).all()
    # the same lists are fine for a matrix that has the row: the bound is n_rows, not the allocation
    with pytest.raises(SnpGpuError):
        d.pair_sites(sym, [0, 5], [1, 2])
    with pytest.raises(SnpGpuError):
        d.pair_sites_dev(ptr + 4, 5, 129, 0, 0, 0)                       # a packed matrix off the 16-byte grid
    del keep


def test_capacity_protocol():
    d = get_device()
    sym = pc.planted(6, 2049, 2, 8, spread=40)
    a, b = _all_pairs(6)
    want = pc.pair_sites(sym, a, b)
    total = len(want[1])
    assert total > 100
    keep, ptr = _packed(d, sym)
    for cap, written in ((0, False), (total - 1, False), (total, True), (total + 5, True)):
        got, off, site, bases = _sites(d, ptr, 6, 2049, a, b, capacity=cap)
        assert got == total                                             # *out_n is always set
        if not written:
            assert (off == -1).all() and (site == MARK32).all() and (bases == MARK8).all(), cap
        else:
            assert np.array_equal(off[:len(a) + 1].astype(np.uint64), want[0]) and np.array_equal(site[:total].view(np.uint32), want[1]), cap
            assert np.array_equal(bases[:total], want[2]) and (site[total:] == MARK32).all() and (bases[total:] == MARK8).all(), cap
    del keep


def test_two_runs_give_the_same_bytes():
    d = get_device()
    sym = pc.planted(9, 4097, 3, 21, spread=200)
    a, b = _all_pairs(9)
    keep, ptr = _packed(d, sym)
    one = _sites(d, ptr, 9, 4097, a, b)
    two = _sites(d, ptr, 9, 4097, a, b)
    assert one[0] == two[0] > 1000
    for x, y in zip(one[1:], two[1:]):
        assert x.tobytes() == y.tobytes()
    del keep


@functools.lru_cache(maxsize=None)
def _identity_case():
    sym = pc.planted(257, 1000, 9, 77, spread=6)
    sym.setflags(write=False)
    return sym


def test_rows_per_pair_are_the_entries_of_the_distance_matrix():
    """The feature's own check: on 257 x 1 000 with planted groups every pair — all 257 x 257 ordered ones — has as many entries as
    Device.distance says; the host form gives the arrays of the device form."""
    d = get_device()
    sym = _identity_case()
    n, s = sym.shape
    mat = d.distance(sym)
    assert (mat[np.triu_indices(n, 1)] <= 12).sum() > 100 and mat.max() > 500           # close pairs and far ones
    a, b = (x.ravel().astype(np.uint32) for x in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    keep, ptr = _packed(d, sym)
    total, off, site, bases = _sites(d, ptr, n, s, a, b)
    del keep
    assert np.array_equal(np.diff(off[:n * n + 1]).reshape(n, n), mat) and total == int(mat.sum())
    # the host form equals the device form, with and without the room known in advance; a sample of the pairs against the statement
    pick = np.random.default_rng(1).choice(n * n, size=300, replace=False)
    pa, pb = a[pick], b[pick]
    want = pc.pair_sites(sym, pa, pb)
    for expect in (None, int(mat[pa, pb].sum()), 1):
        got = d.pair_sites(sym, pa, pb, expect=expect)
        assert all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(got, want)), expect
    lo = int(off[pick[0]])
    assert np.array_equal(site[lo:lo + int(mat[pa[0], pb[0]])].view(np.uint32), want[1][:int(want[0][1])])
    got = d.pair_sites(sym, [], [])
    assert got[0].tolist() == [0] and len(got[1]) == 0 and len(got[2]) == 0


def test_one_computation_for_tree_pairs_and_sites():
    """distance_outputs: the tree, the pairs within T and the matrix of one call equal those of the single calls, and the packed
    matrix it leaves in the context answers pair lists until it is dropped."""
    from snp_pipeline_amd.device import SnpGpuError
    d = get_device()
    sym = _identity_case()
    n = len(sym)
    mat = d.distance(sym)
    tree, csr, got_mat = d.distance_outputs(sym, want_tree=True, want_matrix=True, pairs_within=12, keep_packed=True)
    assert np.array_equal(got_mat, mat)
    assert all(np.array_equal(x, y) for x, y in zip(tree, d.mst(sym)))
    assert all(np.array_equal(x, y) for x, y in zip(csr, d.close_pairs(sym, 12)))
    u, v, dist = tree
    off, site, bases = d.pair_sites_kept(u, v, expect=int(dist.sum()))
    assert np.array_equal(np.diff(off).astype(np.int64), dist.astype(np.int64))
    assert all(np.array_equal(x, y) for x, y in zip((off, site, bases), pc.pair_sites(sym, u, v)))
    a, b, dd = pc.pairs_of_csr(*csr, 12)
    assert all(np.array_equal(x, y) for x, y in zip(d.pair_sites_kept(a, b), pc.pair_sites(sym, a, b))) and len(a) > 100
    with pytest.raises(SnpGpuError):
        d.pair_sites_kept([n], [0])
    d.packed_drop()
    with pytest.raises(SnpGpuError):
        d.pair_sites_kept([0], [1])
    d.packed_drop()                                                       # nothing kept: nothing to do
    only_pairs = d.distance_outputs(sym, pairs_within=12)
    assert only_pairs[0] is None and only_pairs[2] is None and all(np.array_equal(x, y) for x, y in zip(only_pairs[1], csr))
    with pytest.raises(SnpGpuError):
        d.pair_sites_kept([0], [1])                                       # ... and that call kept nothing


def test_pair_sites_of_matrix_works_in_sorted_id_order():
    """The arrays of snp_matrix.load_matrix with the records in falling id order and shorter earlier rows: pairs are indices into the
    sorted ids, and the padding of a shorter row never differs."""
    from snp_pipeline_amd import distance
    d = get_device()
    sym = np.array(_identity_case()[:6, :130])
    lens = np.asarray([130, 130, 130, 129, 64, 1], dtype=np.int64)        # file order: s5 ... s0, so the sorted lengths rise
    for r, k in enumerate(lens):
        sym[r, k:] = ord("-")
    file_ids = ["s%d" % (5 - r) for r in range(6)]
    a, b = _all_pairs(6)
    ids, off, site, bases = distance.pair_sites_of_matrix(d, file_ids, sym, lens, a, b)
    assert ids == sorted(file_ids)
    want = pc.pair_sites(sym[::-1], a, b)
    assert all(np.array_equal(g, w) for g, w in zip((off, site, bases), want)) and len(site) > 100
    mat = d.distance(np.ascontiguousarray(sym[::-1]))
    assert np.array_equal(np.diff(off).astype(np.int64), mat[a, b].astype(np.int64))
    assert int(np.diff(off)[0]) <= 1                                      # s0 has one site: everything behind it is padding
