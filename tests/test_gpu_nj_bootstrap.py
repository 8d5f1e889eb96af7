"""The kernels of csrc/nj_bootstrap.hip — the bootstrap's columns, the resampled pack, the bipartitions of join records and the support
counts — and the host form Device.nj_bootstrap, against the statement of tests/nj_bootstrap_cases.py."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import nj_bootstrap_cases as bc
from tests import nj_cases as nc
from tests.gpu_util import get_device

pytestmark = pytest.mark.gpu

MARK = 0x5A5A5A5A
MARK64 = 0x5A5A5A5A5A5A5A5A
SIZES = [4, 5, 63, 64, 65, 128, 129, 257]


def _dev(array):
    """A host array as a device tensor of the same bytes (unsigned types travel as their signed twins)."""
    import torch
    array = np.ascontiguousarray(array)
    twin = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(array.dtype)
    out = torch.from_numpy(array.view(twin) if twin else array).cuda()
    torch.cuda.synchronize()                                         # (the library works on a stream of its own)
    return out


def _filled(count, value, dtype):
    import torch
    out = torch.full((count,), value, dtype=dtype, device="cuda")
    torch.cuda.synchronize()
    return out


def _host(tensor, dtype):
    return tensor.cpu().numpy().view(dtype)


# ---- the columns -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [0, 1, 63, 64, 65, 1000, 70001])
def test_the_columns_of_a_replicate_are_the_draws_of_the_statement(s):
    import torch
    d = get_device()
    for seed in (0, 1, 2 ** 64 - 1):
        for b in (0, 7):
            out = _filled(s + 8, MARK, torch.int32)
            d.bootstrap_columns_dev(seed, b, s, out.data_ptr())
            torch.cuda.synchronize()
            got = _host(out, np.uint32)
            assert np.array_equal(got[:s], bc.columns(seed, b, s)), (seed, b)
            assert (got[s:] == MARK).all()                          # the words behind the array are untouched
            assert s == 0 or int(got[:s].max()) < s
            out = _filled(s + 8, MARK, torch.int32)                  # ... and ascending, as the host form hands them to the resample
            d.bootstrap_columns_dev(seed, b, s, out.data_ptr(), ascending=True)
            torch.cuda.synchronize()
            got = _host(out, np.uint32)
            assert np.array_equal(got[:s], np.sort(bc.columns(seed, b, s))) and (got[s:] == MARK).all(), (seed, b)


# ---- the resampled pack ----------------------------------------------------------------------------------------------------------
def _pack(sym):
    """The packed matrix of the statement: uint4 {valid, hi, lo, lower} per 32 sites, rows padded with zero words to a multiple of 4."""
    sym = np.asarray(sym, dtype=np.uint8)
    n, s = sym.shape
    words = ((s + 31) // 32 + 3) // 4 * 4
    lower = (sym >= 97) & (sym <= 122)
    upper = np.where(lower, sym - 32, sym)
    valid = np.isin(upper, np.frombuffer(b"ACGT", dtype=np.uint8))
    hi = valid & ((upper == ord("G")) | (upper == ord("T")))
    lo = valid & ((upper == ord("C")) | (upper == ord("T")))
    out = np.zeros((n, words, 4), dtype=np.uint32)
    for p, plane in enumerate((valid, hi, lo, lower)):
        bits = np.zeros((n, words * 32), dtype=np.uint8)
        bits[:, :s] = plane
        out[:, :, p] = np.packbits(bits.reshape(n, words, 32), axis=2, bitorder="little").view("<u4")[:, :, 0]
    return out


def _symbols(n, s, seed):
    rng = np.random.default_rng(seed)
    sym = np.frombuffer(b"ACGTacgtNn-", dtype=np.uint8)[rng.integers(0, 11, size=(n, s))]
    return np.ascontiguousarray(sym)


@pytest.mark.parametrize("n", [1, 5, 130])
def test_the_resampled_pack_is_the_pack_of_the_gathered_symbols(n):
    import torch
    d = get_device()
    for s in (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1000):
        sym = _symbols(n, s, 1000 * n + s)
        packed = _pack(sym)
        assert d.packed_row_bytes(s) == packed.shape[1] * 16
        src = _dev(packed)
        by_device, d_sym = _filled(packed.size, 0, torch.int32), _dev(sym)       # the library's own packer gives the same source
        d.pack_matrix_dev(d_sym.data_ptr(), n, s, s, by_device.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(_host(by_device, np.uint32).reshape(packed.shape), packed)
        drawn = bc.columns(1, 0, s)
        lists = {"identity": np.arange(s), "reversed": np.arange(s)[::-1], "zeros": np.zeros(s), "last": np.full(s, s - 1), "drawn": drawn, "sorted": np.sort(drawn),
                 "longer": np.sort(bc.columns(3, 1, 2 * s + 3) % s)}
        for name, cols in lists.items():
            cols = np.ascontiguousarray(cols, dtype=np.uint32)
            want = _pack(sym[:, cols])
            out, d_cols = _filled(want.size + 16, -1, torch.int32), _dev(cols)            # every bit set: zero padding has to be written
            d.resample_packed_dev(src.data_ptr(), n, s, d_cols.data_ptr(), len(cols), out.data_ptr())
            torch.cuda.synchronize()
            got = _host(out, np.uint32)
            assert np.array_equal(got[:want.size].reshape(want.shape), want), (s, name)
            assert (got[want.size:] == 0xFFFFFFFF).all(), (s, name)
            assert not want[:, (len(cols) + 31) // 32:].any()         # (the padding words of the statement are zero)
        assert np.array_equal(_host(src, np.uint32).reshape(packed.shape), packed)      # the source pack is untouched


def test_a_column_beyond_the_matrix_is_refused_before_anything_is_written():
    import torch
    from snp_pipeline_amd import _lib as L
    from snp_pipeline_amd.device import SnpGpuError
    d = get_device()
    n, s = 5, 100
    src = _dev(_pack(_symbols(n, s, 3)))
    for cols in ([0, 99, 100], [2 ** 32 - 1] + [1] * 300, [100]):
        cols = np.asarray(cols, dtype=np.uint32)
        out, d_cols = _filled(n * 16 * 4, MARK, torch.int32), _dev(cols)
        with pytest.raises(SnpGpuError) as ei:
            d.resample_packed_dev(src.data_ptr(), n, s, d_cols.data_ptr(), len(cols), out.data_ptr())
        torch.cuda.synchronize()
        assert ei.value.code == L.E_ARG and (_host(out, np.uint32) == MARK).all()
    with pytest.raises(SnpGpuError):
        d.resample_packed_dev(src.data_ptr(), n, s, 0, 3, src.data_ptr())
    d.resample_packed_dev(0, 0, s, 0, 3, 0)                          # no row, no column: nothing to do
    d.resample_packed_dev(src.data_ptr(), n, s, 0, 0, 0)


# ---- the bipartitions ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tree(name, n):
    return nc.nj_numpy(nc.MATRICES[name](n))[0]


def _splits_on_device(d, n, trees):
    """The kernel over the join records of the trees, side by side; what lies behind the rows must stay."""
    import torch
    k, w = n - 3, bc.words(n)
    a = _dev(np.asarray([m[0] for t in trees for m in t], dtype=np.uint32))
    b = _dev(np.asarray([m[1] for t in trees for m in t], dtype=np.uint32))
    out = _filled(len(trees) * k * w + 8, MARK64, torch.int64)
    d.nj_splits_dev(a.data_ptr(), b.data_ptr(), n, len(trees), out.data_ptr())
    torch.cuda.synchronize()
    got = _host(out, np.uint64)
    assert (got[len(trees) * k * w:] == MARK64).all()
    return got[:len(trees) * k * w].reshape(len(trees), k, w)


@pytest.mark.parametrize("n", SIZES)
def test_the_bipartitions_of_join_records_are_the_bitsets_of_the_statement(n):
    d = get_device()
    names = ("random", "ties3", "zero", "line")
    for trees in [[_tree(name, n)] for name in names] + [[_tree(name, n) for name in names[:3]]]:       # T = 1 and T = 3
        got = _splits_on_device(d, n, trees)
        for t, merges in enumerate(trees):
            assert np.array_equal(got[t], bc.split_words(n, bc.splits(n, merges))), t
        if n % 64:
            assert not (got[:, :, -1] >> np.uint64(n % 64)).any()    # the complement leaves the tail of the last word zero
        assert not (got[:, :, 0] & np.uint64(1)).any()              # no row holds sample 0


def test_more_words_than_a_wave_has_lanes_need_no_second_thought_and_a_chain_into_slot_0_complements_every_step():
    """2 100 samples, every pair 2 apart: the tree is known without building it, (0, 1) and then slot 0 takes up 2, 3, ...: the set of
    the new node always holds sample 0, so every row is a complement: {t + 2, ..., n - 1} after join t."""
    d = get_device()
    n = 2100
    merges = nc.star_of_equal(n)[0]
    assert len(merges) == n - 3 and all(m[0] == 0 for m in merges)
    got = _splits_on_device(d, n, [merges])[0]
    everyone = (1 << n) - 1
    want = [everyone ^ ((1 << (t + 2)) - 1) for t in range(n - 3)]
    assert want == bc.splits(n, merges)
    assert np.array_equal(got, bc.split_words(n, want))


def test_records_that_name_no_slot_touch_nothing_and_small_trees_have_no_row():
    import torch
    d = get_device()
    n = 70
    a = _dev(np.asarray([1] * (n - 3), dtype=np.uint32))
    b = _dev(np.asarray([n + 5] * (n - 3), dtype=np.uint32))
    out = _filled((n - 3) * 2 + 8, MARK64, torch.int64)
    d.nj_splits_dev(a.data_ptr(), b.data_ptr(), n, 1, out.data_ptr())
    torch.cuda.synchronize()
    got = _host(out, np.uint64)
    assert not got[:(n - 3) * 2].any() and (got[(n - 3) * 2:] == MARK64).all()
    for small in (0, 1, 2, 3):
        d.nj_splits_dev(0, 0, small, 5, 0)
    d.nj_splits_dev(0, 0, 9, 0, 0)


# ---- the support counts ----------------------------------------------------------------------------------------------------------
def _support_on_device(d, n, main, rows):
    import torch
    w = bc.words(n)
    main_rows, rep_rows = bc.split_words(n, main), bc.split_words(n, rows)
    d_main, d_rep = _dev(main_rows), _dev(rep_rows if len(rows) else np.zeros(1, dtype=np.uint64))
    counts = _filled(len(main) + 8, MARK, torch.int32)
    d.split_support_dev(d_main.data_ptr(), len(main), d_rep.data_ptr() if len(rows) else 0, len(rows), w, counts.data_ptr())
    torch.cuda.synchronize()
    got = _host(counts, np.uint32)
    assert (got[len(main):] == MARK).all()                           # what lies behind the counts stays
    assert np.array_equal(_host(d_main, np.uint64).reshape(main_rows.shape), main_rows)
    return got[:len(main)].tolist()


def _sharing_the_cherries(n, main):
    """Rows that are no tree's: the cherries of the main tree as they are, every other bipartition with one sample moved so that it
    is none of the main tree's."""
    have, out = set(main), []
    for x in main:
        if bin(x).count("1") == 2 or bin(x).count("1") == n - 2:
            out.append(x)
            continue
        out.append(next(x ^ (1 << i) for i in range(1, n) if (x ^ (1 << i)) not in have))
    return out


@pytest.mark.parametrize("n", SIZES)
def test_the_counts_are_the_counts_of_the_statement(n):
    import collections
    d = get_device()
    main = bc.splits(n, _tree("random", n))
    other = bc.splits(n, _tree("ties3", n))
    cherries = _sharing_the_cherries(n, main)
    for rows in (main, main + main + main, other, cherries, main + other + cherries, []):
        have = collections.Counter(rows)
        assert _support_on_device(d, n, main, rows) == [have[x] for x in main], len(rows)
    assert _support_on_device(d, n, main, cherries) == [1 if bin(x).count("1") in (2, n - 2) else 0 for x in main]
    assert _support_on_device(d, n, main, main + main) == [2] * (n - 3)


def test_rows_that_differ_in_one_word_alone_are_told_apart():
    """Three words: the search has to look at all of them, the first two being equal."""
    d = get_device()
    n = 190
    base = (1 << 70) | (1 << 3)
    main = [base | (1 << (128 + i)) for i in range(40)]
    rows = [base | (1 << (128 + i)) for i in (0, 39, 39, 17, 45, 50)] + [base, base | (1 << 100) | (1 << 128)]
    assert _support_on_device(d, n, main, rows) == [1 if i in (0, 17) else 2 if i == 39 else 0 for i in range(40)]


# ---- the host form ---------------------------------------------------------------------------------------------------------------
def _check(d, sym, replicates, seed, want):
    got = d.nj_bootstrap(sym, replicates, seed)
    assert len(got) == 7 and got[6].dtype == np.uint32
    assert nc.tree_of_arrays(*got[:6]) == want[0] and got[6].tolist() == want[1]
    plain = d.nj(sym)
    assert all(np.array_equal(x, y) for x, y in zip(got[:4], plain[:4])) and got[4:6] == plain[4:6]      # the main tree is Device.nj's
    return got


def test_the_host_form_on_weak_and_on_strong_data():
    d = get_device()
    got = _check(d, bc.planted(), 8, 1, bc.planted_bootstrap())
    assert sorted(set(got[6].tolist())) == list(range(9))
    again = d.nj_bootstrap(bc.planted(), 8, 1)
    assert all(np.array_equal(x, y) for x, y in zip(got[:4] + (got[6],), again[:4] + (again[6],))) and got[4:6] == again[4:6]
    other = bc.differing_seed()
    moved = _check(d, bc.planted(), 8, other, bc.planted_bootstrap(other))
    assert moved[6].tolist() != got[6].tolist()
    strong = _check(d, bc.additive_symbols(), 8, 1, bc.additive_bootstrap())
    assert strong[6].tolist() == [8] * 62
    with_matrix = d.nj_bootstrap(bc.planted(), 1, 1, want_matrix=True)
    assert np.array_equal(with_matrix[7], bc.distance_matrix(bc.planted()))


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5])
def test_the_smallest_trees(n):
    d = get_device()
    sym = np.ascontiguousarray(bc.planted()[20:20 + n * 6:6])        # one sample of n groups
    assert sym.shape[0] == n
    got = _check(d, sym, 2, 1, bc.bootstrap(sym, 2, 1))
    assert len(got[6]) == max(n - 3, 0)


def test_mixed_case_and_missing_bytes_are_resampled_as_they_are_compared():
    d = get_device()
    sym = bc.planted()[:40].copy()
    rng = np.random.default_rng(11)
    sym[rng.random(sym.shape) < 0.3] |= 0x20
    sym[rng.random(sym.shape) < 0.05] = ord("N")
    sym[rng.random(sym.shape) < 0.05] = ord("-")
    _check(d, sym, 3, 5, bc.bootstrap(sym, 3, 5))


def test_without_a_column_every_matrix_is_zero_and_every_join_has_full_support():
    d = get_device()
    n = 9
    sym = np.zeros((n, 0), dtype=np.uint8)
    got = d.nj_bootstrap(sym, 5, 1)
    assert nc.tree_of_arrays(*got[:6]) == nc.nj_numpy(np.zeros((n, n), dtype=np.int32)) and got[6].tolist() == [5] * (n - 3)


def test_no_replicate_is_refused_before_any_output_is_written():
    from snp_pipeline_amd import _lib as L
    from snp_pipeline_amd.device import SnpGpuError
    d = get_device()
    sym = np.ascontiguousarray(bc.planted()[:10])
    with pytest.raises(SnpGpuError) as ei:
        d.nj_bootstrap(sym, 0)
    assert ei.value.code == L.E_ARG and "replicate" in str(ei.value)
    a, b, support = (np.full(7, MARK, dtype=np.uint32) for _ in range(3))
    la, lb = (np.full(7, MARK64, dtype=np.int64) for _ in range(2))
    star, star_len, n_merges = np.full(3, MARK, dtype=np.uint32), np.full(3, MARK64, dtype=np.int64), C.c_uint32(MARK)
    ptr = lambda x: C.c_void_p(x.ctypes.data)                        # noqa: E731
    rc = d.lib.snpgpu_nj_bootstrap(d.ctx, ptr(sym), 10, sym.shape[1], 0, 1, ptr(a), ptr(b), ptr(la), ptr(lb), None, ptr(star), ptr(star_len), C.byref(n_merges), ptr(support))
    assert rc == L.E_ARG and n_merges.value == MARK
    assert all((x == MARK).all() for x in (a, b, support, star)) and all((x == MARK64).all() for x in (la, lb, star_len))
    rc = d.lib.snpgpu_nj_bootstrap(d.ctx, ptr(sym), 10, sym.shape[1], 3, 1, ptr(a), ptr(b), ptr(la), ptr(lb), None, ptr(star), ptr(star_len), C.byref(n_merges), None)
    assert rc == L.E_ARG and n_merges.value == MARK and (star == MARK).all()      # a null output likewise
