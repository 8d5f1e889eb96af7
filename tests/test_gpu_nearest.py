"""The kernels of csrc/nearest.hip — the q x n distances of two packed matrices on both tile routes, and the selection of the K
closest entries of a row within T — and the library's host form, against the plain statements of tests/nearest_cases.py.
Everything is compared exactly: whole matrices, offsets, columns, distances, and what lies behind the outputs.

A case that is meant for one kernel variant restates the dispatcher's condition (snpgpu_distance_rect_packed_dev) from the device's
CU count and asserts it, so that a change of the heuristic cannot quietly move the case to the other kernel."""
import functools
import os
import re

import numpy as np
import pytest

from tests import clusters_cases as cc
from tests import nearest_cases as nc
from tests.gpu_util import get_device

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARK = -7
NARROW, TILE = 1, 2
QS = (1, 2, 15, 16, 17, 127, 128, 129, 257)
NS = (1, 127, 128, 129, 255, 256, 257, 300)
SHAPE = {NARROW: (16, 64, 16), TILE: (128, 128, 4)}                # query rows, database rows, words per slab
NARROW_PER_CU = 160 * 1024 // (2 * (64 + 16) * 16 * 16)            # workgroups of the narrow route a CU's LDS holds


def _cu():
    import torch
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _plan(q, n, s, route):
    """What snpgpu_distance_rect_packed_dev launches for this shape, restated."""
    tq, tn, kw = SHAPE[route]
    tiles = ((q + tq - 1) // tq) * ((n + tn - 1) // tn)
    words = ((s + 31) // 32 + 3) // 4 * 4
    p = {"tiles": tiles, "words": words, "kind": "direct"}
    if tiles < _cu() and words >= 4 * kw:
        want = NARROW_PER_CU * _cu() // tiles if route == NARROW else (2 * _cu() + tiles - 1) // tiles
        parts = min(want, words // (2 * kw))
        chunk = ((words + parts - 1) // parts + kw - 1) // kw * kw
        p.update(kind="split", k_chunk=chunk, k_parts=(words + chunk - 1) // chunk)
    return p


def _pack(d, sym):
    import torch
    sym_t = torch.from_numpy(np.array(sym, dtype=np.uint8, order="C")).cuda()
    n, s = sym.shape
    pk = torch.full((n, d.packed_row_bytes(s)), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    d.pack_matrix_dev(sym_t.data_ptr(), n, s, s, pk.data_ptr())
    d.sync()
    return pk


def _rect(d, pk_q, q, pk_db, n, s, route, pitch_extra=3, rows_extra=2):
    """The (q + rows_extra, n + pitch_extra) output, filled with MARK before the call."""
    import torch
    out = torch.full((q + rows_extra, n + pitch_extra), MARK, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    d.distance_rect_dev(pk_q.data_ptr(), q, pk_db.data_ptr(), n, s, out.data_ptr(), out_stride=n + pitch_extra, route=route)
    d.sync()
    return out.cpu().numpy()


def _check(got, want, where):
    q, n = want.shape
    assert np.array_equal(got[:q, :n], want), where
    assert (got[q:] == MARK).all() and (got[:, n:] == MARK).all(), where


@functools.lru_cache(maxsize=None)
def _symbols():
    q_sym, db_sym = nc.random_symbols(max(QS), 2400, 21), nc.random_symbols(max(NS), 2400, 22)
    q_sym[5], q_sym[6] = db_sym[9], db_sym[9]                       # two queries that are a database sample
    q_sym[6, ::7] ^= 0x20                                            # ... one of them in the other letter case
    q_sym.setflags(write=False)
    db_sym.setflags(write=False)
    return q_sym, db_sym


@functools.lru_cache(maxsize=None)
def _want(s):
    q_sym, db_sym = _symbols()
    want = nc.rect_distance(q_sym[:, :s], db_sym[:, :s])
    want.setflags(write=False)
    return want


# s: one site; a word and one site (a short narrow slab); the longest row the tile route does not split; the first it splits and a
# full narrow slab; the first the narrow route splits; narrow chunks of 48 and 28 words, the last slab short
@pytest.mark.parametrize("route", [NARROW, TILE])
@pytest.mark.parametrize("s", [1, 33, 384, 385, 2000, 2400])
def test_every_shape_on_both_routes(route, s):
    d = get_device()
    q_sym, db_sym = _symbols()
    want = _want(s)
    assert want[5, 9] == want[6, 9] == 0 and (s == 1 or want.max() > 0)
    assert _plan(257, 300, 384, TILE)["kind"] == "direct" and _plan(257, 300, 385, TILE)["kind"] == "split"
    assert _plan(257, 300, 385, NARROW)["kind"] == "direct" and _plan(257, 300, 2000, NARROW)["kind"] == "split"
    assert (lambda p: (p["k_chunk"], p["k_parts"], p["words"]))(_plan(1, 300, 2400, NARROW)) == (48, 2, 76)
    pk_q, pk_db = _pack(d, q_sym[:, :s]), _pack(d, db_sym[:, :s])
    for q in QS:
        for n in NS:
            _check(_rect(d, pk_q, q, pk_db, n, s, route), want[:q, :n], (q, n))
    # auto: one route for few queries, the other for many; both give the same numbers anyway
    for q in (16, 17, 32, 33):
        _check(_rect(d, pk_q, q, pk_db, 300, s, 0), want[:q, :300], q)


@pytest.mark.parametrize("route", [NARROW, TILE])
def test_the_unsplit_kernel_goes_through_its_grid(route):
    """At least as many tiles as CUs, so that 96 sites are not split: n follows from the CU count."""
    d = get_device()
    tq, tn, _ = SHAPE[route]
    q = 33 if route == NARROW else 129
    rows = (q + tq - 1) // tq
    n = tn * ((_cu() + rows - 1) // rows - 1) + 1
    p = _plan(q, n, 96, route)
    assert p["kind"] == "direct" and p["tiles"] >= _cu() and n % tn == 1
    q_sym, db_sym = nc.random_symbols(q, 96, 31), nc.random_symbols(n, 96, 32)
    want = nc.rect_distance(q_sym, db_sym)
    _check(_rect(d, _pack(d, q_sym), q, _pack(d, db_sym), n, 96, route, pitch_extra=1), want, (q, n))


@pytest.mark.parametrize("route", [NARROW, TILE])
def test_the_square_block_is_the_symmetric_matrix_and_every_byte_counts_as_there(route):
    d = get_device()
    for every_byte in (False, True):
        sym = nc.random_symbols(300, 777, 41, every_byte)
        pk = _pack(d, sym)
        got = _rect(d, pk, 300, pk, 300, 777, route)
        want = d.distance(sym)
        _check(got, want, every_byte)
        assert np.array_equal(want, nc.rect_distance(sym, sym)) and (np.diag(want) == 0).all()


def test_a_pitch_and_rows_behind_the_output_survive_and_no_sites_give_zeros():
    d = get_device()
    q_sym, db_sym = _symbols()
    pk_q, pk_db = _pack(d, q_sym[:, :385]), _pack(d, db_sym[:, :385])
    for route in (NARROW, TILE):
        _check(_rect(d, pk_q, 17, pk_db, 129, 385, route, pitch_extra=127, rows_extra=9), _want(385)[:17, :129], route)
        zero = _rect(d, pk_q, 5, pk_db, 7, 0, route)
        _check(zero, np.zeros((5, 7), dtype=np.int32), route)


def test_bad_rect_arguments_are_refused():
    import torch
    from snp_pipeline_amd.device import SnpGpuError
    d = get_device()
    q_sym, db_sym = _symbols()
    pk_q, pk_db = _pack(d, q_sym[:4, :33]), _pack(d, db_sym[:9, :33])
    out = torch.full((4, 16), MARK, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for args in ((pk_q.data_ptr(), 4, pk_db.data_ptr(), 9, 33, out.data_ptr(), 8, 0),            # a pitch below n
                 (pk_q.data_ptr(), 4, pk_db.data_ptr(), 9, 33, out.data_ptr() + 2, 16, 0),        # a misaligned output
                 (pk_q.data_ptr() + 4, 4, pk_db.data_ptr(), 9, 33, out.data_ptr(), 16, 0),        # a misaligned packed matrix
                 (0, 4, pk_db.data_ptr(), 9, 33, out.data_ptr(), 16, 0),
                 (pk_q.data_ptr(), 4, 0, 9, 33, out.data_ptr(), 16, 0),
                 (pk_q.data_ptr(), 4, pk_db.data_ptr(), 9, 33, 0, 16, 0)):
        with pytest.raises(SnpGpuError):
            d.distance_rect_dev(*args[:6], out_stride=args[6], route=args[7])
    for route in (3, -1):
        with pytest.raises(SnpGpuError):
            d._check(d.lib.snpgpu_distance_rect_packed_dev(d.ctx, pk_q.data_ptr(), 4, pk_db.data_ptr(), 9, 33, route, out.data_ptr(), 16))
    with pytest.raises(ValueError):
        d.distance_rect_dev(pk_q.data_ptr(), 4, pk_db.data_ptr(), 9, 33, out.data_ptr(), route="wide")
    d.distance_rect_dev(0, 0, pk_db.data_ptr(), 9, 33, 0)                                       # nothing to do
    d.distance_rect_dev(pk_q.data_ptr(), 4, 0, 0, 33, 0)
    d.sync()
    assert (out.cpu().numpy() == MARK).all()


# ------------------------------------------------------------------------------------------------ selection
def _select(d, mat, k, t, pitch_extra=3, capacity=None, pad=-1):
    """(row_off, col, dist, total, raw bytes) of snpgpu_nearest_dev over a matrix with -1 in its padding; what lies behind the
    outputs must stay untouched."""
    import torch
    q, n = mat.shape
    host = np.full((q, n + pitch_extra), pad, dtype=np.int32)
    host[:, :n] = mat
    dev_mat = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    total = d.nearest_dev(dev_mat.data_ptr(), q, n, n + pitch_extra, k, t)
    cap = max(total, 1) if capacity is None else capacity             # (capacity 0 would only count)
    off = torch.full((q + 1 + 4,), MARK, dtype=torch.int64, device="cuda")
    col = torch.full((max(cap, 1) + 4,), MARK, dtype=torch.int32, device="cuda")
    dist = torch.full((max(cap, 1) + 4,), MARK, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    again = d.nearest_dev(dev_mat.data_ptr(), q, n, n + pitch_extra, k, t, capacity=cap, d_row_off=off.data_ptr(), d_col=col.data_ptr(), d_dist=dist.data_ptr())
    d.sync()
    assert again == total
    off, col, dist = off.cpu().numpy(), col.cpu().numpy(), dist.cpu().numpy()
    return off, col, dist, total, b"".join(a.tobytes() for a in (off, col, dist))


def _check_select(d, mat, k, t, where):
    q = mat.shape[0]
    want_off, want_col, want_dist = nc.nearest_of_matrix(mat, k, t)
    off, col, dist, total, _ = _select(d, mat, k, t)
    assert total == int(want_off[-1]), where
    assert np.array_equal(off[:q + 1].view(np.uint64), want_off) and (off[q + 1:] == MARK).all(), where
    assert np.array_equal(col[:total].view(np.uint32), want_col) and (col[total:] == MARK).all(), where
    assert np.array_equal(dist[:total], want_dist) and (dist[total:] == MARK).all(), where


def _matrices(n):
    rng = np.random.default_rng(100 + n)
    spread = rng.integers(-50, 1000, size=(3, n)).astype(np.int32)
    two = (rng.integers(0, 2, size=(3, n)) * 40 + 10).astype(np.int32)            # 10 and 50: every cut lies inside a tie
    equal = np.full((2, n), 25, dtype=np.int32)
    edge = rng.integers(-3, 3, size=(3, n)).astype(np.int32)
    edge[0, ::3] = nc.INT_MAX
    edge[1, ::2] = -nc.INT_MAX - 1
    edge[2] = nc.INT_MAX
    return {"spread": spread, "two": two, "equal": equal, "edge": edge}


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1100])
def test_selection_at_every_size(n):
    """A workgroup covers 256 columns in one pass: 257 and 1100 go round its loop."""
    src = open(os.path.join(ROOT, "snp_pipeline_amd", "csrc", "nearest.hip")).read()
    assert int(re.search(r"#define NEAREST_THREADS (\d+)", src).group(1)) == 256
    d = get_device()
    for kind, mat in _matrices(n).items():
        middle = int(np.sort(mat, axis=None)[mat.size // 2])
        for k in sorted({0, 1, 2, max(n - 1, 0), n, n + 5}):
            for t in (0, middle, None, nc.INT_MAX, int(mat.min()) - 1 if mat.min() > -nc.INT_MAX - 1 else None):
                _check_select(d, mat, k, t, (kind, k, t))


def test_an_all_equal_row_takes_its_first_columns_and_a_two_valued_row_cuts_inside_the_tie():
    d = get_device()
    equal = np.full((2, 700), 25, dtype=np.int32)
    off, col, dist, total, _ = _select(d, equal, 300, None)
    assert total == 600 and list(col[:300]) == list(range(300)) and list(col[300:600]) == list(range(300)) and (dist[:600] == 25).all()
    two = np.full((1, 700), 50, dtype=np.int32)
    two[0, 5::10] = 10                                               # 70 entries of 10, 630 of 50
    off, col, dist, total, _ = _select(d, two, 100, None)
    fifty = [j for j in range(700) if j % 10 != 5][:30]
    assert total == 100 and list(col[:70]) == list(range(5, 700, 10)) and list(col[70:100]) == fifty
    assert list(dist[:100]) == [10] * 70 + [50] * 30


def test_the_padding_is_never_chosen():
    """-1 lies between n and the pitch of every row: below every entry, so a read past n would win every selection."""
    d = get_device()
    mat = np.random.default_rng(7).integers(0, 90, size=(4, 300)).astype(np.int32)
    for pitch_extra in (1, 2, 3, 212):
        off, col, dist, total, _ = _select(d, mat, 5, None, pitch_extra=pitch_extra)
        want = nc.nearest_of_matrix(mat, 5, None)
        assert total == 20 and np.array_equal(col[:20].view(np.uint32), want[1]) and np.array_equal(dist[:20], want[2]) and dist[:20].min() >= 0


def test_more_rows_than_the_grid_holds():
    src = open(os.path.join(ROOT, "snp_pipeline_amd", "csrc", "nearest.hip")).read()
    assert int(re.search(r"#define NEAREST_ROW_GRID_CAP (\d+)", src).group(1)) == 1024
    d = get_device()
    mat = np.random.default_rng(8).integers(0, 12, size=(1100, 70)).astype(np.int32)
    for k, t in ((3, None), (0, 2), (70, 11)):
        _check_select(d, mat, k, t, (k, t))


def test_the_capacity_protocol_and_the_same_bytes_twice():
    import torch
    d = get_device()
    mat = np.random.default_rng(9).integers(0, 30, size=(9, 400)).astype(np.int32)
    want = nc.nearest_of_matrix(mat, 7, 12)
    total = int(want[0][-1])
    assert 0 < total <= 63
    first = _select(d, mat, 7, 12)
    assert first[3] == total and first[4] == _select(d, mat, 7, 12)[4]
    # too little room: the count, and nothing else
    off, col, dist, got_total, _ = _select(d, mat, 7, 12, capacity=total - 1)
    assert got_total == total and (off == MARK).all() and (col == MARK).all() and (dist == MARK).all()
    # no rows or no columns: no entries, offsets all zero
    off = torch.full((8,), MARK, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert d.nearest_dev(0, 0, 5, 5, 3, None, capacity=4, d_row_off=off.data_ptr()) == 0
    assert d.nearest_dev(0, 6, 0, 0, 3, None, capacity=4, d_row_off=off.data_ptr()) == 0
    d.sync()
    assert list(off.cpu().numpy()) == [0] * 7 + [MARK]


def test_bad_selection_arguments_are_refused():
    import torch
    from snp_pipeline_amd.device import SnpGpuError
    d = get_device()
    mat = torch.zeros((4, 16), dtype=torch.int32, device="cuda")
    off = torch.zeros(5, dtype=torch.int64, device="cuda")
    col = torch.zeros(64, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(SnpGpuError):
        d.nearest_dev(mat.data_ptr(), 4, 16, 15)                                               # a pitch below n
    with pytest.raises(SnpGpuError):
        d.nearest_dev(mat.data_ptr() + 2, 4, 8, 16)                                            # a misaligned matrix
    with pytest.raises(SnpGpuError):
        d.nearest_dev(0, 4, 16, 16)                                                             # no matrix
    with pytest.raises(SnpGpuError):
        d.nearest_dev(mat.data_ptr(), 4, 16, 16, 2, None, capacity=64, d_row_off=0, d_col=col.data_ptr(), d_dist=col.data_ptr())
    with pytest.raises(SnpGpuError):
        d.nearest_dev(mat.data_ptr(), 4, 16, 16, 2, None, capacity=64, d_row_off=off.data_ptr(), d_col=0, d_dist=col.data_ptr())
    assert d.nearest_dev(mat.data_ptr(), 4, 16, 16, 2, None) == 8


# ------------------------------------------------------------------------------------------------ host form
@pytest.fixture(scope="module")
def listeria(fixture_trees):
    tree = fixture_trees["listeria"][0]
    ids, mat = cc.read_matrix_tsv(os.path.join(tree, "snp_distance_matrix.tsv"))
    fasta_ids, rows = nc.read_fasta_rows(os.path.join(tree, "snpma.fasta"))
    assert fasta_ids == ids and len(ids) == 48
    return ids, rows, mat


@pytest.mark.parametrize("step", [3, 1])
def test_the_host_form_gives_the_rows_of_the_reference_table(listeria, step):
    d = get_device()
    ids, rows, mat = listeria
    for k in (1, 3, 5):
        for t in (None, 20):
            want = nc.nearest_of_matrix(mat[::step], k, t)
            for route in (NARROW, TILE):
                got = d.nearest(rows[::step], rows, k=k, threshold=t, route=route, want_matrix=True)
                assert all(np.array_equal(a, b) for a, b in zip(got[:3], want)), (k, t, route)
                assert np.array_equal(got[3], mat[::step])
            banded = d.nearest(rows[::step], rows, k=k, threshold=t, band_rows=5)
            assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(banded, want)), (k, t)
    everything = d.nearest(rows[::step], rows)
    assert all(np.array_equal(a, b) for a, b in zip(everything, nc.nearest_of_matrix(mat[::step])))


def test_the_host_form_without_rows_and_its_refusals(listeria):
    from snp_pipeline_amd.device import SnpGpuError
    d = get_device()
    ids, rows, mat = listeria
    off, col, dist = d.nearest(rows[:0], rows, k=3)
    assert list(off) == [0] and len(col) == len(dist) == 0
    off, col, dist, m = d.nearest(rows[:4], rows[:0], k=3, want_matrix=True)
    assert list(off) == [0] * 5 and len(col) == 0 and m.shape == (4, 0)
    with pytest.raises(ValueError):
        d.nearest(rows[:4, :100], rows, k=3)
    with pytest.raises(ValueError):
        d.nearest(rows[:4], rows, k=3, route=7)
    with pytest.raises(ValueError):
        d.nearest(rows[:4], rows, k=-1)
    with pytest.raises(SnpGpuError):
        d._check(d.lib.snpgpu_nearest(d.ctx, None, 4, None, 48, rows.shape[1], 3, 5, 0, 0, 0, None, None, None, None, None))
