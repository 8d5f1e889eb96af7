"""The kernels of csrc/compared.hip — the valid plane of a packed matrix, the q x n block of compared-site counts of two planes,
the counts of listed pairs — and the library's host forms, against the plain statements of tests/compared_cases.py.  Everything
is compared exactly, and what lies behind an output must keep the mark it was filled with."""
import functools
import os
import re

import numpy as np
import pytest

from tests import clusters_cases as cc
from tests import compared_cases as pc
from tests import nearest_cases as nc
from tests.gpu_util import get_device

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARK = -7
SLAB = 16 * 32                                                      # sites of one slab of the tile kernel: CMP_KW words
TILE = 128
PLANE_SITES = (1, 31, 32, 33, 127, 128, 129, SLAB - 1, SLAB, SLAB + 1, 2 * SLAB - 1, 2 * SLAB, 2 * SLAB + 1)
QS = (1, 2, 127, 128, 129, 257)
NS = (1, 127, 128, 129, 257, 300)


def test_the_constants_restated_here_are_the_kernels():
    src = open(os.path.join(ROOT, "snp_pipeline_amd", "csrc", "compared.hip")).read()
    assert int(re.search(r"#define CMP_KW (\d+)", src).group(1)) * 32 == SLAB
    assert int(re.search(r"#define CMP_TILE (\d+)", src).group(1)) == TILE
    assert int(re.search(r"#define CMP_PAIR_GRID_CAP (\d+)", src).group(1)) * 4 < 70000
    d = get_device()
    assert [d.valid_plane_row_bytes(s) for s in (0, 1, SLAB, SLAB + 1)] == [0, 64, 64, 128]


def _cu():
    import torch
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _pack(d, sym):
    import torch
    sym_t = torch.from_numpy(np.array(sym, dtype=np.uint8, order="C")).cuda()
    n, s = sym.shape
    pk = torch.full((n, d.packed_row_bytes(s)), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    d.pack_matrix_dev(sym_t.data_ptr(), n, s, s, pk.data_ptr())
    d.sync()
    return pk


def _plane(d, sym, behind=64):
    """The plane of the symbols in a destination filled with 0xA5, `behind` more bytes after its last row."""
    import torch
    n, s = sym.shape
    pk = _pack(d, sym)
    row = d.valid_plane_row_bytes(s)
    out = torch.full((n * row + behind,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    d.valid_plane_dev(pk.data_ptr(), n, s, out.data_ptr())
    d.sync()
    return out


def _rect(d, pl_q, q, pl_db, n, s, pitch_extra=3, rows_extra=2):
    """The (q + rows_extra, n + pitch_extra) output, filled with MARK before the call."""
    import torch
    out = torch.full((q + rows_extra, n + pitch_extra), MARK, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    d.compared_rect_dev(pl_q.data_ptr(), q, pl_db.data_ptr(), n, s, out.data_ptr(), out_stride=n + pitch_extra)
    d.sync()
    return out.cpu().numpy()


def _check(got, want, where):
    q, n = want.shape
    assert np.array_equal(got[:q, :n], want), where
    assert (got[q:] == MARK).all() and (got[:, n:] == MARK).all(), where


# ------------------------------------------------------------------------------------------------ the plane
@pytest.mark.parametrize("every_byte", [False, True])
def test_the_plane_at_every_word_and_slab_edge(every_byte):
    d = get_device()
    sym = pc.random_symbols(5, max(PLANE_SITES), 51, every_byte)
    for s in PLANE_SITES:
        want = pc.valid_plane(sym[:, :s])
        row = d.valid_plane_row_bytes(s)
        assert row == want.shape[1] * 4 and row % 64 == 0
        got = _plane(d, sym[:, :s]).cpu().numpy()
        assert np.array_equal(got[:5 * row].view("<u4").reshape(5, -1), want), s
        assert (got[5 * row:] == 0xA5).all() and len(got) == 5 * row + 64, s        # the bytes behind the last row
        words = (s + 31) // 32
        assert (want[:, words:] == 0).all() and (every_byte or want[:, :words].any())  # (the padding words: zero over 0xA5)


# ------------------------------------------------------------------------------------------------ the block
@functools.lru_cache(maxsize=None)
def _symbols():
    q_sym, db_sym = pc.random_symbols(max(QS), 2400, 61), pc.random_symbols(max(NS), 2400, 62)
    q_sym[5], q_sym[6] = db_sym[9], db_sym[9]
    q_sym[6, ::7] ^= 0x20                                            # the other letter case: compared at the same columns
    q_sym[7, 40:] = 0x2D                                             # a query that ends early
    q_sym.setflags(write=False)
    db_sym.setflags(write=False)
    return q_sym, db_sym


@pytest.mark.parametrize("s", [1, 33, SLAB - 1, SLAB, SLAB + 1, 2400])
def test_every_shape_of_the_block(s):
    d = get_device()
    q_sym, db_sym = _symbols()
    want = pc.compared_rect(q_sym[:, :s], db_sym[:, :s])
    if s >= 33:                                                      # a kernel that returns another quantity cannot pass
        dist = nc.rect_distance(q_sym[:, :s], db_sym[:, :s])
        assert want.min() < want.max() and (want != s).any() and (want != dist).any() and (dist <= want).all()
        assert np.array_equal(want[5], want[6]) and want[7].max() <= 40
    pl_q, pl_db = _plane(d, q_sym[:, :s]), _plane(d, db_sym[:, :s])
    for q in QS:
        for n in NS:
            _check(_rect(d, pl_q, q, pl_db, n, s), want[:q, :n], (q, n))


def test_a_pitch_and_rows_behind_the_output_survive_and_no_sites_give_zeros():
    d = get_device()
    q_sym, db_sym = _symbols()
    pl_q, pl_db = _plane(d, q_sym[:, :513]), _plane(d, db_sym[:, :513])
    want = pc.compared_rect(q_sym[:17, :513], db_sym[:129, :513])
    _check(_rect(d, pl_q, 17, pl_db, 129, 513, pitch_extra=127, rows_extra=9), want, "pitch")
    _check(_rect(d, pl_q, 5, pl_db, 7, 0), np.zeros((5, 7), dtype=np.int32), "no sites")
    _check(_rect(d, pl_q, 5, pl_q, 5, 0), np.zeros((5, 5), dtype=np.int32), "no sites, square")


def test_the_kernel_goes_through_its_grid():
    """At least as many tiles as CUs at 96 sites: n follows from the CU count."""
    d = get_device()
    q = 129
    rows = (q + TILE - 1) // TILE
    n = TILE * ((_cu() + rows - 1) // rows - 1) + 1
    assert rows * ((n + TILE - 1) // TILE) >= _cu() and n % TILE == 1
    q_sym, db_sym = pc.random_symbols(q, 96, 71), pc.random_symbols(n, 96, 72)
    want = pc.compared_rect(q_sym, db_sym)
    assert want.min() < want.max() < 96
    _check(_rect(d, _plane(d, q_sym), q, _plane(d, db_sym), n, 96, pitch_extra=1), want, (q, n))


def test_bad_block_arguments_are_refused():
    import torch
    from snp_pipeline_amd.device import SnpGpuError
    d = get_device()
    q_sym, db_sym = _symbols()
    pl_q, pl_db = _plane(d, q_sym[:4, :33]), _plane(d, db_sym[:9, :33])
    out = torch.full((4, 16), MARK, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for args in ((pl_q.data_ptr(), 4, pl_db.data_ptr(), 9, 33, out.data_ptr(), 8),              # a pitch below n
                 (pl_q.data_ptr(), 4, pl_db.data_ptr(), 9, 33, out.data_ptr() + 2, 16),          # a misaligned output
                 (pl_q.data_ptr() + 4, 4, pl_db.data_ptr(), 9, 33, out.data_ptr(), 16),          # a misaligned plane
                 (0, 4, pl_db.data_ptr(), 9, 33, out.data_ptr(), 16),
                 (pl_q.data_ptr(), 4, 0, 9, 33, out.data_ptr(), 16),
                 (pl_q.data_ptr(), 4, pl_db.data_ptr(), 9, 33, 0, 16)):
        with pytest.raises(SnpGpuError):
            d.compared_rect_dev(*args[:6], out_stride=args[6])
    d.compared_rect_dev(0, 0, pl_db.data_ptr(), 9, 33, 0)                                       # nothing to do
    d.compared_rect_dev(pl_q.data_ptr(), 4, 0, 0, 33, 0)
    d.sync()
    assert (out.cpu().numpy() == MARK).all()


# ------------------------------------------------------------------------------------------------ the square block
@pytest.mark.parametrize("every_byte", [False, True])
def test_the_square_block_is_symmetric_with_the_own_counts_on_its_diagonal(every_byte):
    d = get_device()
    sym = pc.random_symbols(300, 777, 81, every_byte)
    sym[17] = 0x2D                                                   # a sample without a single base
    pl = _plane(d, sym)
    got = _rect(d, pl, 300, pl, 300, 777)
    want = pc.compared_rect(sym, sym)
    _check(got, want, every_byte)
    got = got[:300, :300]
    own = pc.valid_sites(sym).sum(axis=1)
    assert np.array_equal(got, got.T) and np.array_equal(np.diag(got), own)
    assert (got[17] == 0).all() and (got[:, 17] == 0).all() and got.max() > 0
    dist = d.distance(sym)
    assert (got >= dist).all() and (got <= np.minimum.outer(own, own)).all() and (got != dist).any()
    assert np.array_equal(d.compared(sym), want)


@pytest.mark.parametrize("every_byte", [False, True])
def test_the_square_and_the_rectangular_sweep_store_the_same_block(every_byte):
    """257 samples at one site past a slab: three tile rows, the last one row deep, and a second slab that is nearly empty.  The
    same plane twice takes the upper-triangle tiles and their mirror images; a copy of it at another address takes the plain grid."""
    d = get_device()
    n, s, pitch = 2 * TILE + 1, SLAB + 1, 300
    sym = pc.random_symbols(n, s, 83, every_byte)
    pl = _plane(d, sym)
    other = pl.clone()
    assert other.data_ptr() != pl.data_ptr()
    square = _rect(d, pl, n, pl, n, s, pitch_extra=pitch - n)
    rect = _rect(d, pl, n, other, n, s, pitch_extra=pitch - n)
    assert square.shape == (n + 2, pitch) and np.array_equal(square, rect)
    want = pc.compared_rect(sym, sym)
    assert want.min() < want.max()
    _check(square, want, "square")
    _check(rect, want, "rectangular")


def test_a_matrix_of_bases_alone_is_compared_everywhere():
    d = get_device()
    sym = np.frombuffer(b"ACGTacgt", dtype=np.uint8)[np.random.default_rng(82).integers(0, 8, size=(130, 1025))]
    pl = _plane(d, sym)
    _check(_rect(d, pl, 130, pl, 130, 1025), np.full((130, 130), 1025, dtype=np.int32), "all bases")
    assert (d.compared(sym) == 1025).all()


# ------------------------------------------------------------------------------------------------ listed pairs
def _pairs(d, pl_a, n_a, pl_b, n_b, s, a, b, behind=4):
    """out[p] of the device form in an output filled with MARK, `behind` more entries after the last pair."""
    import torch
    m = len(a)
    a_t = torch.from_numpy(np.asarray(a, dtype=np.int32)).cuda()
    b_t = torch.from_numpy(np.asarray(b, dtype=np.int32)).cuda()
    out = torch.full((m + behind,), MARK, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    try:
        d.compared_pairs_dev(pl_a.data_ptr(), n_a, pl_b.data_ptr(), n_b, s, a_t.data_ptr(), b_t.data_ptr(), m, out.data_ptr())
    finally:
        d.sync()
        got = out.cpu().numpy()
    assert (got[m:] == MARK).all()
    return got[:m]


def _pair_lists(m, n_a, n_b, seed):
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, n_a, size=m), rng.integers(0, n_b, size=m)
    if m >= 63:
        a[:8], b[:8] = (3, 3, 9, 9, 8, 7, 6, 5), (3, 3, 2, 2, 8, 7, 6, 5)         # a = b, repeated pairs, descending order
        a[-1], b[-1] = n_a - 1, n_b - 1
    return a, b


@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 70000])
def test_pairs_against_one_matrix_and_against_two(m):
    """70 000 pairs at 40 sites: more than the 4 096 waves of the grid, so every wave goes round its loop."""
    d = get_device()
    s = 40 if m == 70000 else 777
    sym_a, sym_b = pc.random_symbols(21, s, 91), pc.random_symbols(13, s, 92)
    pl_a, pl_b = _plane(d, sym_a), _plane(d, sym_b)
    one, two = pc.compared_rect(sym_a, sym_a), pc.compared_rect(sym_a, sym_b)
    assert one.min() < one.max() and two.min() < two.max()
    a, b = _pair_lists(m, 21, 21, 93)
    assert np.array_equal(_pairs(d, pl_a, 21, pl_a, 21, s, a, b), one[a, b]), "one matrix"
    a, b = _pair_lists(m, 21, 13, 94)
    first = _pairs(d, pl_a, 21, pl_b, 13, s, a, b)
    assert np.array_equal(first, two[a, b]), "two matrices"
    assert first.tobytes() == _pairs(d, pl_a, 21, pl_b, 13, s, a, b).tobytes()
    if m in (65, 70000):
        assert np.array_equal(d.compared_pairs(sym_a, a, b, sym_b), two[a, b])
        assert np.array_equal(pc.compared_pairs(sym_a, a[:65], b[:65], sym_b), two[a[:65], b[:65]])


@pytest.mark.parametrize("every_byte", [False, True])
def test_pairs_at_every_word_and_slab_edge(every_byte):
    d = get_device()
    sym = pc.random_symbols(11, max(PLANE_SITES), 95, every_byte)
    a, b = _pair_lists(65, 11, 11, 96)
    for s in PLANE_SITES:
        pl = _plane(d, sym[:, :s])
        assert np.array_equal(_pairs(d, pl, 11, pl, 11, s, a, b), pc.compared_pairs(sym[:, :s], a, b)), s
    pl = _plane(d, sym)
    assert (_pairs(d, pl, 11, pl, 11, 0, a, b) == 0).all()            # no sites: nothing was compared


def test_a_pair_outside_its_matrix_is_refused_and_nothing_is_written():
    from snp_pipeline_amd.device import SnpGpuError
    d = get_device()
    sym_a, sym_b = pc.random_symbols(21, 100, 97), pc.random_symbols(13, 100, 98)
    pl_a, pl_b = _plane(d, sym_a), _plane(d, sym_b)
    for at, (bad_a, bad_b) in ((0, (21, 0)), (69, (0, 13)), (35, (20, 20))):
        a, b = _pair_lists(70, 21, 13, 99)
        a[at], b[at] = bad_a, bad_b
        import torch
        a_t, b_t = torch.from_numpy(a.astype(np.int32)).cuda(), torch.from_numpy(b.astype(np.int32)).cuda()
        out = torch.full((74,), MARK, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(SnpGpuError):
            d.compared_pairs_dev(pl_a.data_ptr(), 21, pl_b.data_ptr(), 13, 100, a_t.data_ptr(), b_t.data_ptr(), 70, out.data_ptr())
        d.sync()
        assert (out.cpu().numpy() == MARK).all(), at
        host = np.full(70, MARK, dtype=np.int32)
        a32, b32 = a.astype(np.uint32), b.astype(np.uint32)
        rc = d.lib.snpgpu_compared_pairs(d.ctx, sym_a.ctypes.data, 21, sym_b.ctypes.data, 13, 100, a32.ctypes.data, b32.ctypes.data, 70, host.ctypes.data)
        assert rc != 0 and (host == MARK).all(), at
        with pytest.raises(ValueError):
            d.compared_pairs(sym_a, a, b, sym_b)
    a, b = _pair_lists(70, 21, 13, 99)                               # 20 is a row of the first matrix, not of the second
    assert a[-1] == 20
    with pytest.raises(ValueError):
        d.compared_pairs(sym_b, a, b)


# ------------------------------------------------------------------------------------------------ host forms
def test_the_host_forms_are_the_device_forms_on_the_listeria_matrix(fixture_trees):
    d = get_device()
    tree = fixture_trees["listeria"][0]
    ids, mat = cc.read_matrix_tsv(os.path.join(tree, "snp_distance_matrix.tsv"))
    fasta_ids, rows = nc.read_fasta_rows(os.path.join(tree, "snpma.fasta"))
    assert fasta_ids == ids and rows.shape == (48, 10102)
    pl = _plane(d, rows)
    block = _rect(d, pl, 48, pl, 48, 10102)[:48, :48]
    want = pc.compared_rect(rows, rows)
    host = d.compared(rows)
    assert host.dtype == np.int32 and np.array_equal(host, block) and np.array_equal(host, want)
    assert np.diag(host).min() == 9974 and np.diag(host).max() == 10102 and (mat <= host).all()
    a, b = _pair_lists(200, 48, 48, 100)
    listed = d.compared_pairs(rows, a, b)
    assert listed.dtype == np.int32 and np.array_equal(listed, _pairs(d, pl, 48, pl, 48, 10102, a, b)) and np.array_equal(listed, want[a, b])
    assert np.array_equal(d.compared_pairs(rows[::3], a % 16, b, rows), want[::3][a % 16, b])
    assert d.compared(rows[:0]).shape == (0, 0) and (d.compared(rows[:4, :0]) == 0).all() and len(d.compared_pairs(rows, [], [])) == 0
