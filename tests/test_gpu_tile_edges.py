"""The distance kernels (csrc/distance.hip) and the sort / scan primitives (csrc/prims.h under csrc/regions.hip) at the edges
of their tiles, slabs, chunks and passes.  Every distance case compares the WHOLE matrix with oracle/distance_ref.py (checked
against the site-by-site statements in tests/test_distance_ref.py, and here once more against numpy on a block of the very
input), every sort / scan case compares the whole output with numpy / oracle.steps_oracle.  No tolerance anywhere.

A case that is meant for one kernel variant restates the dispatcher's condition (snpgpu_distance_packed_dev) from the
device's CU count and asserts it, so that a change of the heuristic cannot quietly move the case to the other kernel.
"""
import numpy as np
import pytest

from oracle import distance_ref as dr
from oracle import steps_oracle as so

pytestmark = pytest.mark.gpu

TILE, KW = 128, 4                      # PAIR_TILE, PAIR_SLOTS of csrc/pair_tiles.h
I64_MAX = np.iinfo(np.int64).max
MARK = -7


@pytest.fixture(scope="module")
def d():
    from tests.gpu_util import get_device
    dev = get_device()
    dev.use_torch_stream()
    return dev


# ------------------------------------------------------------------------------------------------ distance: helpers
def _padded_words(s):
    return ((s + 31) // 32 + KW - 1) // KW * KW


def _plan(n, s, rank=0, nranks=1):
    """What snpgpu_distance_packed_dev launches for this shape, restated."""
    import torch
    cu = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    nt = (n + TILE - 1) // TILE
    total = nt * (nt + 1) // 2
    mine = (total - rank + nranks - 1) // nranks if total > rank else 0
    words = _padded_words(s)
    p = {"cu": cu, "tiles": total, "mine": mine, "words": words, "slabs": words // KW}
    if mine == 0:
        p["kind"] = "none"
    elif words == 0:
        p["kind"] = "zero"
    elif mine < cu and words >= 4 * KW:
        want = (2 * cu + mine - 1) // mine
        parts = min(want, words // (2 * KW))
        chunk = ((words + parts - 1) // parts + KW - 1) // KW * KW
        p.update(kind="split", want=want, parts=parts, k_chunk=chunk, k_parts=(words + chunk - 1) // chunk)
    else:
        p.update(kind="direct", grid=min(mine, cu * 64))
    return p


def _owner(n, nranks):
    """(n, n) array: the rank that owns entry (i, j) — tile t of the row-major upper triangle goes to rank t % nranks, with
    its mirror image."""
    nt = (n + TILE - 1) // TILE
    own = np.zeros((nt, nt), dtype=np.int32)
    t = 0
    for bi in range(nt):
        for bj in range(bi, nt):
            own[bi, bj] = own[bj, bi] = t % nranks
            t += 1
    return np.repeat(np.repeat(own, TILE, axis=0), TILE, axis=1)[:n, :n]


def _pack(d, sym_t, n_sites=None):
    """sym_t: (n, stride) uint8 cuda tensor.  Packed rows as an (n, row_bytes) uint8 tensor (prefilled, so that a word the
    kernel does not write shows)."""
    import torch
    n, stride = sym_t.shape
    s = stride if n_sites is None else n_sites
    pk = torch.full((n, d.packed_row_bytes(s)), 0xA5, dtype=torch.uint8, device="cuda")
    d.pack_matrix_dev(sym_t.data_ptr(), n, s, stride, pk.data_ptr())
    return pk


def _np_pack(sym):
    """The documented layout (include/snpgpu.h): per row and 32-site word four uint32 { valid, code bit 1, code bit 0,
    lower-case }, bit i = site 32 * word + i, A=0 C=1 G=2 T=3; rows padded with zero words to a multiple of 4 words."""
    n, s = sym.shape
    words = _padded_words(s)
    c = np.zeros((n, words * 32), dtype=np.uint8)
    c[:, :s] = sym
    lower = (c >= 97) & (c <= 122)
    u = np.where(lower, c - 32, c)
    valid = np.isin(u, np.frombuffer(b"ACGT", dtype=np.uint8))
    hi = valid & ((u == ord("G")) | (u == ord("T")))
    lo = valid & ((u == ord("C")) | (u == ord("T")))

    def bits(b):
        return (b.reshape(n, words, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype("<u4")

    out = np.stack([bits(valid), bits(hi), bits(lo), bits(lower)], axis=2)
    return np.ascontiguousarray(out).view(np.uint8).reshape(n, words * 16)


def _assert_same(got, want, what=""):
    import torch
    if bool(torch.equal(got, want)):
        return
    bad = (got != want).nonzero()
    i, j = int(bad[0, 0]), int(bad[0, 1])
    tiles = sorted({(int(a) // TILE, int(b) // TILE) for a, b in bad[:: max(1, len(bad) // 2000)].tolist()})[:12]
    raise AssertionError("%s: %d entries differ; first (%d, %d) tile (%d, %d): got %d, want %d; tiles %s" %
                         (what, len(bad), i, j, i // TILE, j // TILE, int(got[i, j]), int(want[i, j]), tiles))


def _device_ref(sym_t, **kw):
    """distance_ref's torch form on the device — after its rows 0..255 (and its last rows) on this very input equal the
    numpy form on the host."""
    import torch
    ref = dr.distance_torch(sym_t, **kw)
    n = sym_t.shape[0]
    for r0 in sorted({0, max(0, n - 200)}):
        blk = sym_t[r0:r0 + 256]
        assert np.array_equal(ref[r0:r0 + 256, r0:r0 + 256].cpu().numpy(), dr.distance_numpy(blk.cpu().numpy()))
    rows = torch.tensor([0, n // 2, n - 1], device=sym_t.device)
    assert np.array_equal(ref[rows][:, rows].cpu().numpy(), dr.row_loop(sym_t[rows].cpu().numpy()))
    return ref


def _random_sym(rng, n, s, alphabet=b"ACGTacgt-N", probs=(.2, .2, .2, .2, .03, .03, .03, .03, .05, .03)):
    a = np.frombuffer(alphabet, dtype=np.uint8)
    return a[rng.choice(len(a), size=(n, s), p=np.array(probs) / sum(probs))]


# ------------------------------------------------------------------------------------------------ distance: cases
def test_direct_kernel_many_slabs(d):
    """k_distance<false> over 157 slabs (the double-buffered loop, an odd number of slabs): 2 817 rows = 23 x 23 tiles (276
    of them >= the CU count), the last tile row one row deep."""
    import torch
    n, s = 2817, 20_000
    p = _plan(n, s)
    assert p["kind"] == "direct" and p["mine"] == 276 >= p["cu"] and p["slabs"] == 157 and p["grid"] == p["mine"], p
    sym = torch.from_numpy(_random_sym(np.random.default_rng(21), n, s)).cuda()
    out = torch.full((n, n), MARK, dtype=torch.int32, device="cuda")
    d.distance_packed_dev(_pack(d, sym).data_ptr(), n, s, out.data_ptr())
    torch.cuda.synchronize()
    _assert_same(out, _device_ref(sym), "2817 x 20000")


def test_direct_kernel_three_ranks(d):
    """780 tiles over three ranks, 260 each: every rank still takes k_distance<false>; a rank writes its tiles and nothing
    else, and the three together are the matrix."""
    import torch
    n, s = 4865, 4000
    for r in range(3):
        p = _plan(n, s, r, 3)
        assert p["kind"] == "direct" and p["mine"] == 260 >= p["cu"] and p["slabs"] == 32, p
    sym = torch.from_numpy(_random_sym(np.random.default_rng(22), n, s)).cuda()
    pk = _pack(d, sym)
    ref = _device_ref(sym)
    own = torch.from_numpy(_owner(n, 3)).cuda()
    one = torch.full((n, n), MARK, dtype=torch.int32, device="cuda")
    d.distance_packed_dev(pk.data_ptr(), n, s, one.data_ptr(), 1, 3)
    torch.cuda.synchronize()
    _assert_same(one, torch.where(own == 1, ref, torch.full_like(ref, MARK)), "rank 1 of 3 alone")
    acc = torch.zeros((n, n), dtype=torch.int32, device="cuda")
    for r in range(3):
        d.distance_packed_dev(pk.data_ptr(), n, s, acc.data_ptr(), r, 3)
    torch.cuda.synchronize()
    _assert_same(acc, ref, "three ranks")


@pytest.mark.parametrize("s", [96, 600])
def test_grid_stride_loop(d, s):
    """23 100 rows = 181 tile rows = 16 471 tiles, more than the grid's cap of 64 workgroups per CU: 87 workgroups take a
    second tile.  One slab (s = 96) and five (s = 600).  The first 8 sites of row i spell i in base 4, so that a tile
    computed from the wrong rows, or not at all, cannot come out right.  2.1 GB of output and as much reference, both on
    the device: the reference costs five float32 matmuls of 23 100 x 23 100 x s (well under a second) plus numpy on two
    blocks of 256 rows; nothing but those blocks comes back to the host."""
    import torch
    n = 23_100
    p = _plan(n, s)
    assert p["kind"] == "direct" and p["tiles"] == 16_471 and p["mine"] > p["grid"] == p["cu"] * 64, p
    assert p["slabs"] == {96: 1, 600: 5}[s]
    g = torch.Generator(device="cuda")
    g.manual_seed(23 + s)
    lut = torch.tensor(list(b"ACGTacgt-N"), dtype=torch.uint8, device="cuda")
    probs = torch.tensor([.2, .2, .2, .2, .03, .03, .03, .03, .05, .03], device="cuda")
    sym = lut[torch.multinomial(probs, n * s, replacement=True, generator=g)].view(n, s).contiguous()
    idx = torch.arange(n, device="cuda")
    for k in range(8):
        sym[:, k] = lut[(idx >> (2 * k)) & 3]
    out = torch.full((n, n), MARK, dtype=torch.int32, device="cuda")
    d.distance_packed_dev(_pack(d, sym).data_ptr(), n, s, out.data_ptr())
    torch.cuda.synchronize()
    ref = _device_ref(sym, row_block=4096)
    _assert_same(out, ref, "23100 x %d" % s)
    del out, ref
    torch.cuda.empty_cache()


SPLIT_N = [1, 2, 127, 128, 129, 255, 256, 257, 384]
# words: 12 | 16 16 16 16 | 20 | 32 32 | 36 | 100 | 4100
SPLIT_S = [384, 385, 480, 481, 512, 513, 1023, 1024, 1025, 3200, 131_200]


def test_split_plans_are_what_the_cases_need():
    """The shapes below do reach the chunkings they are there for (restated dispatcher, this device's CU count)."""
    assert _plan(384, 384)["kind"] == "direct" and _plan(384, 384)["slabs"] == 3       # the longest row that is not split
    for s in SPLIT_S[1:]:
        for n in SPLIT_N:
            for nranks in (1, 2, 5):
                for r in range(nranks):
                    assert _plan(n, s, r, nranks)["kind"] in ("split", "none"), (n, s, r, nranks)
    p = _plan(128, 385)                                     # the smallest split: 16 words in two chunks of 8
    assert (p["words"], p["k_chunk"], p["k_parts"]) == (16, 8, 2) and p["want"] > p["parts"]
    p = _plan(128, 513)                                     # 20 words, parts capped by words / 8: chunks of 12 and 8
    assert (p["words"], p["parts"], p["k_chunk"], p["k_parts"]) == (20, 2, 12, 2) and p["want"] > p["parts"]
    p = _plan(1, 3200)                                      # 100 words: capped at 12 parts, chunk rounded up to 12 -> 9 parts, last 4
    assert (p["parts"], p["k_chunk"], p["k_parts"]) == (12, 12, 9) and p["words"] - 8 * 12 == 4
    p = _plan(384, 131_200)                                 # not capped; the chunk rounds up and the last part is shorter
    assert p["want"] == p["parts"] < p["words"] // 8 and p["k_chunk"] * (p["k_parts"] - 1) < p["words"] < p["k_chunk"] * p["k_parts"]
    assert p["words"] - p["k_chunk"] * (p["k_parts"] - 1) < p["k_chunk"] and p["words"] % p["k_chunk"] != 0


@pytest.mark.parametrize("s", SPLIT_S)
def test_split_k_edges(d, s):
    """k_distance<true> (and, at s = 384, the longest unsplit row) for 1 ... 384 rows, every rank of 1, 2, 5 and of more
    ranks than there are tiles: the tiles a rank owns (mirror images included) hold the distances, every other entry still
    holds what was there (a rank that owns nothing writes nothing), and a second call into the same buffer gives the same
    answer (the kernel adds into tiles that the zeroing kernel must have cleared: exactly those)."""
    import torch
    sym = _random_sym(np.random.default_rng(s), max(SPLIT_N), s)
    sym[:, -1] = np.frombuffer(b"ACGT", dtype=np.uint8)[np.arange(len(sym)) % 4]      # the last site counts
    ref_all = torch.from_numpy(dr.distance_numpy(sym)).cuda()
    if s <= 1025:
        assert np.array_equal(ref_all[:130, :130].cpu().numpy(), dr.row_loop(sym[:130]))
    sym_t = torch.from_numpy(sym).cuda()
    for n in SPLIT_N:
        pk = _pack(d, sym_t[:n])
        ref = ref_all[:n, :n].contiguous()
        tiles = _plan(n, s)["tiles"]
        for nranks in (1, 2, 5, tiles + 3):
            own = torch.from_numpy(_owner(n, nranks)).cuda()
            if nranks > tiles:                                # (tiles x tiles entries above are < tiles: ranks >= tiles own nothing)
                assert _plan(n, s, tiles, nranks)["kind"] == "none"
            for r in range(nranks):
                out = torch.full((n, n), MARK, dtype=torch.int32, device="cuda")
                d.distance_packed_dev(pk.data_ptr(), n, s, out.data_ptr(), r, nranks)
                first = out.clone()
                d.distance_packed_dev(pk.data_ptr(), n, s, out.data_ptr(), r, nranks)
                torch.cuda.synchronize()
                want = torch.where(own == r, ref, torch.full_like(ref, MARK)) if r < tiles else torch.full_like(ref, MARK)
                _assert_same(first, want, "n=%d s=%d rank %d of %d" % (n, s, r, nranks))
                _assert_same(out, want, "n=%d s=%d rank %d of %d, second call" % (n, s, r, nranks))


@pytest.mark.parametrize("s0", [65, 97, 129, 161, 993, 1025])
def test_padding_bits_and_row_stride_through_the_distance(d, s0):
    """The last valid site at every position of the last 32-site word and of the last 64-site wave group of a row, unsplit
    (s < 385) and split; the final site of every row is a base, and behind it — the rows lie in a wider buffer — come
    valid letters that would change every distance if the pack kernel read past n_sites."""
    import torch
    n = 6
    rng = np.random.default_rng(s0)
    for s in range(s0, s0 + 32):
        assert _plan(n, s)["kind"] == ("direct" if s < 385 else "split")
        stride = s + 37
        buf = _random_sym(rng, n, stride, b"ACGT", (1, 1, 1, 1))
        buf[:, s - 1] = np.frombuffer(b"ACGT", dtype=np.uint8)[(np.arange(n) + s) % 4]
        t = torch.from_numpy(buf).cuda()
        pk = _pack(d, t, n_sites=s)
        out = torch.full((n, n), MARK, dtype=torch.int32, device="cuda")
        d.distance_packed_dev(pk.data_ptr(), n, s, out.data_ptr())
        torch.cuda.synchronize()
        want = dr.row_loop(buf[:, :s])
        assert want[0, 1] != dr.row_loop(buf[:, :s - 1])[0, 1] and not np.array_equal(want, dr.row_loop(buf))
        assert np.array_equal(out.cpu().numpy(), want), s
        assert np.array_equal(pk.cpu().numpy(), _np_pack(buf[:, :s])), s


@pytest.mark.parametrize("s", [1, 33, 100, 480, 1000, 4097])
def test_pack_matrix_row_stride(d, s):
    """row_stride != n_sites (what hot_path.py passes): the packed rows equal, byte for byte, those packed from a contiguous
    copy and the numpy statement of the layout, padding words zero — with letters behind every row's end."""
    import torch
    n = 70
    rng = np.random.default_rng(s)
    for stride in (s + 1, s + 63, 2 * s):
        buf = _random_sym(rng, n, stride)
        buf[:, s:] = _random_sym(rng, n, stride - s, b"ACGTacgt", (1,) * 8)
        t = torch.from_numpy(buf).cuda()
        got = _pack(d, t, n_sites=s).cpu().numpy()
        tight = _pack(d, t[:, :s].contiguous()).cpu().numpy()
        want = _np_pack(buf[:, :s])
        assert np.array_equal(got, tight), stride
        assert np.array_equal(got, want), stride
        words = _padded_words(s)
        assert got.shape == (n, words * 16) and not got[:, ((s + 31) // 32) * 16:].any()


@pytest.mark.parametrize("s", [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1000])
def test_packed_layout_is_the_documented_one(d, s):
    """The packed rows travel between ranks (the C2 all-gather): the layout is an interface.  All 256 byte values."""
    import torch
    n = 9
    sym = np.random.default_rng(s).integers(0, 256, size=(n, s), dtype=np.uint8)
    sym[0, :] = (np.arange(s) * 37 + 11) % 256
    sym[1, :] = np.frombuffer(b"ACGTacgtNn-@`[{", dtype=np.uint8)[np.arange(s) % 15]
    got = _pack(d, torch.from_numpy(sym).cuda()).cpu().numpy()
    assert np.array_equal(got, _np_pack(sym))


@pytest.mark.parametrize("n,s,kind", [(130, 384, "direct"), (130, 2000, "split"), (2817, 300, "direct")])
def test_all_256_byte_values(d, n, s, kind):
    """Every byte value as a symbol: to_upper touches a-z only; '@', '`', '[', '{', 0x80-0xFF are not bases."""
    import torch
    assert _plan(n, s)["kind"] == kind
    rng = np.random.default_rng(n + s)
    sym = rng.integers(0, 256, size=(n, s), dtype=np.uint8)
    letters = np.frombuffer(b"ACGTacgt", dtype=np.uint8)
    sym = np.where(rng.random((n, s)) < 0.5, letters[rng.integers(0, 8, size=(n, s))], sym).astype(np.uint8)
    sym[:, :256] = np.arange(256, dtype=np.uint8)
    sym[1::2, :256] = np.roll(np.arange(256, dtype=np.uint8), 1)
    sym[2::3, :256] = np.arange(256, dtype=np.uint8) ^ 0x20
    want = dr.distance_numpy(sym)
    assert np.array_equal(want[:130, :130], dr.row_loop(sym[:130]))
    assert np.array_equal(d.distance(sym), want)
    t = torch.from_numpy(sym).cuda()
    out = torch.full((n, n), MARK, dtype=torch.int32, device="cuda")
    d.distance_packed_dev(_pack(d, t).data_ptr(), n, s, out.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ sort / scan: helpers
# The primitives have no entry point of their own.  Each element type is reached through the step that sorts it, with
# inputs whose output shows the whole sorted sequence:
#   uint64  dense_windows with the rule (max_snps 0, window 1): every position p is a window (p, p) — the sorted keys
#   Pair    merge_sites: unique keys + carriers = the sorted distinct (key, sample) pairs
#   Ival    merge_regions with intervals that do not touch: the sorted triples
SIZES = [1, 2, 7, 8, 9, 63, 64, 65, 2047, 2048, 2049, 4095, 4096, 4097, 6145, 8191, 8192, 8193,
         16_383, 16_385, 32_767, 32_769, 65_535, 65_537, 131_071, 131_073, 524_287, 524_288, 524_289 + 2048 + 3]
# (the uint32 scan's spine takes a second round above 8 388 608 elements: test_gpu_fullsize.py::test_merge_sites_at_configs4_scale
#  gets there with 5 * 10^7 records, and test_sixty_four_rules below with 131 100 positions x 64 rules)


def _dense_ref(pos, seg_off, ms, ws):
    """Windows in the order the step emits them: segment, position, rule.  Plain numpy per segment."""
    pos, seg_off = np.asarray(pos, dtype=np.int64), np.asarray(seg_off, dtype=np.int64)
    S, E, G = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.uint32)]
    for sg in np.nonzero(np.diff(seg_off))[0]:
        p = np.sort(pos[seg_off[sg]:seg_off[sg + 1]])
        flag = np.zeros((len(p), len(ms)), dtype=bool)
        end = np.zeros((len(p), len(ms)), dtype=np.int64)
        for r, (m, w) in enumerate(zip(ms, ws)):
            k = len(p) - m
            if k > 0:
                flag[:k, r] = p[:k] + (w - 1) >= p[m:]
                end[:k, r] = p[m:]
        i, r = np.nonzero(flag)
        S.append(p[i]); E.append(end[i, r]); G.append(np.full(len(i), sg, dtype=np.uint32))
    return np.concatenate(S), np.concatenate(E), np.concatenate(G)


def _dense_both(d, pos, seg_off, ms, ws):
    """Host form and _dev form; asserts they agree; returns (start, end, segment)."""
    import torch
    pos, seg_off = np.asarray(pos, dtype=np.int64), np.asarray(seg_off, dtype=np.uint32)
    cs, ce, cg = d.dense_windows(pos, seg_off, ms, ws)
    n_pos, cap = len(pos), max(1, len(pos) * len(ms))
    tp, tso = torch.from_numpy(pos).cuda(), torch.from_numpy(seg_off.astype(np.int32)).cuda()
    o_s, o_e = torch.full((cap,), -3, dtype=torch.int64, device="cuda"), torch.full((cap,), -3, dtype=torch.int64, device="cuda")
    o_g, o_n = torch.full((cap,), -3, dtype=torch.int32, device="cuda"), torch.full((2,), -3, dtype=torch.int32, device="cuda")
    d.dense_windows_dev(tp.data_ptr(), tso.data_ptr(), len(seg_off) - 1, n_pos, ms, ws, o_s.data_ptr(), o_e.data_ptr(), o_g.data_ptr(), o_n.data_ptr())
    torch.cuda.synchronize()
    k = int(o_n[0])
    assert int(o_n[1]) == 0 and k == len(cs)
    assert np.array_equal(o_s[:k].cpu().numpy(), cs) and np.array_equal(o_e[:k].cpu().numpy(), ce)
    assert np.array_equal(o_g[:k].cpu().numpy().astype(np.uint32), cg)
    assert bool((o_s[k:] == -3).all()) and bool((o_g[k:] == -3).all())          # nothing written past the count
    return cs, ce, cg


def _check_dense(d, pos, seg_off, ms, ws):
    got = _dense_both(d, pos, seg_off, ms, ws)
    want = _dense_ref(pos, seg_off, ms, ws)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    return got


def _sites_ref(keys, samp):
    keys, samp = np.asarray(keys, dtype=np.uint64), np.asarray(samp, dtype=np.uint32)
    order = np.lexsort((samp, keys))
    k, s = keys[order], samp[order]
    new_key = np.concatenate([[True], k[1:] != k[:-1]])
    new_pair = new_key | np.concatenate([[True], s[1:] != s[:-1]])
    pair_slot = np.cumsum(new_pair) - 1
    off = np.concatenate([pair_slot[new_key], [new_pair.sum()]]).astype(np.uint32)
    return k[new_key], off, s[new_pair]


def _sites_both(d, keys, samp):
    import torch
    keys, samp = np.asarray(keys, dtype=np.uint64), np.asarray(samp, dtype=np.uint32)
    uniq, off, car = d.merge_sites(keys, samp)
    m = len(keys)
    tk, ts = torch.from_numpy(keys.view(np.int64)).cuda(), torch.from_numpy(samp.view(np.int32)).cuda()
    ou = torch.full((m,), -3, dtype=torch.int64, device="cuda")
    oo = torch.full((m + 1,), -3, dtype=torch.int32, device="cuda")
    oc = torch.full((m,), -3, dtype=torch.int32, device="cuda")
    on = torch.full((4,), -3, dtype=torch.int32, device="cuda")
    d.merge_sites_dev(tk.data_ptr(), ts.data_ptr(), m, ou.data_ptr(), oo.data_ptr(), oc.data_ptr(), on.data_ptr())
    torch.cuda.synchronize()
    nu, nc = int(on[0]), int(on[1])
    assert (nu, nc) == (len(uniq), len(car))
    assert np.array_equal(ou[:nu].cpu().numpy().view(np.uint64), uniq)
    assert np.array_equal(oo[:nu + 1].cpu().numpy().view(np.uint32), off) and np.array_equal(oc[:nc].cpu().numpy().view(np.uint32), car)
    return uniq, off, car


def _check_sites(d, keys, samp):
    got = _sites_both(d, keys, samp)
    want = _sites_ref(keys, samp)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    if len(keys) <= 9000:                                   # the numpy statement itself against the oracle's sets and sorted()
        recs = {}
        for k, s in zip(np.asarray(keys).tolist(), np.asarray(samp).tolist()):
            recs.setdefault(s, []).append((k, 0))
        merged, _ = so.merge_sites([(i, i, recs[i]) for i in sorted(recs)])
        assert [k for (k, _), _ in merged] == want[0].tolist()
        assert [i for _, names in merged for i in names] == want[2].tolist()
    return got


def _regions_ref(grp, st, en):
    """utils.merge_regions per group with numpy: sort, running maximum of the ends per group, a new region where the start
    lies more than one past it."""
    grp, st, en = np.asarray(grp, dtype=np.uint32), np.asarray(st, dtype=np.int64), np.asarray(en, dtype=np.int64)
    order = np.lexsort((en, st, grp))
    g, s, e = grp[order], st[order], en[order]
    first = np.concatenate([[True], g[1:] != g[:-1]])
    run = np.empty_like(e)
    bounds = np.concatenate([np.nonzero(first)[0], [len(g)]])
    for a, b in zip(bounds[:-1], bounds[1:]):
        run[a:b] = np.maximum.accumulate(e[a:b])
    head = first.copy()
    head[1:] |= (s[1:] - 1) > run[:-1]                      # (start > max + 1 without the overflow at INT64_MAX; starts are >= 0)
    last = np.concatenate([head[1:], [True]])
    return g[head], s[head], run[last]


def _regions_both(d, grp, st, en):
    import torch
    grp, st, en = np.asarray(grp, dtype=np.uint32), np.asarray(st, dtype=np.int64), np.asarray(en, dtype=np.int64)
    mg, ms, me = d.merge_regions(grp, st, en)
    n = len(grp)
    tg, ts, te = torch.from_numpy(grp.view(np.int32)).cuda(), torch.from_numpy(st).cuda(), torch.from_numpy(en).cuda()
    og = torch.full((n,), -3, dtype=torch.int32, device="cuda")
    os_, oe = torch.full((n,), -3, dtype=torch.int64, device="cuda"), torch.full((n,), -3, dtype=torch.int64, device="cuda")
    on = torch.full((2,), -3, dtype=torch.int32, device="cuda")
    d.merge_regions_dev(tg.data_ptr(), ts.data_ptr(), te.data_ptr(), n, og.data_ptr(), os_.data_ptr(), oe.data_ptr(), on.data_ptr())
    torch.cuda.synchronize()
    k = int(on[0])
    assert int(on[1]) == 0 and k == len(mg)
    assert np.array_equal(og[:k].cpu().numpy().view(np.uint32), mg) and np.array_equal(os_[:k].cpu().numpy(), ms) and np.array_equal(oe[:k].cpu().numpy(), me)
    assert bool((os_[k:] == -3).all()) and bool((oe[k:] == -3).all())
    return mg, ms, me


def _oracle_regions(grp, st, en):
    want = []
    for g in sorted(set(np.asarray(grp).tolist())):
        sel = np.asarray(grp) == g
        for a, b in so.merge_regions(sorted(zip(np.asarray(st)[sel].tolist(), np.asarray(en)[sel].tolist()))):
            want.append((g, a, b))
    return want


def _check_regions(d, grp, st, en, oracle=None):
    got = _regions_both(d, grp, st, en)
    want = _regions_ref(grp, st, en)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    if oracle if oracle is not None else len(grp) <= 70_000:
        want = _oracle_regions(grp, st, en)                 # (compared as arrays: a failure must not print 10^5 tuples)
        assert len(want) == len(got[0])
        for k in range(3):
            assert np.array_equal(got[k], np.array([w[k] for w in want], dtype=got[k].dtype))
    return got


def _as_positions(v):
    """Order pattern v (non-negative ints) as one segment of positions; rules: every position, and equal neighbours."""
    return np.asarray(v, dtype=np.int64) * 3 + 1, [0, len(v)], [0, 1], [1, 1]


def _as_pairs(v):
    v = np.asarray(v, dtype=np.uint64)
    return (v >> np.uint64(1)) * np.uint64(0x0000_4000_0001_0003), (v & np.uint64(1)).astype(np.uint32) * np.uint32(0xFFFF_FFFF)


def _as_intervals(v, n_groups=3):
    v = np.asarray(v, dtype=np.int64)
    per = int(v.max()) // n_groups + 1
    return (v // per).astype(np.uint32) + 5, (v % per) * 4, (v % per) * 4 + (v & 1)       # ends start + 0 / + 1: no two touch


def _check_all_types(d, v):
    _check_dense(d, *_as_positions(v))
    _check_sites(d, *_as_pairs(v))
    g, s, e = _as_intervals(v)
    got = _check_regions(d, g, s, e)
    if len(set(np.asarray(v).tolist())) == len(v):
        assert len(got[0]) == len(v)                        # distinct values: nothing merges, the output is the sorted input


# ------------------------------------------------------------------------------------------------ sort / scan: cases
@pytest.mark.parametrize("n", SIZES)
def test_size_sweep(d, n):
    """Every size around the sort tile (2 048), the doubling merge passes, the scans' workgroups (2 048 and 8 192 elements)
    and the generic scan's spine (256 workgroups = 524 288 elements), shuffled, for the three element types."""
    rng = np.random.default_rng(n)
    # uint64: two segments of unsorted positions up to 2^40 - 1
    pos = rng.integers(0, 1 << 40, size=n)
    _check_dense(d, pos, [0, n // 3, n], [0, 1, 2], [1, 1 << 30, (1 << 31) - 1])
    # Pair: 64-bit keys (bit 63 set in half of them), a few thousand distinct ones, full-range samples
    pool = rng.integers(0, 1 << 64, size=max(1, n // 3), dtype=np.uint64)
    _check_sites(d, pool[rng.integers(0, len(pool), size=n)], rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32) | np.uint32(1 << 31))
    # Ival: intervals that do not touch (the output is the sorted input) ...
    _check_all_types(d, rng.permutation(n))
    # ... and intervals that do: five groups, some ends at the sentinel
    grp = rng.integers(0, 5, size=n) * 1000 + 2
    st = rng.integers(0, 30 * n + 10, size=n)
    en = st + rng.integers(0, 25, size=n)
    en[rng.integers(0, n, size=max(1, n // 5000))] = I64_MAX
    _check_regions(d, grp, st, en)


def _patterns(n):
    rng = np.random.default_rng(n)
    asc = np.arange(n)
    yield "sorted", asc
    for i in sorted({b * 1024 - 1 for b in (1, 2, 3, 5, 8, 13, 63, 64, 65) if b * 1024 < n} | {n - 2}):
        v = asc.copy()
        v[i], v[i + 1] = v[i + 1], v[i]                     # the one inversion: between two workgroups of the sortedness check
        yield "inversion at %d" % i, v
    yield "reversed", asc[::-1].copy()
    for period in (2047, 2049):
        yield "saw-tooth %d" % period, np.argsort(np.argsort((asc % period) * (n // period + 1) + asc // period))   # rising teeth
    yield "organ pipe", np.concatenate([asc[::2], asc[1::2][::-1]])
    yield "two interleaved runs", np.concatenate([asc[n // 2:], asc[:n // 2]])
    yield "shuffled", rng.permutation(n)


@pytest.mark.parametrize("n", [2049, 8193, 67_000])
def test_order_patterns(d, n):
    """Sorted input (the copy path), sorted but for one inversion that sits exactly between two workgroups of the check (a
    missed inversion would send unsorted data down the copy path), reversed, saw-tooth around the tile size, organ pipe."""
    for name, v in _patterns(n):
        assert sorted(v.tolist()) == list(range(n)), name
        try:
            _check_all_types(d, v)
        except AssertionError as e:
            raise AssertionError("%s, n = %d: %s" % (name, n, e))


@pytest.mark.parametrize("n", [4097, 20_000, 70_001])
def test_ties(d, n):
    """Long runs of equal elements across tile ends, merge-pass pair boundaries and 2 048-element output diagonals: keys drawn
    from 1, 2 and 3 values, and one value repeated 5 000 times among distinct neighbours.  Exact equality of the output fails
    if an element is lost or written twice."""
    rng = np.random.default_rng(n)
    cases = [("%d values" % k, rng.integers(0, k, size=n) * 7) for k in (1, 2, 3)]
    rep = min(5000, n // 2)
    for at in (0, 2048 - rep // 2, n // 2 - rep // 3, n - rep):          # where the run of equal values ends up once sorted
        at = max(0, min(n - rep, at))
        vals = np.concatenate([np.arange(at), np.full(rep, at), np.arange(at + 1, n - rep + 1)])
        cases.append(("run of %d at %d, shuffled" % (rep, at), rng.permutation(vals)))
        halves = np.concatenate([vals[1::2], vals[0::2]])   # two sorted runs, the repeated value in both
        cases.append(("run of %d at %d, two sorted halves" % (rep, at), halves))
    for name, v in cases:
        try:
            # uint64: every position a window, and (rule 1, window 1) a window per pair of equal neighbours
            _check_dense(d, *_as_positions(v))
            # Pair: equal key AND sample (the reference's per-sample set keeps one), and equal keys with three samples
            keys, _ = _as_pairs(v * 2)
            _check_sites(d, keys, np.zeros(n, dtype=np.uint32))
            _check_sites(d, keys, (rng.integers(0, 3, size=n) * 1_000_000_007 % (1 << 32)).astype(np.uint32))
            # Ival: identical triples (they merge into one), neighbours that touch nothing
            _check_regions(d, np.full(n, 9), np.asarray(v) * 4, np.asarray(v) * 4 + 1)
        except AssertionError as e:
            raise AssertionError("%s, n = %d: %s" % (name, n, e))


@pytest.mark.parametrize("n", [3 * 2048 + 40 + r for r in range(1, 8)] + [524_288 + 2048 + 8 + 5])
def test_merge_regions_group_ends_and_carries(d, n):
    """The segmented running maximum of k_prim_gscan: groups that change exactly at a workgroup's end (2 048 b), at a thread's
    end (8 t) and one element later; the maximum set by a group's FIRST interval and not exceeded by the thousands that follow
    (the carry crosses threads, workgroups and — in the largest case — the 256-workgroup round of the spine), and must not
    cross into the next group, whose intervals lie below it; n mod 8 = 1 ... 7 (a partly filled thread and workgroup)."""
    cuts = sorted({c for c in (8, 9, 16, 17, 24, 2040, 2048, 2049, 2056, 4096, 4097, 4104, 6144, 6145, 6152, 6153, 6180,
                               300_000, 524_288, 524_289, 525_000, 526_336, 526_337) if c < n})
    group_of = np.searchsorted(cuts, np.arange(n), side="right").astype(np.uint32) * 3 + 1      # groups 1, 4, 7, ...: none is 0
    first = np.concatenate([[True], group_of[1:] != group_of[:-1]])
    st = np.arange(n, dtype=np.int64) * 10
    for shuffle in (False, True):
        order = np.random.default_rng(n).permutation(n) if shuffle else np.arange(n)
        # (a) nothing touches: every interval is a region, whatever group it is in
        got = _check_regions(d, group_of[order], st[order], (st + 3)[order])
        assert len(got[0]) == n
        # (b) the first interval of every group reaches past everything: one region per group, ending where the first ends —
        #     and the next group's first interval (a smaller end for every second group) starts a new one
        en = st + 3
        en[first] = 10 * n + 1000 - group_of[first] % 2 * 500
        got = _check_regions(d, group_of[order], st[order], en[order])
        assert got[0].tolist() == sorted(set(group_of.tolist())) and got[2].tolist() == en[first].tolist()
        # (c) the running maximum comes from the first interval for 3 000 intervals, then regions of their own again
        en = st + 3
        en[first] = st[first] + 30_000
        _check_regions(d, group_of[order], st[order], en[order])


def test_value_extremes(d):
    """The ends of the documented ranges: positions up to 2^40 - 1 (the key is segment << 40 | position), segment index
    2^24 - 2, site keys with bit 63 set (unsigned order), interval ends at INT64_MAX - 1 next to the INT64_MAX sentinel."""
    top = (1 << 40) - 1
    pos = np.array([top, 0, top - 1, top, 5, top - 14, 1 << 39, (1 << 39) - 1, 0, top - 15], dtype=np.int64)
    for ms, ws in ([0, 1, 2], [1, 15, 16]), ([1, 1, 3], [1 << 30, (1 << 31) - 1, 2]):
        _check_dense(d, pos, [0, 4, 4, 10], ms, ws)
    with pytest.raises(Exception):
        d.dense_windows(np.array([top + 1], dtype=np.int64), np.array([0, 1], dtype=np.uint32), [0], [1])
    n_segs = (1 << 24) - 1                                  # the most the key has room for
    seg_off = np.zeros(n_segs + 1, dtype=np.uint32)
    rng = np.random.default_rng(31)
    sizes = {0: 5, 12_345: 3000, 8_388_607: 1, 8_388_608: 2100, n_segs - 2: 7, n_segs - 1: 2500}
    counts = np.zeros(n_segs, dtype=np.int64)
    for k, v in sizes.items():
        counts[k] = v
    seg_off[1:] = np.cumsum(counts)
    pos = rng.integers(0, 1 << 40, size=int(seg_off[-1]))
    pos[-2500:] = rng.integers(top - 4000, top + 1, size=2500)
    got = _check_dense(d, pos, seg_off, [0, 2], [1, 40])
    assert int(got[2].max()) == n_segs - 1
    with pytest.raises(Exception):
        d.dense_windows(np.zeros(1, dtype=np.int64), np.concatenate([seg_off, [seg_off[-1]]]).astype(np.uint32), [0], [1])
    # site keys: unsigned order across bit 63
    keys = np.array([1 << 63, (1 << 63) - 1, (1 << 64) - 1, 0, 1 << 63, (1 << 64) - 1, 1, (1 << 63) + 1, 0], dtype=np.uint64)
    samp = np.array([0xFFFFFFFF, 0, 3, 0x80000000, 0, 3, 0x7FFFFFFF, 2, 0x80000000], dtype=np.uint32)
    got = _check_sites(d, keys, samp)
    assert got[0].tolist() == [0, 1, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, (1 << 64) - 1]
    # interval ends at and next to the sentinel: le + 1 must not wrap, INT64_MAX swallows everything after it
    M = int(I64_MAX)
    cases = [[(0, M - 1), (M - 1, M - 1)], [(0, M - 1), (M, M)], [(0, M - 2), (M, M)], [(0, M), (5, 7), (M - 1, M - 1), (M, M)],
             [(3, M - 1), (4, M), (M - 1, M)], [(0, 5), (7, M - 1), (M - 1, M)], [(M - 1, M - 1), (M, M)], [(M, M), (0, 0), (2, 2)],
             [(0, M - 1), (1, 2), (M - 3, M - 2)]]
    for c in cases:
        for g in (0, 0xFFFFFFFF):
            got = _check_regions(d, [g] * len(c), [a for a, _ in c], [b for _, b in c], oracle=True)
            assert list(zip(got[1].tolist(), got[2].tolist())) == so.merge_regions(c)
    grp = np.concatenate([np.full(len(c), k, dtype=np.uint32) for k, c in enumerate(cases)])
    flat = [iv for c in cases for iv in c]
    _check_regions(d, grp[::-1].copy(), [a for a, _ in flat][::-1], [b for _, b in flat][::-1], oracle=True)


@pytest.mark.parametrize("m,w", [(0, 0), (0, 1), (0, 2), (0, 15), (1, 0), (1, 1), (1, 2), (2, 1), (11, 1000), (12, 1000), (13, 1000), (12, 1 << 30)])
def test_rule_extremes(d, steps_vectors, m, w):
    """max_snps = 0 (every position is a window once the window is >= 1), windows of 0 and 1, max_snps at and past the
    segment's length: dense windows + merge against oracle.find_dense_regions, whose answers for these very rules are pinned
    to the reference by tests/golden/steps_vectors.json.gz."""
    pinned = [v for v in steps_vectors["find_dense_regions"] if (v["m"], v["w"]) == (m, w)]
    assert len(pinned) >= 3
    rng = np.random.default_rng(m * 100 + w % 97)
    lists = [v["snps"] for v in pinned] + [sorted(rng.integers(1, 400, size=k).tolist()) for k in (12, 13, 14, 2049)]
    for snps in lists:
        want = so.find_dense_regions(m, w, snps)
        for v in pinned:
            if v["snps"] == snps:
                assert [list(t) for t in want] == v["out"]
        if not snps:
            continue
        cs, ce, cg = _check_dense(d, np.array(snps)[rng.permutation(len(snps))], [0, len(snps)], [m], [w])
        assert list(zip(cs.tolist(), ce.tolist())) == so.dense_windows(m, w, snps)
        if len(cs):
            _, ms_, me_ = _regions_both(d, cg, cs, ce)
            assert list(zip(ms_.tolist(), me_.tolist())) == want
        else:
            assert want == []


def test_sixty_four_rules(d):
    """MAX_RULES rules at once, over enough positions (131 100 x 64 = 8 390 400 flags) for the uint32 scan's spine to take a
    second round of 1 024 workgroups; a 65th rule is refused."""
    rng = np.random.default_rng(64)
    ms = [r % 7 for r in range(64)]
    ws = [0, 1, 2] + [int(x) for x in rng.integers(1, 3000, size=61)]
    n = 131_100
    assert n * 64 > 1024 * 8192
    pos = rng.integers(1, 40_000_000, size=n)
    cs, ce, cg = d.dense_windows(pos, np.array([0, 50_000, 50_000, n], dtype=np.uint32), ms, ws)
    want = _dense_ref(pos, [0, 50_000, 50_000, n], ms, ws)
    assert len(cs) > 100_000
    assert np.array_equal(cs, want[0]) and np.array_equal(ce, want[1]) and np.array_equal(cg, want[2])
    _check_dense(d, pos[:3000], [0, 1000, 3000], ms, ws)
    with pytest.raises(Exception):
        d.dense_windows(pos[:10], np.array([0, 10], dtype=np.uint32), ms + [1], ws + [1])
