"""The bit planes of the 128-byte call window (csrc/consensus.hip, k_call_lanes<128>: planes_of_32_bytes, Planes::space / term, the
quality comparator, the funnel shift that cuts the bases field's planes out of the window's), stated in numpy and checked
exhaustively: every byte value at every byte of the window, every threshold, every shift.  No GPU: this pins the functions
themselves; tests/test_gpu_call_window_planes.py runs the kernels against the oracle."""
import numpy as np

WIN = 128
U32 = np.uint32


def perm(s0, s1, sel):
    """v_perm_b32: byte j of the result is byte sel[j] of the eight bytes {s0 : s1} (s1 holds bytes 0-3, s0 bytes 4-7)."""
    both = (s0.astype(np.uint64) << np.uint64(32)) | s1.astype(np.uint64)
    out = np.zeros_like(s1)
    for j in range(4):
        k = (sel >> (8 * j)) & 0xFF
        assert k < 8
        out |= ((both >> np.uint64(8 * k)) & np.uint64(0xFF)).astype(U32) << U32(8 * j)
    return out


def exchange(a, b, s, m):
    m = U32(m)
    return (a & m) | ((b << U32(s)) & ~m), ((a >> U32(s)) & m) | (b & ~m)


def planes_of_32_bytes(d):
    """d: eight arrays of dwords (little endian, bytes 4 j .. 4 j + 3) -> eight plane words, as the kernel's function of this name:
    a 4 x 4 byte transpose of the dwords 8 bytes apart, then three exchanges of a bit-position bit against the register index."""
    r = [[None, None] for _ in range(4)]
    for h in range(2):
        u0, u1 = perm(d[2 + h], d[h], 0x05010400), perm(d[2 + h], d[h], 0x07030602)
        u2, u3 = perm(d[6 + h], d[4 + h], 0x05010400), perm(d[6 + h], d[4 + h], 0x07030602)
        r[0][h], r[1][h] = perm(u2, u0, 0x05040100), perm(u2, u0, 0x07060302)
        r[2][h], r[3][h] = perm(u3, u1, 0x05040100), perm(u3, u1, 0x07060302)
    for h in range(2):
        r[0][h], r[1][h] = exchange(r[0][h], r[1][h], 1, 0x55555555)
        r[2][h], r[3][h] = exchange(r[2][h], r[3][h], 1, 0x55555555)
    for h in range(2):
        r[0][h], r[2][h] = exchange(r[0][h], r[2][h], 2, 0x33333333)
        r[1][h], r[3][h] = exchange(r[1][h], r[3][h], 2, 0x33333333)
    for k in range(4):
        r[k][0], r[k][1] = exchange(r[k][0], r[k][1], 4, 0x0F0F0F0F)
    return [r[b & 3][b >> 2] for b in range(8)]


def window_planes(windows):
    """windows: [n, 128] bytes -> pw[b][q]: [n] plane words (bit b of the bytes 32 q .. 32 q + 31)."""
    dw = np.ascontiguousarray(windows, dtype=np.uint8).view("<u4")         # [n, 32]
    pw = [[None] * (WIN // 32) for _ in range(8)]
    for q in range(WIN // 32):
        p = planes_of_32_bytes([dw[:, 8 * q + j] for j in range(8)])
        for b in range(8):
            pw[b][q] = p[b]
    return pw


def plain_planes(windows):
    """The same by definition: bit i of pw[b][q] is bit b of byte 32 q + i."""
    w = windows.astype(U32)
    return [[sum(((w[:, 32 * q + i] >> U32(b)) & U32(1)) << U32(i) for i in range(32)) for q in range(WIN // 32)] for b in range(8)]


def space(p):
    """Planes::space(): str.split()'s separators 9..13 and 28..32."""
    p0, p1, p2, p3, p4, p5, p6 = p
    lo = ~p6 & ~p5
    return (lo & ~p4 & p3 & (p2 | p1 | p0) & ~(p2 & p1)) | (lo & p4 & p3 & p2) | (~p6 & p5 & ~(p4 | p3 | p2 | p1 | p0))


def term(p):
    """Planes::term(): the line terminator candidates 10..13."""
    p0, p1, p2, p3, p4, p5, p6 = p
    return ~p6 & ~p5 & ~p4 & p3 & (p2 ^ p1)


def at_least(p8, thr):
    """The comparator: byte >= thr from the eight planes, least significant bit first (v_bitop3 0xD4 per plane)."""
    ge = np.full_like(p8[0], 0xFFFFFFFF)
    for b in range(8):
        tb = U32(0xFFFFFFFF if (thr >> b) & 1 else 0)
        ge = (p8[b] & ge) | (~tb & (p8[b] | ge))
    return ge


def field_planes(pw_b, bs):
    """One plane of the bases field: the window's four words from byte bs on, 64 bits (two v_alignbit after the choice of dwords)."""
    k1, k2 = bool(bs & 32), bool(bs & 64)
    zero = np.zeros_like(pw_b[0])
    y0, y1, y2, y3 = (pw_b[2], pw_b[3], zero, zero) if k2 else pw_b
    z0, z1, z2 = (y1, y2, y3) if k1 else (y0, y1, y2)
    s = np.uint64(bs & 31)

    def alignbit(hi, lo):
        return ((((hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)) >> s) & np.uint64(0xFFFFFFFF)).astype(U32)
    return alignbit(z1, z0), alignbit(z2, z1)


def bits_of(words):
    """[n] x len(words) dwords -> [n, 32 * len(words)] bits."""
    return np.stack([(w >> U32(i)) & U32(1) for w in words for i in range(32)], axis=1).astype(np.uint8)


def test_every_byte_value_at_every_byte_of_the_window():
    value, at = np.meshgrid(np.arange(128), np.arange(WIN), indexing="ij")
    value, at = value.ravel(), at.ravel()
    for background in (0x00, 0x7F, 0x55):
        windows = np.full((len(value), WIN), background, dtype=np.uint8)
        windows[np.arange(len(value)), at] = value
        pw = window_planes(windows)
        for b in range(8):
            got = bits_of(pw[b])
            assert np.array_equal(got, (windows >> b) & 1), (background, b)


def test_random_windows_of_all_256_byte_values_match_the_definition():
    rng = np.random.default_rng(5)
    windows = rng.integers(0, 256, size=(2000, WIN)).astype(np.uint8)
    pw, want = window_planes(windows), plain_planes(windows)
    for b in range(8):
        for q in range(WIN // 32):
            assert np.array_equal(pw[b][q], want[b][q].astype(U32)), (b, q)


def _planes_of_all_bytes():
    v = np.arange(256, dtype=U32)
    return v, [np.where((v >> b) & 1, 0xFFFFFFFF, 0).astype(U32) for b in range(8)]


def test_space_and_term_are_the_sets_of_str_split_and_of_the_terminators():
    v, p = _planes_of_all_bytes()
    sp, tm = space(p[:7]) & ~p[7], term(p[:7]) & ~p[7]                       # (the kernel: a byte >= 0x80 is no separator)
    for c in range(256):
        assert int(sp[c]) in (0, 0xFFFFFFFF) and int(tm[c]) in (0, 0xFFFFFFFF)
        assert bool(sp[c]) == (c in (9, 10, 11, 12, 13, 28, 29, 30, 31, 32)), c
        assert bool(tm[c]) == (c in (10, 11, 12, 13)), c
    assert {c for c in range(128) if bool(sp[c])} == {c for c in range(128) if chr(c).isspace()}         # str.split()'s own set


def test_comparator_for_every_threshold():
    v, p = _planes_of_all_bytes()
    for thr in range(1, 129):
        ge = at_least(p, thr)
        assert np.array_equal(ge != 0, v >= thr), thr
        assert set(np.unique(ge).tolist()) <= {0, 0xFFFFFFFF}


def test_funnel_shift_for_every_field_start():
    rng = np.random.default_rng(9)
    windows = rng.integers(0, 128, size=(64, WIN)).astype(np.uint8)
    pw = window_planes(windows)
    for bs in range(WIN):
        for b in range(7):
            lo, hi = field_planes(pw[b], bs)
            got = bits_of([lo, hi])
            want = np.zeros((len(windows), 64), dtype=np.uint8)
            n = min(64, WIN - bs)
            want[:, :n] = (windows[:, bs:bs + n] >> b) & 1                 # past the window: zero
            assert np.array_equal(got, want), (bs, b)


def _bytewise_masks(window, o, has=True):
    """The separator and terminator masks by the byte-wise rules the wider windows' tokeniser states (and the 128-byte one stated
    until round 25): bytes before the line start read as blanks; a 64-byte half after one that holds a terminator candidate is all
    separators and holds no candidate; a site without a line: all separators."""
    W, T, done = [0, 0], [0, 0], not has
    for blk in range(2):
        if done:
            W[blk], T[blk] = (1 << 64) - 1, 0
            continue
        for i in range(64):
            c = 0x20 if 64 * blk + i < o else int(window[64 * blk + i])
            if c in (9, 10, 11, 12, 13, 28, 29, 30, 31, 32):
                W[blk] |= 1 << i
            if c in (10, 11, 12, 13):
                T[blk] |= 1 << i
        done = T[blk] != 0
    return W, T


def test_edge_rules_as_masks_give_the_bytewise_tokeniser_masks():
    rng = np.random.default_rng(13)
    pool = np.frombuffer(b"\t\t \n\r\x0b\x0c\x1c\x1d\x1e\x1f" + b"ACGTacgt.,0123456789^$+-*IIIIII" * 3, dtype=np.uint8)
    windows = rng.choice(pool, size=(400, WIN))
    windows[:100, :64] = rng.choice(pool[11:], size=(100, 64))             # no terminator in the first half
    pw = window_planes(windows)
    sp = [space([pw[b][q] for b in range(7)]) & ~pw[7][q] for q in range(4)]
    tm = [term([pw[b][q] for b in range(7)]) & ~pw[7][q] for q in range(4)]
    for n in range(len(windows)):
        for o in (0, 1, 7, 15) if n % 4 else range(16):
            for has in (True, False):
                before = (1 << o) - 1
                s = [int(sp[0][n]) | before] + [int(sp[q][n]) for q in (1, 2, 3)]
                t = [int(tm[0][n]) & ~before] + [int(tm[q][n]) for q in (1, 2, 3)]
                W, T, done = [0, 0], [0, 0], not has
                for blk in range(2):
                    W[blk] = (1 << 64) - 1 if done else s[2 * blk] | (s[2 * blk + 1] << 32)
                    T[blk] = 0 if done else t[2 * blk] | (t[2 * blk + 1] << 32)
                    done = done or T[blk] != 0
                assert (W, T) == _bytewise_masks(windows[n], o, has), (n, o, has)


def test_quality_range_mask():
    """allq: no byte below thr among the `need` qualities from byte qs on — the comparator's words under below(qs + need) & ~below(qs)."""
    rng = np.random.default_rng(17)
    windows = rng.integers(33, 80, size=(200, WIN)).astype(np.uint8)
    pw = window_planes(windows)
    for thr in (33, 34, 48, 73, 79, 80, 128):
        ge = [at_least([pw[b][q] for b in range(8)], thr) for q in range(4)]
        for n in range(len(windows)):
            word = sum(int(ge[q][n]) << (32 * q) for q in range(4))
            for qs, need in ((0, 0), (0, 128), (5, 1), (63, 2), (64, 64), (31, 33), (100, 28), (128, 0), (int(rng.integers(0, 100)), int(rng.integers(0, 28)))):
                rmask = ((1 << (qs + need)) - 1) & ~((1 << qs) - 1)
                assert ((rmask & ~word) == 0) == bool((windows[n, qs:qs + need] >= thr).all()), (thr, n, qs, need)
