"""The boolean algebra of the one-lane-per-site call kernels' count path (csrc/consensus.hip, k_call_lanes), stated in numpy and
checked over every ASCII byte value: the seven bit planes of the bases field, the byte classes ('^', sign, '$', digit) and the
thirteen symbol classes derived from them, against the rule the kernel's byte -> class table (S.cls) is filled by and against plain
byte compares.  No GPU: this pins the functions themselves; tests/test_gpu_call_counts.py runs the kernels against the oracle."""
import numpy as np

ALL = np.arange(128, dtype=np.uint32)


def cls_rule(c):
    """S.cls[c]: rank of the symbol among "*ACGNT" (6: '.' / ','), | 8 on the reverse strand (>= 'a', pileup.py:269-270); 0xFF: other."""
    u = c - 32 if 97 <= c <= 122 else c
    k = "*ACGNT".find(chr(u)) if chr(u) in "*ACGNT" else 0xFF
    if k != 0xFF and c >= 0x61:
        k |= 8
    if c == ord("."):
        k = 6
    if c == ord(","):
        k = 14
    return k


def gather_planes(field):
    """pl[b]: one mask bit per byte of the field, as the kernel gathers them: two dwords a step, the plane's bit of every byte
    (w & 0x01010101 << b), two dot4 with 0x08040201 / 0x80402010 (eight plane bits << b), one shift into place."""
    n = len(field)
    padded = np.zeros((n + 7) // 8 * 8 + 8, dtype=np.uint8)
    padded[:n] = field
    words = (n + 31) // 32 or 1
    pl = np.zeros((7, words), dtype=np.uint64)
    for jp in range((n + 7) // 8):
        w0, w1 = padded[8 * jp:8 * jp + 4].astype(np.uint64), padded[8 * jp + 4:8 * jp + 8].astype(np.uint64)
        pos = (8 * jp) & 31
        for b in range(7):
            sel = np.uint64(1 << b)
            v = int(((w0 & sel) * np.array([1, 2, 4, 8], dtype=np.uint64)).sum() + ((w1 & sel) * np.array([16, 32, 64, 128], dtype=np.uint64)).sum())
            assert v < 1 << 32                                     # the dot4 accumulates in 32 bits
            placed = (v << (pos - b)) if pos >= b else (v >> (b - pos))
            assert placed < 1 << 32                                # nothing is shifted out of the mask word
            pl[b][jp >> 2] |= np.uint64(placed)
    return pl


def class_masks(p):
    """The expressions of the kernel's struct Planes (the one place it states them) on the planes p[0..6] (any unsigned integer
    arrays), name -> mask."""
    p0, p1, p2, p3, p4, p5, p6 = p
    pu = ~p6 & p5 & ~p4
    out = {
        "caret": p6 & ~p5 & p4 & p3 & p2 & p1 & ~p0,
        "sign": pu & p3 & p0 & (p2 ^ p1),
        "dollar": pu & ~p3 & p2 & ~p1 & ~p0,
        "digit": ~p6 & p5 & p4 & ~(p3 & (p2 | p1)),
    }
    lo3 = ~p4 & ~p3
    ac = lo3 & ~p2 & p0
    e = {"A": ac & ~p1, "C": ac & p1, "G": lo3 & p2 & p1 & p0, "N": ~p4 & p3 & p2 & p1 & ~p0, "T": p4 & ~p3 & p2 & ~p1 & ~p0}
    kp = ~p6 & p5 & ~p4 & p3 & ~p0
    out["*"], out["."], out[","] = kp & ~p2 & p1, kp & p2 & p1, kp & p2 & ~p1
    for s, m in e.items():
        out[s] = p6 & ~p5 & m
        out[s.lower()] = p6 & p5 & m
    return out


SYMBOLS = "*ACGNT"


def test_class_masks_match_the_table_rule_for_every_ascii_byte():
    planes = [np.where((ALL >> b) & 1, 0xFFFFFFFF, 0).astype(np.uint32) for b in range(7)]
    m = class_masks(planes)
    assert len([k for k in m if k not in ("caret", "sign", "dollar", "digit")]) == 13
    for c in range(128):
        hit = [k for k in m if m[k][c] and k not in ("caret", "sign", "dollar", "digit")]
        k = cls_rule(c)
        if k == 0xFF:
            assert hit == [], (c, hit)                             # "any other symbol": in none of the thirteen
            continue
        assert hit == [chr(c)], (c, hit)                           # exactly its own class
        want = "." if k == 6 else "," if k == 14 else (SYMBOLS[k & 7].lower() if k & 8 else SYMBOLS[k & 7])
        assert want == chr(c)
        # the byte lane the count lands in: lane k & 7 of cnt_r when k & 8, of cnt_f otherwise; '.' and ',' in lane 6
        lane, reverse = k & 7, bool(k & 8)
        assert (lane, reverse) == ((6, c == ord(",")) if chr(c) in ".," else (SYMBOLS.index(chr(c).upper()), c >= 0x61))
        assert all(int(v[c]) in (0, 0xFFFFFFFF) for v in m.values())
    for c in range(128):
        assert bool(m["caret"][c]) == (c == ord("^"))
        assert bool(m["sign"][c]) == (chr(c) in "+-")
        assert bool(m["dollar"][c]) == (c == ord("$"))
        assert bool(m["digit"][c]) == (48 <= c <= 57)


def test_planes_gather_every_bit_at_every_field_length():
    rng = np.random.default_rng(7)
    for n in (0, 1, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 254, 255):
        for field in (rng.integers(0, 128, size=n).astype(np.uint8), np.full(n, 0x7F, dtype=np.uint8)):
            pl = gather_planes(field)
            for b in range(7):
                for i in range(n):
                    assert (int(pl[b][i >> 5]) >> (i & 31)) & 1 == (int(field[i]) >> b) & 1, (n, b, i)
                for q in range(pl.shape[1]):                       # nothing past the field's last byte
                    assert int(pl[b][q]) >> max(0, min(32, n - 32 * q)) == 0


def test_counts_are_popcounts_under_the_kept_mask():
    """The fast path end to end on the CPU: planes of a random field, class masks, popcounts under a random kept mask K, against
    counting the kept bytes one by one by the table rule; a kept byte of no class is reported (the site is handed on)."""
    rng = np.random.default_rng(11)
    pool = np.frombuffer(b"*ACGNTacgnt.,.,.,AAAA^$+-09R<>#", dtype=np.uint8)
    for n in (1, 5, 32, 33, 64, 65, 128, 129, 255):
        field = rng.choice(pool, size=n)
        keep = rng.random(n) < 0.8
        pl = gather_planes(field)
        want_f, want_r, want_other = [0] * 7, [0] * 7, False
        for c, k in zip(field, keep):
            if k:
                cl = cls_rule(int(c))
                if cl == 0xFF:
                    want_other = True
                else:
                    (want_r if cl & 8 else want_f)[cl & 7] += 1
        got_f, got_r, other = [0] * 7, [0] * 7, 0
        for q in range(pl.shape[1]):
            kq = np.uint64(sum(1 << i for i in range(32) if 32 * q + i < n and keep[32 * q + i]))
            m = class_masks([pl[b][q] for b in range(7)])
            union = np.uint64(0)
            for name, lane, rev in [("*", 0, 0), (".", 6, 0), (",", 6, 1)] + [(s, i, 0) for i, s in enumerate(SYMBOLS) if i] + [(s.lower(), i, 1) for i, s in enumerate(SYMBOLS) if i]:
                (got_r if rev else got_f)[lane] += bin(int(m[name] & kq)).count("1")
                union |= m[name]
            other |= int(kq & ~union)
        assert (got_f, got_r, other != 0) == (want_f, want_r, want_other), n
