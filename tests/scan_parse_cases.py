"""Pileups for the one-window round of the scan's lane-per-line parse (csrc/scan.hip, k_scan_wave, the `fast_round` branch): the
24 bytes that end with the TAB after the position, one masked compare per dword against the layout of scan_layout(), a SWAR digit
test on the last four digits.  Which masks apply depends on the length L of the contig name and the digit count g of the position
column, so every builder here takes a cell (L, g), writes the position column zero-padded to exactly g bytes (int() takes
0000009999, and so do the reference and the kernel) and builds ONE file per case, of 4 to 15 scan tiles of short lines.

Plain Python / NumPy, no device and no library code (the pattern of tests/lines_cases.py, on which this builds).  Every builder
asserts its own geometry — the tile a changed line lies in, the byte a decoy differs in, the offset a seam line starts at — so
that a case cannot miss its edge silently; tests/test_scan_parse_cpu.py runs them all and pins `expectation` against the oracle.

`expectation` is what the reader with a position set (oracle.pileup_oracle.scan_sites, which is pileup.py:423-429) makes of a
file: the last line of every listed key, or the first line it ends at with an exception."""
import functools
import itertools
from collections import namedtuple

import numpy as np

from oracle import pileup_oracle as po
from tests import lines_cases as lc

TILE = 4096                                                     # SCAN_TILE: bytes a wave takes per step
MIN_TILES, MAX_TILES = 4, 15                                    # (a file of at most 15 tiles is one wave's run; under 4 it hardly leaves the first rounds)
TAB = b"\t"
DEPTHS = (0, 9, 10, 9999, 10000, 123, 99999, 7)                 # depth columns written over every seventh line's own
_ALPHABET = b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789"
_EXOTIC = (b"\x1c", b"\x1d", b"\x1e", b"\x1f")

Expect = namedtuple("Expect", "last hits n_lines depth_sum error")


# ---- the statement ------------------------------------------------------------------------------------------------------------------
def expectation(data, keys):
    """Expect(last, hits, n_lines, depth_sum, None): {key: 1 + offset of the last line at it, or 0}, the lines that are at some key,
    the lines, po.depth_sum — or Expect(None, None, None, None, (exception class, offset of the line)) where the reader ends:
    every line is split and its second field goes through int() (pileup.py:425-426), a line at a listed key becomes a Record
    (po.parse_record)."""
    wanted = set(keys)
    last = {k: 0 for k in keys}
    hits = 0
    starts = lc.line_starts(data)
    for s, ln in zip(starts, lc.lines_of(data, starts)):
        try:
            f = po.split_fields(ln) if any(c in ln for c in _EXOTIC) else ln.split()      # (as po.scan_sites chooses)
            chrom, pos = f[:2]
            key = (chrom, int(pos))
            if key in wanted:
                po.parse_record(f, 0)
                last[key] = int(s) + 1
                hits += 1
        except (ValueError, IndexError) as e:
            return Expect(None, None, None, None, (type(e), int(s)))
    return Expect(last, hits, len(starts), po.depth_sum(data), None)


# ---- lines and files ----------------------------------------------------------------------------------------------------------------
def cell_name(L):
    """The contig name of L bytes: every byte differs from its neighbours, names of different lengths differ."""
    name = (b"n%d_" % L + _ALPHABET)[:L]
    assert len(name) == L
    return name


def field(v, g):
    """The position column of value v in exactly g bytes."""
    f = b"%0*d" % (g, v)
    assert len(f) == g and int(f) == v, (v, g)
    return f


def make_line(name, posfield, i, seed=0, depth=None, sep1=TAB, sep2=TAB):
    """A short line (0 to 8 reads, lc.pileup_line's) without terminator whose first two columns are `name` and `posfield` as given;
    every seventh line carries a depth column of DEPTHS in place of its own (the reads stay: Record's zip takes the shorter)."""
    _, _, ref, d, bases, quals = lc.pileup_line(b"N", i, seed=seed).split(TAB)
    if depth is None and i % 7 == 3:
        depth = DEPTHS[(i // 7) % len(DEPTHS)]
    if depth is not None:
        d = b"%d" % depth
    return name + sep1 + posfield + sep2 + TAB.join((ref, d, bases, quals))


def exact_line(name, posfield, width):
    """A line of exactly `width` bytes without terminator: the length comes from the reads, an odd byte from a second depth digit."""
    rest = width - (len(name) + len(posfield) + 6)              # depth digits + two bytes a read
    assert rest >= 3, (width, rest)
    d, r = (b"7", (rest - 1) // 2) if rest % 2 else (b"12", (rest - 2) // 2)
    ln = name + TAB + posfield + TAB + b"A" + TAB + d + TAB + b".,"[:1] * r + TAB + b"I" * r
    assert len(ln) == width and r >= 1
    return ln


def join(lines, term=b"\n"):
    return b"".join(ln + term for ln in lines)


def offsets(lines, term=b"\n"):
    """The offset at which every line of `lines` starts in join(lines, term)."""
    return np.concatenate([[0], np.cumsum([len(ln) + len(term) for ln in lines])[:-1]]).astype(np.int64)


def n_tiles(data):
    return (len(data) + TILE - 1) // TILE


def check_size(data):
    assert MIN_TILES <= n_tiles(data) <= MAX_TILES, (len(data), n_tiles(data))
    return data


def stretch(name, g, values, seed=0, first=0):
    return [make_line(name, field(v, g), first + i, seed=seed) for i, v in enumerate(values)]


def grow(name, g, value_of, seed=0, tiles=MIN_TILES, extra=200, at_least=0):
    """Lines of value_of(i), i = 0, 1, ..., until the file has `tiles` - 1 whole tiles and `extra` bytes, and `at_least` lines."""
    lines, size, vals = [], 0, []
    for i in itertools.count():
        if size >= (tiles - 1) * TILE + extra and i >= at_least:
            break
        vals.append(value_of(i))
        lines.append(make_line(name, field(vals[-1], g), i, seed=seed))
        size += len(lines[-1]) + 1
    return lines, vals


def listed(name, values):
    """Every second position: the even ones."""
    return sorted({(name, v) for v in values if v % 2 == 0})


def first_line_from(offs, at):
    """Index of the first line that starts at or after byte `at`."""
    i = int(np.searchsorted(offs, at, side="left"))
    assert i < len(offs), (at, int(offs[-1]))
    return i


# ---- A: the lattice -----------------------------------------------------------------------------------------------------------------
LATTICE_L = range(1, 47)
LATTICE_G = range(1, 12)


def lattice_cycle(g):
    """The values a cell walks through, again and again: all that g < 4 digits allow; the last 300 and the first 200 of four digits;
    9 900 .. 10 100 — the top digits go from 0 to 1 at 10 000, where a one-window round fails and recalibrates — and then 40 .. 79
    (back to top digits 0) for five digits and more."""
    if g <= 3:
        return list(range(10 ** g))
    if g == 4:
        return list(range(9700, 10000)) + list(range(0, 200))
    return list(range(9900, 10101)) + list(range(40, 80))


def lattice_case(L, g, seed=1):
    """(data, keys) of cell (L, g)."""
    name, cyc = cell_name(L), lattice_cycle(g)
    lines, vals = grow(name, g, lambda i: cyc[i % len(cyc)], seed=seed * 100 + L, at_least=2 * len(cyc) + 10 if g >= 5 else 0)
    data = check_size(join(lines))
    fields = [ln.split(TAB)[1] for ln in lines]
    assert all(len(f) == g for f in fields) and all(ln.startswith(name + TAB) for ln in lines)
    if g >= 5:
        crossings = sum(1 for a, b in zip(vals, vals[1:]) if (a, b) == (9999, 10000))
        assert crossings >= 2 and {9998, 9999, 10000, 10001, 10002, 10003} <= set(vals)
    else:
        assert len(vals) > len(set(vals)) or g >= 3              # (one and two digits cycle: a position comes again, and the last line wins)
    return data, listed(name, vals)


# ---- B: near-miss names -------------------------------------------------------------------------------------------------------------
# L + g in {21, 22, 23, 37, 38, 39}.  Of the name lengths 1, 4, 5, 16, 17 and 44 only 16 and 17 reach one of those sums with 1 to 11
# digits (21 .. 23); the sums 37 .. 39 — where the two pieces of a long name meet — are taken with 5 and with 10 digits, and 21 .. 23
# with 10 digits as well.
DECOY_SUMS = (21, 22, 23, 37, 38, 39)
DECOY_CELLS = sorted({(L, s - L) for s in DECOY_SUMS for L in (1, 4, 5, 16, 17, 44) if 1 <= s - L <= 11} |
                     {(s - g, g) for s in DECOY_SUMS for g in (5, 10)})


def decoy_indices(L, g):
    ks = {0, 3, 4, 11, 12, 15, 16, L - (22 - g) - 1, L - (22 - g), L - 2, L - 1}
    return sorted(k for k in ks if 0 <= k < L)


def decoy_name(name, k):
    d = bytearray(name)
    d[k] ^= 1                                                    # (a letter, digit or '_' stays a byte above 0x20)
    d = bytes(d)
    assert len(d) == len(name) and [i for i in range(len(name)) if d[i] != name[i]] == [k] and d[k] > 0x20
    return d


def decoy_case(L, g, k, own_keys=False, seed=2):
    """(data, keys, decoys): the contig's lines at 1000, 1001, ... (one run of top digits), and in tiles 2, 4 and 6 one line each of a
    name that differs from the contig's in byte k alone, at a position that is listed for the contig and whose real line lies more
    than a tile earlier.  decoys: [(offset of the decoy line, the key it must NOT be at)].  own_keys: the decoy's name is in the set
    with those positions, and its lines are at them."""
    name = cell_name(L)
    decoy = decoy_name(name, k)
    lines, vals = grow(name, g, lambda i: 1000 + i, seed=seed * 100 + L, tiles=8, extra=600)
    assert max(vals) < 9000
    offs = offsets(lines)
    plan = []
    for t in (2, 4, 6):
        i = first_line_from(offs, t * TILE + 300)
        back = first_line_from(offs, (t - 1) * TILE - 600)      # the real line: more than a tile before
        v = vals[back] if vals[back] % 2 == 0 else vals[back + 1]
        plan.append((i, v))
    out, decoys = [], []
    at = 0
    for i, ln in enumerate(lines):
        for j, v in plan:
            if j == i:
                dl = make_line(decoy, field(v, g), 5000 + i, seed=seed)
                decoys.append((at, (name, v)))
                out.append(dl)
                at += len(dl) + 1
        out.append(ln)
        at += len(ln) + 1
    data = check_size(join(out))
    keys = listed(name, vals)
    for off, key in decoys:
        assert data[off - 1] == 10 and data[off:off + L + 1] == decoy + TAB and off // TILE in (2, 4, 6)
        assert key in keys
        real = data.index(name + TAB + field(key[1], g) + TAB)
        assert data[real - 1] == 10 and real + TILE < off
    assert decoy not in data[:TILE] and data.count(decoy + TAB) == 3
    if own_keys:
        keys = sorted(set(keys) | {(decoy, v) for _, (_, v) in decoys})
    return data, keys, decoys


# ---- C: near-miss top digits --------------------------------------------------------------------------------------------------------
def top_digit_cases():
    return [(g, i) for g in range(5, 11) for i in range(g - 4)]


def top_digit_case(g, i, L=6, seed=3):
    """(data, keys, odd): lines at 2000, 2001, ... (top digits all 0) and, in tiles 1 and 3, one line whose position column differs
    from its neighbours' in digit i alone (a 1 there).  The line's own position is not listed; the position a compare without that
    digit would take it for (the same last four digits under the stretch's top digits) IS, and its real line came earlier.
    odd: [(offset of the line, that key)]."""
    name = cell_name(L)
    lines, vals = grow(name, g, lambda n: 2000 + n, seed=seed * 100 + g, tiles=5)
    assert max(vals) < 9000 and 0 <= i < g - 4
    offs = offsets(lines)
    keys = listed(name, vals)
    out, odd, at = [], [], 0
    plan = {first_line_from(offs, t * TILE + 500): t for t in (1, 3)}
    for n, ln in enumerate(lines):
        if n in plan:
            v = vals[n - 40] if vals[n - 40] % 2 == 0 else vals[n - 39]
            f = bytearray(field(v, g))
            assert f[i] == 0x30
            f[i] = 0x31
            f = bytes(f)
            assert (name, int(f)) not in keys and int(f) % 10000 == v and int(f) // 10000 == 10 ** (g - 5 - i) and (name, v) in keys
            ol = make_line(name, f, 7000 + n, seed=seed)
            odd.append((at, (name, v)))
            out.append(ol)
            at += len(ol) + 1
        out.append(ln)
        at += len(ln) + 1
    data = check_size(join(out))
    for off, key in odd:
        assert data[off - 1] == 10 and off // TILE in (1, 3)
        assert data.index(name + TAB + field(key[1], g) + TAB) < off
    return data, keys, odd


# ---- D: every byte in a digit place -------------------------------------------------------------------------------------------------
DIGIT_CELLS = ((8, 4), (20, 10))                                # L + g <= 21 with four digits; the two-piece form, L + g = 30, with ten
ODD_BYTES = b"/:+-_@Pp`\x01\x1f!\x7f\t \v\f\r"


@functools.lru_cache(maxsize=None)
def digit_base(L, g, seed=4):
    """(lines, values, index of the line to change): the line lies in the file's last tile, with lines before and after it there."""
    name = cell_name(L)
    m = 10 ** min(g, 4)
    lines, vals = grow(name, g, (lambda i: 1000 + i) if g >= 4 else (lambda i: i % m), seed=seed * 100 + L + g, extra=1500)
    offs = offsets(lines)
    last_tile = n_tiles(join(lines)) - 1
    idx = first_line_from(offs, last_tile * TILE + 400)
    assert idx + 5 < len(lines) and max(vals) < 9000
    if g < 4:
        # These positions come again and again, and a buffer that repeats a listed position is judged by the last line of it alone
        # (Device.call_consensus).  So the line to change is at 3, 13 or 135: whatever part of that column a changed byte leaves as
        # the position is odd, hence unlisted, and the outcome never hangs on a Record built from an earlier line of a key.
        vals[idx] = (3, 13, 135)[g - 1]
        lines[idx] = make_line(name, field(vals[idx], g), idx, seed=seed * 100 + L + g)
        assert len(offsets(lines)) == len(offs) and n_tiles(join(lines)) == last_tile + 1
    return tuple(lines), tuple(vals), idx


def digit_byte_case(L, g, place, byte, seed=4):
    """(data, keys, offset of the changed line): byte `byte` at index `place` of the position column of one line of the last tile."""
    lines, vals, idx = digit_base(L, g, seed)
    name = cell_name(L)
    assert 0 <= place < g
    f = bytearray(field(vals[idx], g))
    f[place] = byte
    changed = make_line(name, bytes(f), idx, seed=seed * 100 + L + g)
    old = lines[idx]
    assert len(changed) == len(old) and [q for q in range(len(old)) if old[q] != changed[q]] == ([L + 1 + place] if old != changed else [])
    out = list(lines)
    out[idx] = changed
    data = check_size(join(out))
    off = int(offsets(lines)[idx])
    assert off // TILE == n_tiles(data) - 1 and data[off:off + len(changed)] == changed
    keys = listed(name, vals)
    if g < 4:                                                    # (see digit_base)
        parts = [p for p in bytes(f).replace(b"_", b"").replace(b"+", b"").split() if p.isdigit()]
        assert all(int(p) % 2 == 1 for p in parts[:1]) and (name, vals[idx]) not in keys
    return data, keys, off


# ---- E: starts that are none, and odd starts ----------------------------------------------------------------------------------------
START_CELLS = ((17, 4), (18, 4), (19, 4), (11, 10), (12, 10), (13, 10))      # L + g = 21, 22, 23


def _start_base(L, g, seed):
    name = cell_name(L)
    lines, vals = grow(name, g, lambda i: 1000 + i, seed=seed * 100 + L + g, tiles=5)
    return name, lines, vals, offsets(lines)


def false_start_case(L, g, ch, seed=5):
    """(data, keys, fakes): in tiles 1, 2 and 3 an unlisted line carries, inside its last column, the byte `ch` ('\\v' or '\\f') and
    then bytes that read like the start of a listed line (name TAB digits TAB ...) whose real line came earlier.  No line starts
    there.  fakes: [(offset of the would-be start, its key)]."""
    name, lines, vals, offs = _start_base(L, g, seed)
    keys = listed(name, vals)
    fakes = []
    for t in (1, 2, 3):
        i = first_line_from(offs, t * TILE + 700)
        i += vals[i] % 2 == 0                                   # an unlisted carrier
        v = vals[i - 31]
        assert vals[i] % 2 == 1 and v % 2 == 0
        fakes.append((i, v))
        lines[i] = lines[i] + ch + name + TAB + field(v, g) + TAB + b"A\t1\t.\tI"
    data = check_size(join(lines))
    offs = offsets(lines)
    out = []
    for i, v in fakes:
        off = data.index(ch + name + TAB + field(v, g) + TAB, int(offs[i])) + 1
        assert off < offs[i + 1] and data.index(b"\n" + name + TAB + field(v, g) + TAB) + 1 < offs[i]
        out.append((off, (name, v)))
    assert set(lc.line_starts(data)) == set(map(int, offs))
    return data, keys, out


def lone_cr_case(L, g, seed=6):
    """(data, keys, after): in tiles 1, 2 and 3 the line before a listed line ends in a lone '\\r'.  after: offsets of those listed
    lines, which are lines."""
    name, lines, vals, offs = _start_base(L, g, seed)
    terms = [b"\n"] * len(lines)
    after = []
    for t in (1, 2, 3):
        i = first_line_from(offs, t * TILE + 900)
        i += vals[i] % 2 == 1
        terms[i - 1] = b"\r"
        after.append(int(offs[i]))
    data = check_size(b"".join(ln + t for ln, t in zip(lines, terms)))
    for off in after:
        assert data[off - 1] == 13 and data[off:off + L + 1] == name + TAB and off in set(map(int, lc.line_starts(data)))
    return data, listed(name, vals), after


def crlf_case(L, g, seed=7):
    name, lines, vals, _ = _start_base(L, g, seed)
    data = check_size(join(lines, b"\r\n"))
    assert len(lc.line_starts(data)) == len(lines)
    return data, listed(name, vals)


ODD_SEPARATORS = (b" \t", b"\t ", b"\t\t")


def odd_separator_case(L, g, seed=8):
    """(data, keys, odd): listed lines in tiles 1 to 3 whose separator after the name, after the position, or both, is blank-TAB,
    TAB-blank or two TABs.  odd: [(offset, key)]: each is the last line of its key."""
    name, lines, vals, offs = _start_base(L, g, seed)
    combos = [(a, b) for a in (TAB,) + ODD_SEPARATORS for b in (TAB,) + ODD_SEPARATORS if (a, b) != (TAB, TAB)]
    odd = []
    for n, (a, b) in enumerate(combos):
        i = first_line_from(offs, TILE + 150 + n * 600)
        i += vals[i] % 2 == 1
        lines[i] = make_line(name, field(vals[i], g), i, seed=seed * 100 + L + g, sep1=a, sep2=b)
        odd.append((i, (name, vals[i])))
    assert len({i for i, _ in odd}) == len(combos) == 15
    data = check_size(join(lines))
    offs = offsets(lines)
    return data, listed(name, vals), [(int(offs[i]), k) for i, k in odd]


# ---- F: seams -----------------------------------------------------------------------------------------------------------------------
SEAM_CELLS = ((1, 1), (9, 4), (12, 10), (17, 5), (28, 10), (44, 10), (45, 3))
SEAM_J = range(0, 73)
SEAMS_PER_FILE = 13                                              # tile ends 1 .. 13 of a file of 15 tiles


def seam_groups():
    js = list(SEAM_J)
    return [tuple(js[a:a + SEAMS_PER_FILE]) for a in range(0, len(js), SEAMS_PER_FILE)]


def seam_case(L, g, js, seed=9, long_name=None):
    """(data, keys, seams): for the n-th j of `js` a listed line starts exactly j bytes before the end of tile n (at j = 0 the '\\n'
    in front of it is the tile's last byte); the line before it has the length that takes.  seams: [(offset, key)].
    long_name: instead, ONE unlisted line of that name starts one byte before the end of tile 0 (seams: its offset, None)."""
    name = cell_name(L)
    fixed = L + g + 6
    lo, hi = fixed + 4, 2 * fixed + 41                           # bytes of an exact_line with its '\n'
    m = 10 ** min(g, 4)
    v = 1000 % m
    lines, seams, at = [], [], 0
    vals = []

    def put(ln, value=None):
        nonlocal at
        lines.append(ln)
        if value is not None:
            vals.append(value)
        at += len(ln) + 1

    def value(parity):
        nonlocal v
        v = (v + 1) % m if g < 4 else v + 1
        if v % 2 != parity:
            v = (v + 1) % m if g < 4 else v + 1
        return v

    targets = [(TILE - 1, None)] if long_name else [((n + 1) * TILE - j, j) for n, j in enumerate(js)]
    for target, j in targets:
        while target - at > hi:
            x = value(len(lines) % 2)
            put(make_line(name, field(x, g), len(lines), seed=seed * 100 + L), x)
        assert lo <= target - at <= hi
        x = value(1)                                            # (the line of fitted length is not listed)
        put(exact_line(name, field(x, g), target - at - 1), x)
        assert at == target
        if long_name:
            put(long_name + TAB + field(value(0), g) + TAB + b"A\t2\t.,\tII")
            seams.append((target, None))
        else:
            x = value(0)
            put(make_line(name, field(x, g), len(lines), seed=seed * 100 + L), x)
            seams.append((target, (name, x)))
    x = value(0)                                                # (a listed line right behind the last one)
    put(make_line(name, field(x, g), len(lines), seed=seed * 100 + L), x)
    while at < (len(targets) + 1) * TILE + 300 or at < (MIN_TILES - 1) * TILE + 300:
        x = value(len(lines) % 2)
        put(make_line(name, field(x, g), len(lines), seed=seed * 100 + L), x)
    data = check_size(join(lines))
    keys = listed(name, vals)
    starts = set(map(int, lc.line_starts(data)))
    assert max(vals) < 9000
    for (off, key), (target, j) in zip(seams, targets):
        assert off == target and off in starts and data[off - 1] == 10
        if long_name:
            assert off % TILE == TILE - 1 and data[off:off + len(long_name) + 1] == long_name + TAB
        else:
            assert (TILE - off % TILE) % TILE == j and key in keys and data[off:off + L + 1 + g + 1] == name + TAB + field(key[1], g) + TAB
            if j == 0:
                assert off % TILE == 0
    return data, keys, seams


# ---- G: ten digits for real ---------------------------------------------------------------------------------------------------------
WIDE_CELLS = (5, 28)                                             # name lengths: short, and L + g = 38
WRAP = 4294970000                                                # top digits 429 497: 429 497 * 10 000 is 2 704 modulo 2^32


def wide_case(L, large, seed=10):
    """(data, keys): ten-digit columns.  Lines at 0 .. 119 and 2650 .. 2949 (every second one listed), then runs of true ten-digit
    values: 4 294 959 950 .. 4 294 960 049 (top digits 429 495 -> 429 496: the last top whose positions all fit 32 bits),
    4 294 967 200 .. 4 294 967 399 (through 2^32 under ONE set of top digits, 429 496: a line past 2^32 never calibrates a layout, but
    one before it does, and 429 496 * 10 000 + the last four digits of 2^32 + n is n modulo 2^32, a LISTED position for even n) and
    WRAP + n, n = 0 .. 199 — whose 32-bit remainders 2704 + n are listed too.  None of these lines is a site, unless `large`:
    then 4 294 959 999, 4 294 960 000 and 4 294 967 295 are listed (a bitmap of 2^32 bits)."""
    name = cell_name(L)
    small = list(range(0, 120)) + list(range(2650, 2950))
    vals = small + list(range(4294959950, 4294960050)) + list(range(4294967200, 4294967400)) + [WRAP + n for n in range(200)]
    lines = stretch(name, 10, vals, seed=seed * 100 + L)
    data = check_size(join(lines))
    assert len(join(lines[-200:])) > TILE + 1000                 # the run of WRAP + n: more than a tile, so some tile holds nothing else
    keys = listed(name, small)
    assert all((name, (WRAP + n) & 0xFFFFFFFF) in keys for n in range(0, 200, 2)) and (WRAP & 0xFFFFFFFF) == 2704
    past = [v for v in vals if 1 << 32 <= v < WRAP - 200]
    assert len(past) == 104 and all(v // 10000 == 429496 for v in past + [4294967200]) and all((name, v - (1 << 32)) in keys for v in past[::2])
    if large:
        keys = sorted(set(keys) | {(name, 4294959999), (name, 4294960000), (name, 4294967295)})
    return data, keys
