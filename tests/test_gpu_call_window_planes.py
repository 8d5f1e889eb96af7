"""The 128-byte call window through its bit planes (csrc/consensus.hip, k_call_lanes<128>: one gather of the staged window, the
tokeniser, the bases field's planes and the quality test all from it) against oracle/pileup_oracle.py through the C ABI: base,
filter mask and every field of the count records, with count records and without them (gpu_util.check_against_oracle runs both
chains), and which pass took which line (Device.call_pass_counts) by the rules the lane passes have always had — the change must
not make the 128-byte pass take a line it used to hand on, or hand on one it used to take.

Those rules, for a line of six or more fields whose symbols the lane passes count: a window of W bytes starts at the 16-byte
boundary at or below the line's first byte; the pass takes the line when the first byte of 10..13 after the line's start lies
inside the window and is '\\n' or '\\r' (a '\\v' or '\\f' there sends the line on, to the end of the chain) and the bases field is
at most 64 / 128 / 255 bytes; the 128-byte pass runs when the file's lines average at most 100 bytes."""
import random
import re

import pytest

from oracle import pileup_oracle as po
from tests import deep_lines_cases as cases
from tests.gpu_util import check_against_oracle, get_device

pytestmark = pytest.mark.gpu

CHROM = b"win"
P0 = po.CallerParams(0, 0.6, 3, 0, 0.0)


@pytest.fixture(scope="module")
def d():
    return get_device()


class File:
    """Pileup bytes under construction: listed lines at rising positions, short unlisted fillers where a line has to start at a
    given byte of its 16-byte block."""

    def __init__(self):
        self.out, self.keys, self.pos = b"", [], 99              # positions of three digits throughout

    def add(self, ref, bases, quals, start=None, depth=None, chrom=CHROM, sep=b"\t", term=b"\n", tail=b""):
        self.pos += 1
        if start is not None:
            pad = (start - len(self.out)) % 16
            if pad:
                self.out += cases.filler(self.pos, pad + 32, b"\n") + b"\n"
            assert len(self.out) % 16 == start
        n = depth if depth is not None else max(1, len(quals))
        fields = [chrom, b"%d" % self.pos, ref, b"%d" % n] + ([bases, quals] if bases else [])
        ln = sep.join(fields) + tail
        self.at = len(self.out)                                  # where the line begins ...
        self.field_at = self.at + len(ln) - len(tail) - len(quals) - len(sep) - len(bases)      # ... and its bases field
        self.out += ln + term
        self.keys.append((chrom, self.pos))
        return self

    def window_byte(self, offset):
        """The byte of the 128-byte window that byte `offset` of the file falls on, for the line added last."""
        return offset - (self.at & ~15)

    def done(self):
        """Short fillers until the lines average under 100 bytes: the 128-byte pass runs (k_call_mode)."""
        n = len(re.findall(rb"\r\n|\n|\r", self.out))
        more = max(0, (len(self.out) - 90 * n + 49) // 50)
        return self.out + (cases.filler(1, 40, b"\n") + b"\n") * more, self.keys


def expected_passes(data, listed):
    """Which pass takes each listed line, by the rules in the header (lines as Python's universal newlines split them)."""
    starts, at = [], 0
    for m in re.finditer(rb"\r\n|\n|\r", data):
        starts.append((at, m.start()))
        at = m.end()
    assert at == len(data)
    deep = len(data) > 100 * len(starts)
    took = {"lanes128": 0, "lanes256": 0, "lanes512": 0, "wave": 0}
    for start, stop in starts:
        f = po.split_fields(data[start:stop])
        if len(f) < 2 or not f[1].isdigit() or (f[0], int(f[1])) not in listed:
            continue
        assert len(f) >= 6 or len(f) == 4
        first = re.search(rb"[\n\x0b\x0c\r]", data[start:]).start()
        end_at = (start & 15) + first
        field = f[4] if len(f) >= 6 else b""
        plain = not re.sub(rb"[.,ACGTNacgtn*$+\-0-9]", b"", re.sub(rb"\^.", b"", field))
        name = "wave"
        if data[start + first] in b"\n\r":
            for cand, win, most in cases.WINDOWS:
                if plain and end_at < win and len(field) <= most and not (deep and win == 128):
                    name = cand
                    break
        took[name] += 1
    return took


def check(d, f, params=(P0,)):
    data, keys = f.done()
    res = None
    for p in params:
        res = check_against_oracle(d, data, keys, [], p)
        took = d.call_pass_counts()
        assert took == expected_passes(data, set(keys)), took
    return took


def field_of(n, rng=None):
    """A bases field of n bytes and its reads' qualities: every other byte a '$' (which rides on a read), so that a field of 64
    bytes and its qualities still end inside the window."""
    sym = b"ACGTacgt.,*"
    bases = b"".join(bytes([rng.choice(sym) if rng else sym[i % len(sym)]]) + b"$" for i in range(n // 2)) + (b"g" if n & 1 else b"")
    return bases, b"I" * ((n + 1) // 2)


def test_line_start_and_field_start_at_every_byte(d):
    """The line at every offset 0..15 of its 16-byte block and contig names of 1..90 bytes: the bases field begins at every byte
    offset mod 32 of the window, before, across and behind the window's bytes 32, 64 and 96, and is as long as still fits."""
    f = File()
    rng = random.Random(1)
    seen_o, seen_bs, crossing = set(), set(), set()
    for width in range(1, 91):
        for start in sorted({(5 * width) % 16, (5 * width + 9) % 16, (width + 1) % 16}):
            head = width + 1 + 3 + 1 + 1 + 1 + 2 + 1
            room = 127 - start - head                            # bytes of field + separator + qualities before the terminator's last place
            n = min(64, (room - 1) * 2 // 3)
            if n < 1:
                continue
            bases, quals = field_of(n, rng)
            f.add(b"C", bases, quals, start=start, depth=10 + len(quals) % 80, chrom=b"n" * width)
            bs = f.window_byte(f.field_at)
            assert bs == start + head and f.out[f.field_at:f.field_at + n] == bases and f.window_byte(len(f.out) - 1) <= 127
            seen_o.add(start)
            seen_bs.add(bs)
            crossing |= {edge for edge in (32, 64, 96) if bs < edge < bs + n}
    for start in range(16):                                      # ... and every line start with the shortest head
        f.add(b"G", b".,.,A", b"IIIII", start=start, chrom=b"n")
        seen_o.add(start)
    assert seen_o == set(range(16)) and {bs % 32 for bs in seen_bs} == set(range(32)) and crossing == {32, 64, 96}
    assert min(seen_bs) < 32 and max(seen_bs) > 96
    took = check(d, f)
    assert took["lanes128"] == len(f.keys)


def test_field_lengths(d):
    """Bases fields of 0, 1, 31, 32, 33, 63, 64 and 65 bytes at four line starts; 65 is the 256-byte pass's."""
    f = File()
    for n in (0, 1, 31, 32, 33, 63, 64, 65):
        for start in (0, 5, 11, 15):
            if n == 0:
                f.add(b"A", b"", b"", start=start, depth=2)      # four fields
            else:
                f.add(b"T", *field_of(n), start=start)
            assert f.window_byte(len(f.out) - 1) <= 127
    took = check(d, f, (P0, po.CallerParams(0, 0.6, 30, 0, 0.0)))
    assert took == {"lanes128": 28, "lanes256": 4, "lanes512": 0, "wave": 0}


@pytest.mark.parametrize("sep", (9, 11, 12, 28, 29, 30, 31, 32))
def test_separators(d, sep):
    """Every separator of str.split() between the fields, alone, doubled and tripled, and behind the last field; '\\v' and '\\f'
    are terminator candidates to the lane passes, which hand such a line on."""
    f = File()
    one = bytes([sep])
    for rep in (1, 2, 3):
        for start in (0, 9, 15):
            f.add(b"A", b".,.,G^Ic$", b"IIIIII", start=start, sep=one * rep)
            f.add(b"g", b"AAAAc+2TTa-1n.", b"JJJJJJJ", start=start, sep=one * rep, tail=one * (rep - 1))
            f.add(b"C", b"*tT", b"III", start=start, sep=b"\t" + one * rep)
    for _ in range(20):
        f.add(b"A", b".,.,", b"IIII")                            # plain lines between them
    took = check(d, f)
    assert (took["wave"], took["lanes128"]) == ((27, 20) if sep in (11, 12) else (0, 47))


def test_terminators(d):
    """Lines ended by '\\n', '\\r\\n' and a lone '\\r' are the 128-byte pass's; '\\v' or '\\f' before the '\\n' sends the line on."""
    f = File()
    rng = random.Random(3)
    for i in range(40):
        for term in (b"\n", b"\r\n", b"\r", b"\x0b\n", b"\x0c\n", b" \x0b\r\n"):
            n = rng.randint(1, 40)
            bases, quals = field_of(n, rng)
            f.add(b"A", bases, quals, start=(i + len(term)) % 16 if i % 3 else None, term=term)
    took = check(d, f)
    assert took == {"lanes128": 120, "lanes256": 0, "lanes512": 0, "wave": 120}


def test_line_ends_on_the_windows_last_byte_and_one_behind_it(d):
    """The terminator on byte 127 of the window: the 128-byte pass's.  On byte 128: the 256-byte pass's."""
    f = File()
    want = {"lanes128": 0, "lanes256": 0, "lanes512": 0, "wave": 0}
    for start in range(16):
        for end_at, name in ((127, "lanes128"), (128, "lanes256"), (126, "lanes128")):
            for term in (b"\n", b"\r\n"):
                head = len(CHROM) + 1 + 3 + 1 + 1 + 1 + 2 + 1
                rest = end_at - start - head - 1                 # field + qualities
                reads = rest // 2 - 2
                dollars = rest - 2 * reads
                bases = b"Ac" * (reads // 2) + b"." * (reads & 1) + b"$" * dollars
                assert len(bases) <= 64
                f.add(b"A", bases, b"I" * reads, start=start, depth=reads, term=term)
                assert f.window_byte(len(f.out) - len(term)) == end_at
                want[name] += 1
    took = check(d, f, (P0, po.CallerParams(0, 0.6, 45, 0, 0.0)))
    assert took == want


@pytest.mark.parametrize("minq", (0, 15, 40))
def test_qualities_at_the_threshold(d, minq):
    """One quality of thr - 1, thr and thr + 1 (thr = 33 + minq) among passing ones, at the first, the last and every other place
    of fields that lie across the window's bytes 32, 64 and 96.  (At -q 0, thr - 1 is a blank: it ends the quality field.)"""
    thr = 33 + minq
    p = po.CallerParams(minq, 0.6, 3, 0, 0.0)
    f = File()
    for n in (1, 2, 17, 40):
        for at in sorted({0, n // 2, n - 1} | set(range(0, n, 3))):
            for q in (thr - 1, thr, thr + 1):
                for start in (0, 13):
                    quals = bytearray(b"~" * n)
                    quals[at] = q
                    if not bytes(quals).strip():
                        continue                                 # (a blank alone is no field)
                    f.add(b"T", bytes(b"AcGt."[i % 5] for i in range(n)), bytes(quals), start=start, depth=n)
    for q in (thr - 1, thr, thr + 1):                            # ... and every quality the same
        for n in (1, 31, 32, 33, 50) if q != 32 else ():
            f.add(b"A", b"a" * n, bytes([q]) * n, depth=n)
    took = check(d, f, (p,))
    assert took["lanes128"] == len(f.keys)


def test_quality_field_shorter_and_longer_than_the_kept_bases(d):
    f = File()
    for n in (1, 2, 5, 31, 32, 33, 40):
        for delta in (-1, 0, 1, 3):
            for bases in (b"A" * n, b"^Ia" * (n // 3) + b"c" * (n - 3 * (n // 3)), b"t$" * (n // 2) + b"G" * (n & 1), b".+2AC" * (n // 5) + b"," * (n % 5)):
                kept = len(re.sub(rb"\^.|\$|[+-]2AC", b"", bases))
                if kept + delta >= 1:
                    f.add(b"C", bases, b"I" * (kept + delta), depth=max(1, kept))
    took = check(d, f, (P0, po.CallerParams(20, 0.6, 3, 0, 0.0)))
    assert took["lanes128"] == len(f.keys)


def test_markers_across_the_word_boundaries(d):
    """'^x' pairs, '$', indel markers and '*' ending at, beginning at and straddling bytes 32, 64 and 96 of the window (the dwords
    the field's planes are shifted out of) and bytes 32 and 64 of the field (its two mask words)."""
    f = File()
    markers = (b"^I", b"^^", b"^+", b"$", b"+2AC", b"-1n", b"+12ACGTACGTACGT", b"*")
    head = len(CHROM) + 1 + 3 + 1 + 1 + 1 + 2 + 1
    n_lines = 0
    for m in markers:
        for start in (0, 7):
            for edge in (32, 64, 96):                            # of the window
                for begin in {edge - len(m), edge - max(1, len(m) // 2), edge - 1, edge}:
                    lead = begin - start - head                  # bytes of the field before the marker
                    if lead < 1 or lead + len(m) + 2 > 64:
                        continue
                    bases = b"Ac" * (lead // 2) + b"." * (lead & 1) + m + b"gT"
                    reads = lead + 2 + (1 if m == b"*" else 0)
                    quals = b"I" * min(reads, 126 - start - head - len(bases) - 1)      # (what the window holds; the zip truncates)
                    if not quals:
                        continue
                    f.add(b"T", bases, quals, start=start, depth=10 + reads % 80)      # (two digits, as `head` has it)
                    assert f.window_byte(f.field_at) + lead == begin and f.window_byte(len(f.out) - 1) <= 127
                    n_lines += 1
            for at in (31, 32, 33, 63, 64):                      # of the field: the marker's last byte there
                lead = at + 1 - len(m)
                if lead < 1 or at + 1 > 64:
                    continue
                bases = b"aC" * (lead // 2) + b"," * (lead & 1) + m
                room = 126 - start - head - len(bases) - 1
                if room < 1:
                    continue
                f.add(b"G", bases, b"I" * min(lead + 1, room), start=start, depth=10 + lead)
                n_lines += 1
    assert n_lines > 150
    took = check(d, f, (P0, po.CallerParams(13, 0.6, 3, 0, 0.0)))
    assert took["lanes128"] == len(f.keys)
