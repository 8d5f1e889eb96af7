"""The read-base counts of the one-lane-per-site call kernels (csrc/consensus.hip, k_call_lanes: bit planes of the bases field,
class masks, popcounts under the kept mask; the byte-by-byte walk when a quality fails or is missing) against
oracle/pileup_oracle.py through the C ABI: base, filter mask and every field of the count records, each case with count records
and without them (gpu_util.check_against_oracle runs both chains), and which pass took the lines (Device.call_pass_counts).

A window of W bytes holds a line only when the line ends inside it, so a bases field with one quality per read reaches the
128-byte pass up to about 55 reads, the 256-byte pass up to about 120 and the 512-byte pass up to 248: the fields of 254 and 255
reads with all their qualities are the wave-per-site kernel's (and checked there).  The largest counts of the lane kernels are
checked in files of their own: lines that end on the window's last byte, all qualities present (every wave on the popcount path),
and the same width with a short quality string (the byte-by-byte path)."""
import random

import pytest

from oracle import fuzz
from oracle import pileup_oracle as po
from tests import deep_lines_cases as cases
from snp_pipeline_amd import _lib as L
from tests.gpu_util import check_against_oracle, get_device, gpu_consensus

pytestmark = pytest.mark.gpu

CHROM = b"cnt"
P0 = po.CallerParams(0, 0.6, 3, 0, 0.0)
# the five caller parameter sets of tests/golden (oracle/gen_golden.py)
PARAM_SETS = ((0, 0.6, 1, 0, 0.0), (0, 0.6, 3, 0, 0.0), (15, 0.9, 5, 2, 0.1), (20, 0.75, 2, 1, 0.25), (0, 1.0, 0, 0, 0.5))
LENGTHS = (0, 1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 254, 255)
CLASSES = b"*AaCcGgNnTt.,"                                          # the thirteen classes: '*', five letters on either strand, '.' and ','
REFS = b"ACGNTacgnt"


@pytest.fixture(scope="module")
def d():
    return get_device()


class File:
    """Pileup bytes under construction: listed lines of chromosome CHROM at rising positions, unlisted fillers between them."""

    def __init__(self):
        self.out, self.keys, self.pos = b"", [], 0

    def add(self, ref, bases, quals, start=None, pos=None, depth=None, chrom=CHROM):
        """One listed line; start: the byte offset of its first byte within its 16-byte block (a filler in front makes it so)."""
        self.pos = pos if pos is not None else self.pos + 1
        if start is not None:
            pad = (start - len(self.out)) % 16
            if pad:
                self.out += cases.filler(self.pos, pad + 32, b"\n") + b"\n"
            assert len(self.out) % 16 == start
        ln = cases.line(self.pos, ref, bases, quals, depth=depth if depth is not None else max(1, len(quals)), chrom=chrom)
        self.last = (len(self.out), len(self.out) + len(ln) - len(quals) - 1 - len(bases))       # where the line and its bases field begin
        self.out += ln + b"\n"
        self.keys.append((chrom, self.pos))
        return self

    def done(self):
        """Short fillers until the lines average under 100 bytes: the 128-byte pass runs (k_call_mode)."""
        n = self.out.count(b"\n")
        more = max(0, (len(self.out) - 90 * n + 49) // 50)
        return self.out + (cases.filler(1, 40, b"\n") + b"\n") * more, self.keys


def check(d, f, params=(P0,), passes=True):
    data, keys = f.done() if isinstance(f, File) else f
    res = None
    for p in params:
        res = check_against_oracle(d, data, keys, [], p)
    took = d.call_pass_counts()
    assert sum(took.values()) == len(keys)
    if passes:
        assert took == cases.expected_passes(data, set(keys)), took
    return res, took


def reads_of(n, symbol):
    return bytes([symbol]) * n


def test_field_lengths_one_class(d):
    """Every length edge, one class filling the field (a single count of up to 255), every class in turn over the lengths."""
    f = File()
    for i, n in enumerate(LENGTHS):
        for j in range(3):
            sym = CLASSES[(3 * i + j) % len(CLASSES)]
            if n == 0:
                f.add(b"A", b"*", b"*", depth=0) if j == 0 else f.add(b"A", b"", b"", depth=1 + j)
            else:
                f.add(b"G", reads_of(n, sym), b"I" * n)
    res, took = check(d, f, (P0, po.CallerParams(13, 0.6, 3, 0, 0.0)))
    assert took["lanes128"] and took["lanes256"] and took["lanes512"] and took["wave"] == 6      # 254 and 255 reads: over 512 bytes
    assert int(res.counts["total"][:, 0].max()) == 255


REF_T = b"T"


def _head(pos):
    """Bytes of a line of REF_T besides its bases and qualities (a depth of three digits)."""
    return len(cases.line(pos, REF_T, b"", b"", depth=100, chrom=CHROM))


def _expected_symbol(sym):
    """(ranked symbol, on the forward strand) of a read byte over REF_T: '.' and ',' stand for the reference base."""
    c = bytes([sym])
    return (REF_T if c in b".," else c.upper())[0], c in b".*" or c.isupper()


def _widest_lines(f):
    """Every class alone in a line that starts on a 16-byte boundary, has one quality per read and ends on the last byte that the
    512-byte window holds: as many reads as fit (248), and bases fields of 255 and 254 BYTES, of which as few as fit are '^x' pairs
    (241 and 242 reads).  Returns [(key, symbol, forward, count)]."""
    want = []
    f.pos = 99                                                     # positions of three digits throughout: one head length
    for sym in CLASSES:
        one = bytes([sym])
        head = _head(f.pos + 1)
        n = (511 - head) // 2
        f.add(REF_T, one * n, b"I" * n, start=0)
        assert n == 248 and len(f.out) - 1 - f.last[0] == 511 and f.last[0] % 16 == 0       # the newline: the window's last byte
        want.append((f.keys[-1],) + _expected_symbol(sym) + (n,))
        for size in (255, 254):
            reads = min(size, 511 - head - size)
            pairs = (size - reads + 1) // 2                         # a pair is three bytes and one read
            reads = size - 2 * pairs
            f.add(REF_T, (b"^I" + one) * pairs + one * (size - 3 * pairs), b"I" * reads, start=0)
            assert len(f.out) - 1 - f.last[0] == 511 and f.last[0] % 16 == 0
            want.append((f.keys[-1],) + _expected_symbol(sym) + (reads,))
    return want


def _slots(d, data, keys, p, want_counts):
    _, res, ss = gpu_consensus(d, data, keys, [], p, want_counts=want_counts)
    return res, {key: s for s, key in enumerate(ss.key_tuples())}


def test_widest_lines_of_the_512_window_one_class(d):
    """The largest single counts the popcount path can meet.  No line of this file lacks a quality and -q is 0, so every wave of
    every pass is on the popcount path.  With count records every field is checked against the oracle and, here, against the
    count the line was built with; without them the count shows in the depth filter: min_cons_depth at each count and one above."""
    f = File()
    want = _widest_lines(f)
    data, keys = f.done()
    assert sorted({n for *_, n in want}) == [241, 242, 248] and len(keys) == 3 * len(CLASSES) <= 64
    for depth in (241, 242, 248, 249):
        p = po.CallerParams(0, 0.6, depth, 0, 0.0)
        check_against_oracle(d, data, keys, [], p)
        assert d.call_pass_counts() == {"lanes128": 0, "lanes256": 0, "lanes512": len(keys), "wave": 0}
        res, slot = _slots(d, data, keys, p, True)
        res2, slot2 = _slots(d, data, keys, p, False)
        for key, sym, forward, n in want:
            c = res.counts[slot[key]]
            assert (int(c["good_depth"]), int(c["fwd_good_depth"]), int(c["rev_good_depth"])) == (n, n if forward else 0, 0 if forward else n), key
            assert int(c["n_symbols"]) == 1 and int(c["sym"][0]) == sym, key
            assert (int(c["total"][0]), int(c["fwd"][0]), int(c["rev"][0])) == (n, n if forward else 0, 0 if forward else n), key
            mask = L.F_DEPTH if n < depth else 0
            base = 0x2D if mask or sym == 0x2A else sym
            assert (int(c["filters"]), int(res.filters[slot[key]]), int(res.bases[slot[key]])) == (mask, mask, base), (key, depth)
            assert (int(res2.filters[slot2[key]]), int(res2.bases[slot2[key]])) == (mask, base), (key, depth)


def test_widest_lines_with_a_short_quality_string(d):
    """A bases field of 255 bytes (254 reads and a '$') with as many qualities as the 512-byte window still holds, 241: a quality
    is missing, the whole wave walks its bytes one by one (the paired path), and the count is the number of qualities."""
    f = File()
    f.pos = 99
    want = []
    for sym in b"At,*":
        quals = 511 - _head(f.pos + 1) - 255
        f.add(REF_T, bytes([sym]) * 254 + b"$", b"I" * quals, start=0, depth=254)
        want.append((f.keys[-1],) + _expected_symbol(sym) + (quals,))
    data, keys = f.done()
    check_against_oracle(d, data, keys, [], P0)
    assert d.call_pass_counts() == {"lanes128": 0, "lanes256": 0, "lanes512": 4, "wave": 0}
    res, slot = _slots(d, data, keys, P0, True)
    for key, sym, forward, n in want:
        c = res.counts[slot[key]]
        assert n == 241 and (int(c["good_depth"]), int(c["sym"][0]), int(c["total"][0]), int(c["fwd"][0])) == (n, sym, n, n if forward else 0), key


@pytest.mark.parametrize("n", (5, 33, 41, 65, 129))
def test_field_alignment(d, n):
    """The line at every offset 0-15 of its 16-byte block, chromosome names of 1-4 bytes: the field at every byte of a dword."""
    f = File()
    rng = random.Random(n)
    seen = set()
    f.pos = 99
    for width in range(1, 5):
        for start in range(16):
            bases = bytes(rng.choice(CLASSES) for _ in range(n))
            f.add(b"C", bases, b"I" * n, start=start, chrom=b"cntx"[:width])
            assert f.out[f.last[1]:f.last[1] + n] == bases
            seen.add((f.last[0] % 16, f.last[1] % 4))
    assert seen == {(s, b) for s in range(16) for b in range(4)}
    check(d, f)


def test_every_class_alone_and_mixed(d):
    f = File()
    for sym in CLASSES:
        for n in (1, 7, 30):
            f.add(b"G", reads_of(n, sym), b"I" * n)
    for ref in REFS:                                               # '.' and ',' stand for the reference base, in either case
        f.add(bytes([ref]), b"..,.,,,." + CLASSES, b"I" * (8 + len(CLASSES)))
        f.add(bytes([ref]), b".", b"I")
        f.add(bytes([ref]), b",,", b"II")
    rng = random.Random(3)
    for _ in range(40):
        n = rng.randint(1, 50)
        f.add(bytes([rng.choice(REFS)]), bytes(rng.choice(CLASSES) for _ in range(n)), b"I" * n)
    check(d, f, tuple(po.CallerParams(*p) for p in PARAM_SETS))


def test_reference_r_goes_to_the_wave_kernel(d):
    f = File()
    for _ in range(30):
        f.add(b"A", b".,.,G", b"IIIII")
    f.add(b"R", b"..,,A", b"IIIII").add(b"r", b",", b"I").add(b"R", b"ACGT", b"IIII")     # the last has no '.' / ',': a lane calls it
    data, keys = f.done()
    check_against_oracle(d, data, keys, [], P0)
    assert d.call_pass_counts() == {"lanes128": 31, "lanes256": 0, "lanes512": 0, "wave": 2}


def test_bytes_that_look_like_classes_but_are_not_counted(d):
    f = File()
    fields = [b"^A.", b"^aT", b"^*,", b"^.G", b"^,c", b"^NA", b"^^A", b"^^^A.", b"^^^^A", b"^^^^^AC", b"A^^", b"A^^^", b"AC^",
              b".$", b"A$", b"t$,$", b"$", b".+2AC,", b",-2ac.", b"A+2ACG", b"C-12ACGTACGTACGTt", b"A-12ACG", b".+3AC", b"*", b"**a*",
              b".-1*A", b"^$A$", b".+10ACGTNacgtnT,", b"^+.", b"^-1A", b"A+2^AC"]
    for bases in fields:
        for pre in (b"", b"Ac.,", b"G" * 29, b"t" * 61):
            body = pre + bases
            f.add(b"A", body, b"I" * len(body))                    # (the zip stops at the shorter: qualities to spare)
    data, keys = f.done()
    for p in (P0, po.CallerParams(13, 0.6, 3, 0, 0.0)):
        check_against_oracle(d, data, keys, [], p)
    assert sum(d.call_pass_counts().values()) == len(keys)


def test_other_symbols_are_handed_on(d):
    """An IUPAC letter, '>' or '<' anywhere in the field: the wave-per-site kernel's, with the oracle's result."""
    f = File()
    n_odd = 0
    for sym in b"RYKMSWrykmsw><":
        for n, at in ((1, 0), (9, 0), (9, 8), (40, 31), (40, 32), (40, 33), (40, 39), (100, 63), (100, 64), (100, 99), (200, 128), (200, 199)):
            body = bytearray(b"Ac.,G"[i % 5] for i in range(n))
            body[at] = sym
            f.add(b"A", bytes(body), b"I" * n)
            n_odd += 1
    for _ in range(20):
        f.add(b"A", b"^RA^>c^<.", b"III")                           # ... but not as the byte after a '^'
    data, keys = f.done()
    check_against_oracle(d, data, keys, [], P0)
    took = d.call_pass_counts()
    assert took == cases.expected_passes(data, set(keys)) and took["wave"] == n_odd and took["lanes128"] == 20


def _two_wave_file(short_at, bad_quality_at=()):
    f = File()
    rng = random.Random(21)
    for i in range(128):
        n = rng.randint(4, 40)
        bases = bytes(rng.choice(CLASSES + b"ACGT.,.,") for _ in range(n))
        quals = bytearray(b"I" * n)
        if i in bad_quality_at:
            quals[n // 2] = 33 + 12
        if i in short_at:
            quals = quals[:-1]
        f.add(bytes([rng.choice(REFS)]), bases, bytes(quals), depth=n)
    return f.done()


@pytest.mark.parametrize("minq", (0, 13))
def test_both_paths_in_one_launch(d, minq):
    """One line per wave of 64 sites with a quality string one short (minq 13: and one failing quality): its whole wave takes the
    paired path.  Every other lane gives what it gives when all waves take the count path."""
    p = po.CallerParams(minq, 0.6, 3, 0, 0.0)
    odd = (5, 64 + 17)
    plain, keys = _two_wave_file(())
    mixed, keys2 = _two_wave_file(odd, odd if minq else ())
    assert keys == keys2
    a = check_against_oracle(d, plain, keys, [], p)
    assert d.call_pass_counts()["lanes128"] == 128
    b = check_against_oracle(d, mixed, keys, [], p)
    assert d.call_pass_counts()["lanes128"] == 128
    _, res_a, ss = gpu_consensus(d, plain, keys, [], p, want_counts=False)
    _, res_b, _ = gpu_consensus(d, mixed, keys, [], p, want_counts=False)
    slots = {key: s for s, key in enumerate(ss.key_tuples())}
    assert sorted(slots[keys[i]] // 64 for i in odd) == [0, 1]      # one in each wave
    changed = {slots[keys[i]] for i in odd}
    for s in range(128):
        if s in changed:
            assert a.counts[s]["good_depth"] > b.counts[s]["good_depth"]
        else:
            assert a.counts[s].tobytes() == b.counts[s].tobytes(), s
            assert (a.bases[s], a.filters[s], res_a.bases[s], res_a.filters[s]) == (b.bases[s], b.filters[s], res_b.bases[s], res_b.filters[s])


@pytest.fixture(scope="module")
def fuzz_file():
    rng = random.Random(2024)
    f = File()
    for _ in range(2000):
        depth = rng.randint(1, 120)
        bases = "".join(fuzz._bases_token(rng) for _ in range(depth))
        if rng.random() < 0.75:                                    # ('#', '<' or '>' sends a line to the wave-per-site kernel)
            bases = bases.replace("#", "*").replace("<", "*").replace(">", "*")
        bases = bases.encode()
        # one quality per token: every token of the alphabet is one read (a '^' pair, a '$' and an indel ride on a read)
        quals = bytes(rng.randint(33, 74) for _ in range(depth))
        f.add(bytes([rng.choice(REFS)]), bases, quals, depth=depth)
    return f.done()


@pytest.mark.parametrize("k", range(2))
def test_seeded_fuzz(d, fuzz_file, k):
    data, keys = fuzz_file
    check(d, (data, keys), (po.CallerParams(*PARAM_SETS[1]), po.CallerParams(*PARAM_SETS[2]))[k:k + 1], passes=False)
    took = d.call_pass_counts()
    # The lines are well formed and every sign is a marker: a lane pass hands a line on only for '#', '<' or '>' outside a '^x' pair.
    want = cases.expected_passes(data, set(keys))
    assert want["lanes128"] > 300 and want["lanes256"] > 300 and want["lanes512"] > 100 and want["wave"] > 100
    if k == 0:                                                     # -q 0: every quality passes, such a symbol is always a read
        assert took == want
    else:                                                          # -q 15: ... it is no read when its quality fails, and its line stays
        most = cases.expected_passes(data.replace(b"#", b"*").replace(b"<", b"*").replace(b">", b"*"), set(keys))
        assert all(want[n] <= took[n] <= most[n] for n in ("lanes128", "lanes256", "lanes512")) and took["wave"] >= most["wave"]
