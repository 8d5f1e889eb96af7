"""One site set, every look-up of it.  bit_off[contig] + pos goes to a bitmap word, rank[word] + popc(word & ((1 << shf) - 1)) gives
the site; csrc/scan.hip writes that out four times, and each case below runs through all of them and is held against the statements
of tests/lines_cases.py (which key a line is at, the last line of every key, the flag byte of every line):

  window    TAB-separated lines, call_consensus(want_counts=True): k_scan_wave<false, 0>.  A line whose name has at most 44 bytes and
            whose position has at most 10 digits takes the one-lane-per-line parse and the register-window probe (two VGPRs of 64
            words, ds_bpermute, refill loop); a line of another contig than the wave's hint waits for the tile's second trip and is
            probed there.  (A second contig change within one 4 KiB tile, and a name over 44 bytes, go to the queue: the cases give
            every contig more than a tile of lines.)
  depth     the same bytes, want_depth_sum=True: snpgpu_scan_range launches k_scan_wave<false, 4> — the same parse and probe compiled
            a second time with the depth column added, registers allocated anew.  It is NOT the exact instantiation: k_scan_wave<true, 0>
            returns at once unless the queue overflowed (scan.hip, `if (kExact && a.ctl[1] == 0) return`), so its loop is reached by a
            file with more odd lines than the queue holds and by nothing else (test_exact_pass_at_a_contigs_last_position below,
            beside tests/test_gpu_consensus.py::test_queue_overflow_takes_the_exact_pass).
  queue     the same lines with two blanks in place of the first TAB: the blank after the name passes as a separator, the digit window
            then starts with a blank (no digit: `bad`), and the line is left to k_scan_queue's exact parser.  No case comes near the
            queue's 983 040 entries.
  flags     call_all_lines(check=False): k_lines_flags, a lane per line.

Each case aims at one edge of the geometry: contigs packed into one bitmap without word alignment (one past a contig's max_pos is
the next contig's bit 0, in the same word: only `pos <= max_pos` keeps a line from its neighbour's site), the popcount mask and the
rank directory, the 64-word register window, the forms a contig name takes in the wave's hint.  The flags are a seeded irregular
choice among IN_SNPLIST, IN_SNPLIST | EXCLUDED and EXCLUDED, so that a rank that is off by one returns a different byte."""
import random

import numpy as np
import pytest

from oracle import pileup_oracle as po
from snp_pipeline_amd import _lib as L
from snp_pipeline_amd import device as dev
from tests import lines_cases as lc
from tests.gpu_util import check_against_oracle, get_device

pytestmark = pytest.mark.gpu

P = po.CallerParams(0, 0.6, 1, 0, 0.0)
FLAG_VALUES = (L.SITE_IN_SNPLIST, L.SITE_IN_SNPLIST | L.SITE_EXCLUDED, L.SITE_EXCLUDED)
TILE = 4096


@pytest.fixture(scope="module")
def d():
    return get_device()


@pytest.fixture(scope="module")
def prm():
    return dev.make_params(P.min_base_quality, P.min_cons_freq, P.min_cons_depth, P.min_cons_strand_depth, P.min_cons_strand_bias)


def _text(lines, sep=b"\t", seed=0):
    """(name, position) pairs as pileup lines ending in '\\n' (short: 0 to 8 reads)."""
    return b"".join(lc.pileup_line(name, pos, sep=sep, seed=seed) + b"\n" for name, pos in lines)


def _flags_for(keys, seed):
    rng = random.Random(seed)
    return [rng.choice(FLAG_VALUES) for _ in keys]


def _bit_offsets(keys):
    """bit_off and max_pos per contig as snpgpu_siteset_create lays them out (contigs bytewise sorted, max_pos + 1 bits each)."""
    top = {}
    for c, p in keys:
        top[c] = max(top.get(c, 0), p)
    off, at = {}, 0
    for c in sorted(top):
        off[c] = at
        at += top[c] + 1
    return off, top, at


def _four_ways(d, prm, tmp_path, lines, keys, seed, oracle=True):
    """The case through the four look-ups (module docstring) and, once, through check_against_oracle for the bases and counts."""
    flags = _flags_for(keys, seed)
    ss = d.siteset(keys, flags)
    order = ss.key_tuples()
    assert sorted(order) == sorted(set(keys))
    tab, blanks = _text(lines, seed=seed), _text(lines, sep=b"  ", seed=seed)
    assert blanks.replace(b"  ", b"\t") == tab and len(blanks) == len(tab) + len(lines)
    for name, data, kw in (("window", tab, {"want_counts": True}), ("depth", tab, {"want_depth_sum": True}), ("queue", blanks, {"want_counts": True})):
        starts = lc.line_starts(data)
        last, hits = lc.last_line_of(data, starts, keys)
        res = d.call_consensus(ss, data, prm, **kw)
        got = d.line_offsets(ss).astype(np.int64)
        want = np.asarray([last[k] for k in order], dtype=np.int64)
        wrong = np.nonzero(got != want)[0]
        assert len(wrong) == 0, (name, [(order[i], int(got[i]), int(want[i])) for i in wrong[:6]])
        assert (res.n_matched, res.n_lines) == (hits, len(lines)), name
        if name == "depth":
            assert res.depth_sum == po.depth_sum(data)
    path = str(tmp_path / "reads.all.pileup")
    with open(path, "wb") as f:
        f.write(tab)
    starts = lc.line_starts(tab)
    off, fl, _ = d.call_all_lines(ss, path, prm, check=False)
    assert np.array_equal(off.astype(np.int64), starts + 1)
    want = lc.line_flags(tab, starts, keys, flags)
    wrong = np.nonzero(fl != want)[0]
    assert len(wrong) == 0, ("flags", [(lines[i], int(fl[i]), int(want[i])) for i in wrong[:6]])
    if oracle:
        by_key = dict(zip(keys, flags))
        snps = [k for k in keys if by_key[k] & L.SITE_IN_SNPLIST]
        check_against_oracle(d, tab, snps, [k for k in keys if by_key[k] & L.SITE_EXCLUDED], P)
    return want, hits


# ---- neighbouring contigs in one word -----------------------------------------------------------------------------------------------
SPANS = [(b"a", 31), (b"a0", 1), (b"b", 32), (b"c", 33), (b"d", 33), (b"e", 2047), (b"f", 2048), (b"g", 2049)]      # bits: max_pos + 1
ABSENT = b"c5"                                                  # in the file, not in the set, sorts between c and d


def _neighbour_case():
    keys = [(b"a", p) for p in (3, 17, 29, 30)]                 # the first contig: a few positions; every other one 0 .. 33 densely
    for c, span in SPANS[1:]:
        keys += [(c, p) for p in range(0, min(34, span))] + [(c, span - 1)] + ([(c, span - 2)] if span > 40 and c != b"f" else [])
    keys = sorted(set(keys))
    bit_off, top, total_bits = _bit_offsets(keys)
    assert [top[c] + 1 for c, _ in SPANS] == [s for _, s in SPANS]
    assert {31, 0, 1, 2} <= {bit_off[c] % 32 for c, _ in SPANS}
    # the lines one to 34 past the last contig's max_pos stay inside the bitmap's spare word (n_words = ceil(bits / 32) + 1)
    assert total_bits + 33 < ((total_bits + 31) // 32 + 1) * 32
    lines = []
    for c, span in SPANS:
        m = span - 1
        at = set(range(0, 41)) | {m - 1, m} | set(range(m + 1, m + 35))
        at |= set(range(m + 35, m + 230)) if c != SPANS[-1][0] else set(range(41, 236))      # (bulk: more than a tile of lines per contig)
        lines += [(c, p) for p in sorted(at) if p >= 0]
        if c == b"c":
            lines += [(ABSENT, p) for p in range(0, 200)]
    lines += [(b"e", 2046), (b"b", 31), (b"g", 0), (b"a0", 0), (b"a0", 1)]      # again, out of order: the last line of a key wins
    return lines, keys


def test_neighbouring_contigs_share_bitmap_words(d, prm, tmp_path):
    """Eight contigs (a prefix pair a / a0 among them) of 31, 1, 32, 33, 33, 2047, 2048 and 2049 bits: their first bits lie at 31, 0,
    1 and 2 modulo 32.  Every contig has lines at max_pos - 1, max_pos and max_pos + 1 .. + 34, and the next contig lists 0 .. 33:
    without `pos <= max_pos` each of those 34 lines is a site of its neighbour.  "0" is a position.  A contig that is not in the
    set lies between two that are."""
    lines, keys = _neighbour_case()
    per_contig = {c: len(_text([ln for ln in lines if ln[0] == c])) for c, _ in SPANS}
    assert min(per_contig.values()) > TILE                      # (no tile holds three contigs: the probe takes the lines, not the queue)
    want, hits = _four_ways(d, prm, tmp_path, lines, keys, seed=41)
    top = {c: s - 1 for c, s in SPANS}
    for (c, p), f in zip(lines, want):
        assert (f != 0) == ((c, p) in set(keys))
        if c in top and p > top[c]:
            assert f == 0                                       # the statement itself: nothing past max_pos is a site
    assert hits == sum(1 for ln in lines if ln in set(keys))


def test_positions_at_and_past_32_bits(d, prm, tmp_path):
    """Lines at 2^32 - 1, 2^32 and 2^32 + p for a listed p, and at 11 digits: none is a site — (uint32_t)pos of 2^32 + p is p."""
    keys = [(b"k", p) for p in (0, 5, 6, 40, 4095)] + [(b"m", p) for p in range(0, 34)]
    lines = [(b"k", p) for p in range(0, 300)] + [(b"k", 4095)]
    lines += [(b"k", (1 << 32) - 1), (b"k", 1 << 32), (b"k", (1 << 32) + 5), (b"k", (1 << 32) + 40), (b"k", 4294967296 + 4095), (b"k", 99999999999),
              (b"k", 10000000005)]
    lines += [(b"m", p) for p in range(0, 300)] + [(b"m", (1 << 32) + 7), (b"m", (1 << 32) - 1)]
    want, hits = _four_ways(d, prm, tmp_path, lines, keys, seed=42)
    assert hits == len(keys) and all(f == 0 for (c, p), f in zip(lines, want) if p > 4095)


# ---- popcount mask and rank ---------------------------------------------------------------------------------------------------------
def test_full_words_single_bits_and_the_rank_directory(d, prm, tmp_path):
    """One contig at bit 0, so a position is its bit: four consecutive words with all 32 bits listed, four with bit 0 alone, four with
    bit 31 alone (the mask (1 << shf) - 1 at shf 0 and 31; a popcount of 32), and positions 262 100 to 262 200 around bit 262 144 =
    word 8 192, where the rank directory's prefix sum passes from its first workgroup to its second."""
    listed = list(range(128, 256)) + [256 + 32 * k for k in range(4)] + [384 + 32 * k + 31 for k in range(4)] + list(range(262100, 262201)) + [7, 600]
    keys = [(b"p", p) for p in listed]
    bit_off, _, _ = _bit_offsets(keys)
    assert bit_off[b"p"] == 0
    lines = [(b"p", p) for p in range(0, 640)] + [(b"p", p) for p in range(262080, 262220)]
    want, hits = _four_ways(d, prm, tmp_path, lines, keys, seed=43)
    assert hits == len(set(listed))


# ---- the register window ------------------------------------------------------------------------------------------------------------
def test_register_window_edges_refills_and_jumps_back(d, prm, tmp_path):
    """The probe's window is 64 words = 2 048 bits from the word of the first lane that missed.  Pairs of lines (A, A + delta) with A
    word-aligned and delta = 2 016 .. 2 080: the last bit inside and the first bit outside both occur; a stretch whose lines jump by more
    than 2 048 each (every lane of a round needs a window of its own); a jump back to the start of the file's positions (wi < win_base:
    rel wraps); the listed position in the bitmap's last word with lines just below and above it (the refill's `inb` edge).  Every
    second line is listed, so a stale window shows as a wrong hit or as a miss."""
    lines, listed = [], []
    a = 0
    for k, delta in enumerate(range(2016, 2081)):               # pairs from word-aligned starts, 8 192 apart
        a = 8192 * (k + 1)
        lines += [(b"w", a), (b"w", a + delta)]
        listed.append(a + delta if k % 2 == 0 else a)
        if k % 3 == 0:
            listed.append(a + 2047)                             # (a neighbour the line is NOT at)
    base = a + 10000
    far = [base + 5000 * k + (k * 37) % 1000 for k in range(200)]                     # > 2 048 apart
    lines += [(b"w", p) for p in far]
    listed += far[::2]
    back = [33 * k for k in range(1, 120)]                      # back to the first words, then up again in small steps
    lines += [(b"w", p) for p in back]
    listed += back[1::2]
    top = far[-1] + 3000                                        # the last listed position: the bitmap's last word but one (the spare)
    lines += [(b"w", p) for p in range(top - 70, top + 70)]
    listed += list(range(top - 70, top + 1, 2)) + [top]
    lines += [(b"w", p) for p in back[:40]]                     # and once more from the far end to the start
    keys = [(b"w", p) for p in sorted(set(listed))]
    want, hits = _four_ways(d, prm, tmp_path, lines, keys, seed=44)
    assert 0.3 < np.count_nonzero(want) / len(want) < 0.7
    assert len(_text(lines)) > 2 * TILE


def test_listed_line_in_the_last_word_of_a_window_that_is_not_refilled(d, prm, tmp_path):
    """A round of the fast parse takes one line from every lane's 64 bytes, and a single lane outside the window starts the refill
    loop, which hands every lane that missed a window of its own.  So the window's last word (rel == 63) is looked up through the
    window itself only in a round ALL of whose lines lie inside one window.  One contig at bit 0, every line within the 2 048
    positions from the word-aligned p0: a third in the first word (p0 .. p0 + 31), a third in the last (p0 + 2016 .. p0 + 2047), a
    third between.  Whichever line a wave starts with, its first line of the first word bases the window at p0's word (the refill
    takes the first missing lane's word, and only lines of the first word lie below any other base), and from then on no line
    misses: the lines of the last word are read at rel == 63, round after round and tile after tile.  Every second position there
    is listed, p0 + 2047 among them; each occurs again in later rounds, and the last line of a key wins."""
    p0 = 4096
    lines = []
    for i in range(720):
        k = i // 3
        lines.append((b"w", (p0 + k % 32, p0 + 2016 + (k * 7) % 32, p0 + 32 + (i * 37) % 1984)[i % 3]))
    listed = [p0 + 2016 + b for b in range(0, 32, 2)] + [p0 + 2047] + [p0 + b for b in range(1, 32, 2)] + [p0 + 32 + 74 * k for k in range(26)]
    keys = [(b"w", p) for p in sorted(set(listed))]
    bit_off, top, _ = _bit_offsets(keys)
    assert bit_off[b"w"] == 0 and p0 % 2048 == 0 and top[b"w"] == p0 + 2047
    assert all(p0 <= p <= p0 + 2047 for _, p in lines) and len(_text(lines)) > 3 * TILE
    last_word = [p for _, p in lines if p >= p0 + 2016]
    assert len(last_word) == 240 and set(last_word) == set(range(p0 + 2016, p0 + 2048))
    want, hits = _four_ways(d, prm, tmp_path, lines, keys, seed=47)
    assert hits >= 120 + 120


# ---- name forms ---------------------------------------------------------------------------------------------------------------------
def test_names_of_1_to_60_bytes(d, prm, tmp_path):
    """Contig names of 1, 16, 17, 40, 44, 45 and 60 bytes, each with sites, in one file: the wave's hint holds a name in one piece
    (up to 16 bytes) or in two (17 to 44), and past 44 bytes its lines go to the queue.  Two of the names share their first 15 bytes, two are a prefix
    pair."""
    names = [b"n", b"q" * 15 + b"A", b"q" * 15 + b"B" + b"x", b"r" * 40, b"s" * 43 + b"1", b"s" * 43 + b"12", b"t" * 60]
    assert [len(n) for n in names] == [1, 16, 17, 40, 44, 45, 60] and names == sorted(names)
    lines, keys = [], []
    for i, n in enumerate(names):
        ps = list(range(90 + i, 90 + i + 260))
        lines += [(n, p) for p in ps]
        keys += [(n, p) for p in ps[i % 2::2]] + [(n, ps[-1])]
        assert len(_text([(n, p) for p in ps])) > TILE
    lines += [(names[1], 95), (names[2], 96), (names[5], 101), (names[4], 100)]      # again at the end: other contigs within one tile
    want, hits = _four_ways(d, prm, tmp_path, lines, keys, seed=45)
    assert hits == sum(1 for ln in lines if ln in set(keys))


# ---- the exact instantiation --------------------------------------------------------------------------------------------------------
def test_exact_pass_at_a_contigs_last_position(d, prm):
    """The look-up of the exact instantiation (k_scan_wave<true, 0>) runs only after the queue has overflowed, so this case has to be
    large: more than 983 040 lines that only the exact parser takes (two blanks after the name), the shortest there are (depth 0).
    Two contigs share bitmap words: `y` lists 0 .. 33, `x` ends one bit before it; lines of x at max_pos - 1, max_pos and the 34 past
    it lie in the middle of the file and again at its end."""
    n = (1 << 20) - 65536 + 3000
    m = 700001                                                  # x's max_pos: x has 700 002 bits, y starts at bit 2 of a word
    rng = random.Random(46)
    listed = sorted(set(rng.sample(range(1, m), 400)) | {m - 1, m, m - 64, 0})
    keys = [(b"x", p) for p in listed] + [(b"y", p) for p in range(0, 34)]
    assert (m + 1) % 32 == 2
    xs = list(range(0, n - 200))
    lines = [(b"x", p) for p in xs] + [(b"y", p) for p in range(0, 100)] + [(b"x", p) for p in range(m - 1, m + 35)] + [(b"y", p) for p in range(20, 84)]
    data = b"".join([b"%s  %d\tA\t0\t*\t*\n" % ln for ln in lines])
    assert len(lines) == n
    flags = _flags_for(keys, 46)
    ss = d.siteset(keys, flags)
    order = ss.key_tuples()
    res = d.call_consensus(ss, data, prm)
    got = d.line_offsets(ss).astype(np.int64)
    starts = lc.line_starts(data)
    last, hits = lc.last_line_of(data, starts, keys)
    want = np.asarray([last[k] for k in order], dtype=np.int64)
    wrong = np.nonzero(got != want)[0]
    assert len(wrong) == 0, [(order[i], int(got[i]), int(want[i])) for i in wrong[:6]]
    assert (res.n_matched, res.n_lines) == (hits, n)
    assert hits == len(listed) + 34 + 2 + 14
