"""The one-window round of k_scan_wave (csrc/scan.hip, the `fast_round` branch of the lane-per-line parse) over every name length
L and digit count g: the files of tests/scan_parse_cases.py through the two instantiations a host buffer reaches,

  counts    call_consensus(want_counts=True): k_scan_wave<false, 0>;
  depth     call_consensus(want_depth_sum=True): k_scan_wave<false, 4>, the same loop compiled a second time with the depth column
            (five depth digits send a line to the exact parser there and nowhere else),

held exactly against scan_parse_cases.expectation — the oracle's reader (po.parse_record, CPython's int()) line by line: the last
line of every listed key (Device.line_offsets), n_matched, n_lines and po.depth_sum; where the reader ends with an exception, its
class (PileupFormatError.reference_exception) and the byte offset of the line (the status word, as Device.raise_first_error
reads it).  No expectation is taken from a device result.  Once per group gpu_util.check_against_oracle ties in bases and counts.

Why the files look as they do.  A host buffer of at most 16 MiB is one streamed chunk whose waves are dealt at least 8 tiles each
(stream.hip, run_stream: snpgpu_scan_deal(ctx, &e, 1, c == nc ? 1 : 8)), so a file of at most 15 tiles (61 440 bytes) is the run
of ONE wave from tile 0: its first round is general and calibrates g and the top digits, every later round is a one-window round
until a line fails it, and four failing rounds in a row make the next 64 general.  So each case is its own file of 4 to 15
tiles of short lines (a tile takes two or more rounds), with the line it is about far from the first tile and alone among
well-behaved neighbours.  The SHARPNESS of the cases rests on that dealing rule — under another one more lines would take the
general round, which is checked by the same assertions and is right more easily; their CORRECTNESS does not: every expectation is
a statement about the bytes of the file alone.  (The device-pointer entry points deal one tile per wave below 16 MiB and are not
used here.)  profiles/r15/scan_parse_mutants.md lists the value-only mutants of scan.hip these cases were shown to catch."""
import re

import numpy as np
import pytest

from oracle import pileup_oracle as po
from snp_pipeline_amd import _lib as L
from snp_pipeline_amd import device as dev
from tests import scan_parse_cases as sp
from tests.gpu_util import check_against_oracle, get_device

pytestmark = pytest.mark.gpu

P = po.CallerParams(0, 0.6, 1, 0, 0.0)
ROUTES = (("counts", {"want_counts": True}), ("depth", {"want_depth_sum": True}))


@pytest.fixture(scope="module")
def d():
    return get_device()


@pytest.fixture(scope="module")
def prm():
    return dev.make_params(P.min_base_quality, P.min_cons_freq, P.min_cons_depth, P.min_cons_strand_depth, P.min_cons_strand_bias)


def _siteset(d, keys):
    return d.siteset(keys, [L.SITE_IN_SNPLIST] * len(keys))


def _run(d, prm, data, keys, what, ss=None, exp=None):
    """One file through both routes against its expectation; returns the expectation."""
    exp = exp or sp.expectation(data, keys)
    ss = ss or _siteset(d, keys)
    order = ss.key_tuples()
    assert sorted(order) == sorted(set(keys))
    for route, kw in ROUTES:
        if exp.error is not None:
            cls, off = exp.error
            with pytest.raises(dev.PileupFormatError) as caught:
                d.call_consensus(ss, data, prm, **kw)
            err = caught.value
            assert err.reference_exception is cls, (what, route, str(err), exp.error)
            if hasattr(err, "scan_code"):                       # (a line no Record can be built from names its site, not its offset)
                assert int(re.search(r"at byte offset (\d+)", str(err)).group(1)) == off, (what, route, str(err), exp.error)
            continue
        res = d.call_consensus(ss, data, prm, **kw)
        got = d.line_offsets(ss).astype(np.int64)
        want = np.asarray([exp.last[k] for k in order], dtype=np.int64)
        wrong = np.nonzero(got != want)[0]
        assert len(wrong) == 0, (what, route, [(order[i], int(got[i]), int(want[i])) for i in wrong[:6]])
        assert (res.n_matched, res.n_lines) == (exp.hits, exp.n_lines), (what, route)
        if route == "depth":
            assert res.depth_sum == exp.depth_sum, (what, route)
    return exp


def _oracle_too(d, data, keys):
    check_against_oracle(d, data, keys[::2], keys[1::3], P)


# ---- A: the lattice -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", sp.LATTICE_G)
def test_every_name_length_with_g_digits(d, prm, g):
    """Cells (L, g), L = 1 .. 46, one file each: one-window rounds with the '\\n' in the masks (L + g <= 21), with the byte before the
    line read on its own (22), in two pieces (23 .. 38), general rounds only (39 and more), the queue (L >= 45, g = 11).  The
    position column has exactly g bytes; from five digits on the values pass 9 998 .. 10 003 at least twice a file."""
    for L_ in sp.LATTICE_L:
        data, keys = sp.lattice_case(L_, g)
        exp = _run(d, prm, data, keys, (L_, g))
        assert exp.error is None
        if L_ == 9:
            _oracle_too(d, data, keys)


# ---- B: near-miss names -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L_,g", sp.DECOY_CELLS)
def test_a_name_that_differs_in_one_byte(d, prm, L_, g):
    """For every index k of decoy_indices: three lines (tiles 2, 4, 6) of a name that differs from the file's contig in byte k alone,
    at a position that is listed for the contig.  A compare that misses byte k makes such a line the last of that key.  Then the
    same file with the decoy's name in the set: its lines are at its own sites."""
    for k in sp.decoy_indices(L_, g):
        data, keys, decoys = sp.decoy_case(L_, g, k)
        exp = _run(d, prm, data, keys, (L_, g, k))
        assert all(0 < exp.last[key] < off + 1 for off, key in decoys)
        data, keys2, decoys = sp.decoy_case(L_, g, k, own_keys=True)
        exp2 = _run(d, prm, data, keys2, (L_, g, k, "own"))
        assert exp2.hits == exp.hits + 3
    _oracle_too(d, data, keys2)


# ---- C: near-miss top digits --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g,i", sp.top_digit_cases())
def test_a_position_that_differs_in_one_top_digit(d, prm, g, i):
    """Inside a long run of one set of top digits, two lines whose digit i is 1 where the neighbours' is 0; what a compare without
    that digit would make of them — the run's top digits with their last four — is a listed position with a real line earlier."""
    data, keys, odd = sp.top_digit_case(g, i)
    exp = _run(d, prm, data, keys, (g, i))
    assert all(0 < exp.last[key] < off + 1 for off, key in odd)
    if i == 0:
        _oracle_too(d, data, keys)


# ---- D: every byte in a digit place -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("from_end", (1, 2, 3, 4))
@pytest.mark.parametrize("L_,g", sp.DIGIT_CELLS)
def test_every_byte_in_one_of_the_last_four_digit_places(d, prm, L_, g, from_end):
    """Bytes 0x00 .. 0x7F, one changed line per file, in the file's last tile.  The oracle says what the line is: most bytes make it a
    ValueError at that line's offset; a digit, '_' between digits and '+' in front another position; TAB and blank two fields more;
    '\\n' and '\\r' two lines."""
    ss, outcomes = None, set()
    for byte in range(128):
        data, keys, off = sp.digit_byte_case(L_, g, g - from_end, byte)
        ss = ss or _siteset(d, keys)
        exp = _run(d, prm, data, keys, (L_, g, from_end, byte), ss=ss)
        outcomes.add(exp.error and exp.error[0])
    assert ValueError in outcomes and None in outcomes
    if from_end == 1:
        _oracle_too(d, sp.join(sp.digit_base(L_, g)[0]), keys)


@pytest.mark.parametrize("L_,g", ((20, 10), (8, 7), (8, 3), (8, 2), (8, 1)))
def test_odd_bytes_in_the_top_digit_places_and_in_short_columns(d, prm, L_, g):
    """/ : + - _ @ P p ` 0x01 0x1F ! 0x7F TAB blank \\v \\f \\r at every top-digit place of ten and seven digits (the places the masks hold as
    constants), and at every place of one, two and three digits (the places `dmk4` cuts the digit dword down to)."""
    ss = None
    for place in (range(g - 4) if g > 4 else range(g)):
        for byte in sp.ODD_BYTES:
            data, keys, off = sp.digit_byte_case(L_, g, place, byte)
            ss = ss or _siteset(d, keys)
            _run(d, prm, data, keys, (L_, g, place, byte), ss=ss)


# ---- E: starts that are none, and odd starts ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("L_,g", sp.START_CELLS)
def test_starts_that_are_none_and_odd_starts(d, prm, L_, g):
    """L + g = 21, 22, 23 — the byte before the line is in the masks, is read on its own, is read on its own with the name in two pieces.
    '\\v' and '\\f' inside a last column, followed by what reads like a listed line: no line there.  A lone '\\r' before a listed line: a
    line.  The cell's file with CR LF ends.  Lines with blank-TAB, TAB-blank and two TABs after the name and after the position:
    the same keys as with TABs."""
    for ch in (b"\v", b"\f"):
        data, keys, fakes = sp.false_start_case(L_, g, ch)
        exp = _run(d, prm, data, keys, (L_, g, ch))
        assert all(0 < exp.last[key] < off + 1 for off, key in fakes)
    data, keys, after = sp.lone_cr_case(L_, g)
    exp = _run(d, prm, data, keys, (L_, g, "lone CR"))
    assert all(off + 1 in exp.last.values() for off in after)
    data, keys = sp.crlf_case(L_, g)
    _run(d, prm, data, keys, (L_, g, "CR LF"))
    data, keys, odd = sp.odd_separator_case(L_, g)
    exp = _run(d, prm, data, keys, (L_, g, "separators"))
    assert all(exp.last[key] == off + 1 for off, key in odd)
    _oracle_too(d, data, keys)


# ---- F: seams, deterministically ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L_,g", sp.SEAM_CELLS)
def test_a_listed_line_0_to_72_bytes_before_a_tile_end(d, prm, L_, g):
    """For every j in 0 .. 72 a listed line that starts exactly j bytes before a tile end (13 tile ends a file): its
    `name TAB digits TAB` lies in the tile, across the seam or wholly in the halo."""
    for js in sp.seam_groups():
        data, keys, seams = sp.seam_case(L_, g, js)
        exp = _run(d, prm, data, keys, (L_, g, js))
        assert exp.error is None and len(seams) == len(js)
    _oracle_too(d, data, keys)


def test_a_name_that_runs_past_the_halo(d, prm):
    """An unlisted name of 130 bytes that starts one byte before a tile end: it ends past the 128-byte halo, where TileView::get goes
    to global memory.  The lines around it are listed."""
    data, keys, seams = sp.seam_case(9, 4, (), long_name=b"Z" * 130)
    exp = _run(d, prm, data, keys, "130 bytes")
    assert exp.error is None and seams[0][0] == sp.TILE - 1


# ---- G: ten digits for real ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L_", sp.WIDE_CELLS)
def test_ten_digit_values_past_32_bits(d, prm, L_):
    """Runs of true ten-digit positions: through 4 294 960 000 (the first top digits whose positions do not all fit 32 bits); through
    2^32 under those same top digits, 429 496 — the lines before 2^32 are what a layout could be calibrated from, and 429 496 * 10 000
    plus the last four digits of 2^32 + n is n in 32 bits, a listed position; and 4 294 970 000 + n, whose 32-bit remainder 2704 + n is
    listed too.  None of them is a site."""
    data, keys = sp.wide_case(L_, large=False)
    exp = _run(d, prm, data, keys, (L_, "wide"))
    assert exp.hits == len(keys) == 210


@pytest.mark.parametrize("L_", sp.WIDE_CELLS)
def test_ten_digit_values_that_are_listed(d, prm, L_):
    """The same file with 4 294 959 999, 4 294 960 000 and 4 294 967 295 listed (a bitmap of 2^32 bits): those three lines are sites,
    4 294 967 296 and the lines past it are none."""
    data, keys = sp.wide_case(L_, large=True)
    exp = _run(d, prm, data, keys, (L_, "wide, listed"))
    assert exp.hits == 213 and all(exp.last[(sp.cell_name(L_), v)] for v in (4294959999, 4294960000, 4294967295))
