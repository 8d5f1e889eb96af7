"""The builders of tests/scan_parse_cases.py hit the edges they name, and their expectations come out of the oracle.  Every builder
asserts its own geometry while it builds, so running it is the first check; on top of that each near-miss is shown to matter: a
reader that ignored the one byte the case is about (the decoy's name byte, the top digit, the '\\v' that is no line end) would
report another last line for a listed key.  No device, no library code."""
import re

import pytest

from oracle import pileup_oracle as po
from tests import lines_cases as lc
from tests import scan_parse_cases as sp


def _same_as_oracle(data, keys):
    """expectation() against lc.last_line_of / po.depth_sum where the reader gets through, and against po.scan_sites — the keys it
    yields, the exception it ends with — always."""
    exp = sp.expectation(data, keys)
    seen, raised = [], None
    try:
        for rec in po.scan_sites(data, set(keys), 0):
            seen.append((rec.chrom, rec.position))
    except (ValueError, IndexError) as e:
        raised = type(e)
    if exp.error is None:
        assert raised is None and len(seen) == exp.hits
        assert {k for k, v in exp.last.items() if v} == set(seen)
        assert exp.depth_sum == po.depth_sum(data) and exp.n_lines == len(lc.line_starts(data))
    else:
        assert raised is exp.error[0]
        off = exp.error[1]
        assert off in set(map(int, lc.line_starts(data)))
        before = sp.expectation(data[:off], keys)               # the reader gets through everything in front of that line
        assert before.error is None and before.hits == len(seen)
    return exp


def _same_as_lines_cases(data, keys, exp):
    last, hits = lc.last_line_of(data, lc.line_starts(data), keys)
    assert (last, hits) == (exp.last, exp.hits)


def test_expectation_is_the_oracles_reader():
    data = b"c\t5\tA\t2\t.,\tII\nc\t007\tC\t0\t*\t*\nc\t+5\tA\t1\t.\tI\nd\t5\tA\t10000\t.\tI\rc\t1_0\tG\t1\tg\tI\r\nc\t7\tA\t3\t.\tI"
    keys = [(b"c", 5), (b"c", 7), (b"c", 10), (b"c", 11)]
    exp = _same_as_oracle(data, keys)
    _same_as_lines_cases(data, keys, exp)
    assert exp.last == {(b"c", 5): data.index(b"c\t+5") + 1,(b"c", 7): data.rindex(b"c\t7") + 1, (b"c", 10): data.index(b"c\t1_0") + 1, (b"c", 11): 0}
    assert (exp.hits, exp.n_lines, exp.depth_sum) == (5, 6, 2 + 0 + 1 + 10000 + 1 + 3)
    for bad, cls in ((b"c\t5:\tA\t1\t.\tI\n", ValueError), (b"c\n", ValueError), (b"c\t5\n", IndexError), (b"c\t5\tA\tx\n", ValueError), (b"c\t7\tA\t2\t.,\n", IndexError)):
        exp = _same_as_oracle(data + b"\n" + bad + data, keys)
        assert exp.error == (cls, len(data) + 1)
    assert sp.expectation(data + b"\nc\t9\tA\tx\n", keys).error is None      # (not listed: no Record is built)
    fs = b"c\t1\x1c5\tA\t1\t.\tI\n"                                          # 0x1c separates fields: position 1, reference base 5, depth A
    assert _same_as_oracle(fs, [(b"c", 1)]).error == (ValueError, 0) and _same_as_oracle(fs, [(b"c", 15)]).error is None


# ---- A ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", sp.LATTICE_G)
def test_lattice_cells(g):
    for L in sp.LATTICE_L:
        data, keys = sp.lattice_case(L, g)
        exp = sp.expectation(data, keys)
        assert exp.error is None and exp.hits >= 50 and all(exp.last.values())
        first = data[:data.index(b"\n")].split(b"\t")
        assert (len(first[0]), len(first[1])) == (L, g)
        if L in (1, 22, 46):
            _same_as_lines_cases(data, keys, _same_as_oracle(data, keys))
    assert len({sp.cell_name(L) for L in sp.LATTICE_L}) == 46


def test_lattice_covers_every_form_of_the_round():
    cells = [(L, g) for L in sp.LATTICE_L for g in sp.LATTICE_G]
    assert len(cells) == 506
    one_window = [c for c in cells if c[0] <= 44 and c[1] <= 10 and sum(c) <= 38]
    assert {sum(c) for c in one_window} >= set(range(2, 39))
    assert any(sum(c) == 22 for c in one_window) and any(sum(c) == 38 and c[1] == g for c in one_window for g in range(1, 11))
    assert [c for c in cells if c[0] >= 45 or c[1] == 11] and [c for c in cells if sum(c) >= 39 and c[0] <= 44 and c[1] <= 10]


# ---- B ------------------------------------------------------------------------------------------------------------------------------
def test_decoy_cells_and_indices():
    assert {L + g for L, g in sp.DECOY_CELLS} == set(sp.DECOY_SUMS)
    assert {(16, 5), (16, 6), (16, 7), (17, 4), (17, 5), (17, 6), (28, 10), (33, 5)} <= set(sp.DECOY_CELLS)
    assert sp.decoy_indices(28, 10) == [0, 3, 4, 11, 12, 15, 16, 26, 27]      # (L - 12 - 1 = 15 and L - 12 = 16: where the two pieces meet)
    assert sp.decoy_indices(16, 5) == [0, 3, 4, 11, 12, 14, 15]
    assert {12, 15} <= set(sp.decoy_indices(27, 10)) and 27 - 12 > 12          # bytes 12 .. 14 of that name are in the hint registers alone


@pytest.mark.parametrize("L,g", sp.DECOY_CELLS)
def test_decoy_lines_would_move_a_listed_key(L, g):
    for k in sp.decoy_indices(L, g):
        name, decoy = sp.cell_name(L), sp.decoy_name(sp.cell_name(L), k)
        data, keys, decoys = sp.decoy_case(L, g, k)
        exp = sp.expectation(data, keys)
        assert exp.error is None and len(decoys) == 3
        sloppy = sp.expectation(data.replace(decoy, name), keys)               # a reader that does not look at byte k
        for off, key in decoys:
            assert 0 < exp.last[key] < off + 1 and sloppy.last[key] == off + 1
        assert sloppy.hits == exp.hits + 3
        data2, keys2, _ = sp.decoy_case(L, g, k, own_keys=True)
        own = sp.expectation(data2, keys2)
        assert data2 == data and own.hits == exp.hits + 3 and all(own.last[(decoy, key[1])] == off + 1 for off, key in decoys)
    _same_as_lines_cases(data, keys, _same_as_oracle(data, keys))


# ---- C ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g,i", sp.top_digit_cases())
def test_top_digit_lines_would_move_a_listed_key(g, i):
    data, keys, odd = sp.top_digit_case(g, i)
    exp = _same_as_oracle(data, keys)
    _same_as_lines_cases(data, keys, exp)
    assert len(odd) == 2
    for off, key in odd:
        line = data[off:data.index(b"\n", off)]
        at = off + 6 + 1 + i
        assert data[at] == 0x31 and line.split(b"\t")[1].count(b"1") >= 1
        sloppy = sp.expectation(data[:at] + b"0" + data[at + 1:], keys)
        assert 0 < exp.last[key] < off + 1 == sloppy.last[key]


# ---- D ------------------------------------------------------------------------------------------------------------------------------
def test_every_byte_in_a_digit_place_has_the_oracles_outcome():
    kinds = {}
    for L, g in sp.DIGIT_CELLS:
        for byte in range(128):
            data, keys, off = sp.digit_byte_case(L, g, g - 3, byte)
            exp = sp.expectation(data, keys)
            base = sp.expectation(sp.join(sp.digit_base(L, g)[0]), keys)
            if exp.error is not None:
                kind = exp.error[0].__name__
                assert off <= exp.error[1] <= off + L + g                     # the changed line, or the second line a '\n' or '\r' makes of it
            elif exp.n_lines != base.n_lines:
                kind = "lines"
            else:
                kind = "same" if exp.last == base.last else "moved"
            kinds.setdefault(kind, []).append(byte)
            if byte in (0x00, 0x09, 0x0A, 0x0D, 0x1C, 0x2B, 0x39, 0x3A, 0x5F):
                _same_as_oracle(data, keys)
    assert set(kinds) >= {"ValueError", "moved"}
    assert set(b":/@P`-\x7f\x01\x00") <= set(kinds["ValueError"]) and set(b"0123456789") <= set(kinds["moved"] + kinds.get("same", []))
    assert ord("_") in kinds["moved"] + kinds.get("same", [])                 # 1_00 is a position
    # '+' in front of the digits is a position as well; TAB and blank make two fields of the column: another position
    for byte, place in ((ord("+"), 0), (9, 0), (32, 0), (9, 1), (32, 2)):
        data, keys, off = sp.digit_byte_case(8, 4, place, byte)
        assert sp.expectation(data, keys).error is None
    data, keys, off = sp.digit_byte_case(20, 10, 3, 9)                         # 000<TAB>001234: an unlisted position, two fields more
    assert sp.expectation(data, keys).error is None and sp.expectation(data, keys + [(sp.cell_name(20), 0)]).error[0] is ValueError


def test_digit_byte_cases_of_one_to_three_digits():
    for g in (1, 2, 3):
        for place in range(g):
            for byte in sp.ODD_BYTES:
                data, keys, off = sp.digit_byte_case(8, g, place, byte)
                _same_as_oracle(data, keys)


# ---- E ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,g", sp.START_CELLS)
def test_starts_that_are_none_and_odd_starts(L, g):
    assert L + g in (21, 22, 23)
    for ch in (b"\v", b"\f"):
        data, keys, fakes = sp.false_start_case(L, g, ch)
        exp = _same_as_oracle(data, keys)
        sloppy = sp.expectation(data.replace(ch, b"\n"), keys)                 # a reader that takes the byte for a line end
        assert len(fakes) == 3
        for off, key in fakes:
            assert 0 < exp.last[key] < off + 1 == sloppy.last[key]
    data, keys, after = sp.lone_cr_case(L, g)
    exp = _same_as_oracle(data, keys)
    _same_as_lines_cases(data, keys, exp)
    assert len(after) == 3 and all(off + 1 in exp.last.values() for off in after)
    data, keys = sp.crlf_case(L, g)
    _same_as_lines_cases(data, keys, _same_as_oracle(data, keys))
    data, keys, odd = sp.odd_separator_case(L, g)
    exp = _same_as_oracle(data, keys)
    _same_as_lines_cases(data, keys, exp)
    assert all(exp.last[key] == off + 1 for off, key in odd)
    seps = {re.match(rb"[^\t ]+([\t ]+)\d+([\t ]+)", data[off:off + 64]).groups() for off, key in odd}
    assert len(seps) == 15 and (b"\t", b"\t") not in seps and {len(a + b) for a, b in seps} == {3, 4}


# ---- F ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,g", sp.SEAM_CELLS)
def test_seam_lines_start_where_asked(L, g):
    seen = set()
    for js in sp.seam_groups():
        data, keys, seams = sp.seam_case(L, g, js)
        exp = sp.expectation(data, keys)
        assert exp.error is None
        for (off, key), j in zip(seams, js):
            assert (sp.TILE - off % sp.TILE) % sp.TILE == j and off // sp.TILE + (j > 0) == js.index(j) + 1
            seen.add(j)
            if g >= 4:
                assert exp.last[key] == off + 1                               # (with fewer digits the positions come again later)
    assert seen == set(range(73))
    _same_as_lines_cases(data, keys, _same_as_oracle(data, keys))


def test_a_name_past_the_halo():
    long_name = b"Z" * 130
    data, keys, seams = sp.seam_case(9, 4, (), long_name=long_name)
    (off, _), = seams
    assert off == sp.TILE - 1 and off + 130 > sp.TILE + 128                    # the name's end lies past the 128-byte halo of tile 0
    exp = _same_as_oracle(data, keys)
    assert exp.error is None and not any(k[0] == long_name for k in keys)
    nxt = data.index(b"\n", off) + 1
    assert nxt + 1 in exp.last.values()                                        # the line behind it is listed


# ---- G ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", sp.WIDE_CELLS)
def test_ten_digit_values(L):
    data, keys = sp.wide_case(L, large=False)
    exp = _same_as_oracle(data, keys)
    _same_as_lines_cases(data, keys, exp)
    assert exp.hits == 210 == len(keys) and max(p for _, p in keys) < 3000
    data2, keys2 = sp.wide_case(L, large=True)
    exp2 = sp.expectation(data2, keys2)
    assert data2 == data and exp2.hits == 213 and max(p for _, p in keys2) == (1 << 32) - 1
    name = sp.cell_name(L)
    wrapped = b"".join(b"%s\t%010d" % (name, (sp.WRAP + n) & 0xFFFFFFFF) for n in range(0, 200, 2))
    assert wrapped.count(name) == 100 and all((name, 2704 + n) in exp.last for n in range(0, 200, 2))
    assert L + 10 == 38 or L + 10 <= 21
