"""The statements of tests/lines_cases.py pinned on the CPU: line_starts against bytes.splitlines(keepends=True) and CPython's
universal-newlines reader (zero differences over 20 000 seeded strings), line_flags / last_line_of against the oracle's
call_consensus_sites, and the builders against the offsets their cases ask for."""
import io
import random

import numpy as np
import pytest

from oracle import fuzz
from oracle import pileup_oracle as po
from tests import lines_cases as lc


def _splitlines_starts(data):
    """Cumulative lengths of bytes.splitlines(keepends=True) — restricted to the terminators of a pileup: bytes.splitlines ends a line at
    '\\n', '\\r' and '\\r\\n' only (str.splitlines would also take '\\v', '\\f', 0x1c-0x1e and 0x85)."""
    lens = [len(p) for p in data.splitlines(keepends=True)]
    return np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64) if lens else np.zeros(0, dtype=np.int64)


def _text_reader_lines(data):
    return sum(1 for _ in io.TextIOWrapper(io.BytesIO(data), newline=None, encoding="latin-1"))


def test_line_starts_equal_splitlines_and_the_universal_newlines_reader():
    rng = random.Random(20240)
    fixed = [b"", b"a", b"\n", b"\r", b"\r\n", b"a\n", b"a\r", b"a\r\n", b"\r\r\n", b"\n\r", b"\n\r\n", b"\r\n\r", b"a\vb\fc\x1cd\x1de\x1ef\x85g",
             b"a\v", b"a\f\n", b"\x1c\r", b"\x85\r\n"]
    strings = fixed + [lc.random_text(rng, rng.randrange(0, 31)) for _ in range(20000)]
    differences = 0
    ends_seen = set()
    for s in strings:
        got = lc.line_starts(s)
        differences += not np.array_equal(got, _splitlines_starts(s))
        differences += len(got) != _text_reader_lines(s)
        differences += len(got) > 0 and not (got[0] == 0 and np.all(np.diff(got) > 0) and got[-1] < len(s))
        ends_seen.add(s[-2:] if s.endswith(b"\r\n") else s[-1:])
    assert differences == 0
    assert {b"", b"\n", b"\r", b"\r\n", b"\v", b"\f", b"\x1c", b"\x1d", b"\x1e", b"\x85"} <= ends_seen      # every terminator ends some string


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_flags_and_last_lines_equal_the_oracles_detail(seed):
    """Three fuzzed files of several contigs, some lines repeated further down and some keys without a line: the keys hit and the
    last line of each are those of po.call_consensus_sites' detail (which keeps the record of the LAST line of a key)."""
    rng = random.Random(seed)
    data, _, sites = fuzz.synth_pileup(seed, genome_len=300, contigs=("chrA", "chrA1", "b", "zz_%d" % seed), n_sites=40)
    lines = data.split(b"\n")[:-1]
    again = [rng.choice(lines) for _ in range(60)]                       # repeated positions, unsorted
    for i, ln in enumerate(again):                                        # ... with other reads, so that the last line shows
        f = ln.split(b"\t")
        f[3:] = [b"%d" % (i % 7 + 1), b"G" * (i % 7 + 1), b"I" * (i % 7 + 1)]
        again[i] = b"\t".join(f)
    data = b"\n".join(lines + again) + b"\n"
    keys = sites + [(b"chrA", 100000 + seed), (b"absent", 5)]
    flags = [rng.choice((1, 2, 3)) for _ in keys]
    starts = lc.line_starts(data)
    assert len(starts) == len(lines) + len(again)
    p = po.CallerParams(0, 0.6, 1, 0, 0.0)
    _, detail = po.call_consensus_sites(data, keys, set(), p)
    last, hits = lc.last_line_of(data, starts, keys)
    assert {k for k, v in last.items() if v} == set(detail)
    assert hits == sum(1 for _ in po.scan_sites(data, set(keys), 0)) > len(detail)       # (some key has two lines)
    by_start = dict(zip((int(s) for s in starts), lc.lines_of(data, starts)))
    for key, (rec, _, _) in detail.items():
        assert po.parse_record(by_start[last[key] - 1].split(), 0) == rec, key
    fl = lc.line_flags(data, starts, keys, flags)
    want = dict(zip(keys, flags))
    for s, f, ln in zip(starts, fl, lc.lines_of(data, starts)):
        r = po.parse_record(ln.split(), 0)
        assert int(f) == want.get((r.chrom, r.position), 0)
    assert set(np.unique(fl)) == {0, 1, 2, 3}


def test_positions_as_int_takes_them():
    data = b"c\t007\tA\t0\t*\t*\nc\t+7\tA\t0\t*\t*\nc\t1_0\tA\t0\t*\t*\nc  7\tA\t0\t*\t*\n\n"
    starts = lc.line_starts(data)
    assert [lc.name_and_position(ln, blank_ok=True) for ln in lc.lines_of(data, starts)] == [(b"c", 7), (b"c", 7), (b"c", 10), (b"c", 7), None]
    assert lc.line_flags(data, starts, [(b"c", 7), (b"c", 10)], [2, 3], blank_ok=True).tolist() == [2, 2, 3, 2, 0]
    with pytest.raises(IndexError):                                      # a Record cannot be built from []
        lc.line_flags(data, starts, [(b"c", 7)], [1])


def test_builders_put_every_terminator_where_the_case_asks():
    for width in list(range(11, 40)) + [63, 64, 65, 299, 300, 1000, 1001, 1002, 1003]:
        for pos in (1, 9, 10, 12345):
            if width >= lc.min_width(b"c", pos):
                ln = lc.pileup_line(b"c", pos, width)
                assert len(ln) == width
                rec = po.parse_record(ln.split(), 0)
                assert (rec.chrom, rec.position) == (b"c", pos) and rec.raw_depth == len(ln.split()[4]) - (ln.split()[4] == b"*")
    with pytest.raises(ValueError):
        lc.pileup_line(b"c", 1, 10)
    for term in (lc.LF, lc.CRLF, lc.CR, b"\r\r\n"):
        for delta in (-2, -1, 0, 1):
            placements = [(e + delta, term) for e in (16, 64, 16384, 32768)]
            specs, targets = lc.plan_terminators(placements, name=b"c", end=40000, seed=delta)
            data, starts = lc.build_pileup(specs, targets)
            assert len(data) == 40000
            for off, t in placements:
                assert data[off:off + len(t)] == t and data[off - 1] not in (10, 13)
            got = lc.line_starts(data)
            assert set(starts.tolist()) <= set(got.tolist())
            assert len(got) == len(starts) + (4 if term == b"\r\r\n" else 0)              # ('\r' then '\r\n': a blank line between them)
    for last in (lc.LF, lc.CR, lc.CRLF, b""):
        specs, targets = lc.plan_terminators([], end=16384 + 1, last_term=last)
        data, starts = lc.build_pileup(specs, targets)
        assert len(data) == 16385 and (data.endswith(last) if last else data[-1] not in (10, 13))
        assert np.array_equal(lc.line_starts(data), starts)
