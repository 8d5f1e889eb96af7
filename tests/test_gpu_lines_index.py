"""k_lines_index<false/true> (csrc/scan.hip: count per 16 KiB block, prefix sum, emit of 1 + offset per line) and k_lines_flags
through call_all_lines / call_all_lines_compact, against the statements of tests/lines_cases.py at the places where the index can
go wrong: a terminator at a 16-byte load, 64-byte thread and 16 KiB block edge, '\\r' | '\\n' split by an edge (the '\\n' is byte 0 of
the next thread or block and is seen through the one extra byte `pc`), a lone '\\r' as a block's last byte, files that end on an edge,
blank lines whose two terminators straddle an edge, an output capacity one short, and more lines than k_lines_flags' capped grid
takes in one turn.

The alignment shift.  k_lines_index carries a `shift` path (p0 < 0) for buffers that are not 16-byte aligned.  Its only callers are
snpgpu_enqueue_lines_count / _emit / _offsets.  `grep snpgpu_enqueue_lines_ csrc/` finds three calls of them (_count twice, _emit
once), all in the body of all_lines_pass (csrc/stream.hip), and none of _offsets.  all_lines_pass hands them the buffer load_file
gave it, unchanged: load_raw returns the pool's slot 0 and load_bgzf its slot 1, both straight from hipMalloc (pool_ensure), whose
allocations are aligned to 256 bytes at the least.  No entry point of the library passes an offset into a slot, so none can produce
shift != 0: the path is dead code today, it cannot be run through an entry point that exists, and it is left alone (a caller that
ever indexes a pileup inside a larger buffer needs these edge cases again at shifts 1, 8 and 15)."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

from oracle import pileup_oracle as po
from snp_pipeline_amd import _lib as L
from snp_pipeline_amd import device as dev
from tests import lines_cases as lc
from tests.gpu_util import check_record, get_device

pytestmark = pytest.mark.gpu

P = po.CallerParams(0, 0.6, 1, 0, 0.0)
BLOCK = 16384
EDGES = (16, 64, BLOCK, 2 * BLOCK)
FLAG_VALUES = (L.SITE_IN_SNPLIST, L.SITE_IN_SNPLIST | L.SITE_EXCLUDED, L.SITE_EXCLUDED)
MARK = 0xA5


@pytest.fixture(scope="module")
def d():
    return get_device()


@pytest.fixture(scope="module")
def prm():
    return dev.make_params(P.min_base_quality, P.min_cons_freq, P.min_cons_depth, P.min_cons_strand_depth, P.min_cons_strand_bias)


def _write(tmp_path, data, name="reads.all.pileup"):
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(data)
    return path


def _raw_all_lines(d, ss, path, prm, capacity):
    """snpgpu_call_all_lines_file as it is, into arrays filled with MARK: (rc, n_lines, offsets + 1, flags, records, status), nothing
    cut to n_lines and nothing raised — a file with a blank line comes back with E_PILEUP and everything written."""
    cap = int(capacity)
    off = np.full(max(cap, 1), MARK * 0x0101010101010101, dtype=np.uint64)
    flags = np.full(max(cap, 1), MARK, dtype=np.uint8)
    counts = np.frombuffer(bytes([MARK]) * (dev.COUNTS_DTYPE.itemsize * max(cap, 1)), dtype=dev.COUNTS_DTYPE).copy()
    status = np.zeros(L.SCAN_STATUS_WORDS, dtype=np.uint64)
    n_lines = C.c_uint64(MARK)
    as_ptr = lambda a: a.ctypes.data_as(C.c_void_p)                  # noqa: E731
    rc = d.lib.snpgpu_call_all_lines_file(d.ctx, ss.handle, os.fsencode(path), C.byref(prm), cap, C.byref(n_lines), as_ptr(off), as_ptr(flags),
                                          as_ptr(counts), as_ptr(status))
    return int(rc), int(n_lines.value), off, flags, counts, status


def _check_line_record(c, rec, flag, where):
    """check_record for a line of the all-lines pass: a line at an excluded position fails the Region filter on top of the caller's
    own (call_consensus.py:165-168), and no other line does."""
    assert bool(int(c["filters"]) & po.F_REGION) == bool(int(flag) & L.SITE_EXCLUDED), where
    plain = c.copy()
    plain["filters"] = int(c["filters"]) & ~po.F_REGION
    check_record(plain, rec, P, where)


def _site_set(d, data, starts, seed, blank_ok=False):
    """Every third line's (name, position) with a seeded irregular flag, and a few keys no line has."""
    rng = random.Random(seed)
    keys = []
    for i, ln in enumerate(lc.lines_of(data, starts)):
        key = lc.name_and_position(ln, blank_ok)
        if key is not None and i % 3 == 1 and 0 <= key[1] < (1 << 32):
            keys.append(key)
    keys = sorted(set(keys)) + [(b"ctg", 3_000_000), (b"zzz", 1)]
    flags = [rng.choice(FLAG_VALUES) for _ in keys]
    return keys, flags, d.siteset(keys, flags)


def _check_file(d, prm, tmp_path, data, seed=0, malformed_at=None, sample=40, records=True, compact=True):
    """One file through the all-lines pass: the offsets are line_starts + 1 element by element, the flags line_flags', full records
    po.parse_record's on a sample of lines (the first and last ones and those around every edge among them).  malformed_at: the
    offset of the first blank line — the library then answers E_PILEUP with that offset in status[0], and still writes everything."""
    starts = lc.line_starts(data)
    n = len(starts)
    keys, flags, ss = _site_set(d, data, starts, seed, blank_ok=malformed_at is not None)
    path = _write(tmp_path, data)
    rc, n_lines, off, fl, counts, status = _raw_all_lines(d, ss, path, prm, n + 3)
    assert n_lines == n and int(status[1]) == n
    assert np.array_equal(off[:n].astype(np.int64), starts + 1), np.nonzero(off[:n].astype(np.int64) != starts + 1)[0][:5]
    assert (off[n:] == MARK * 0x0101010101010101).all() and (fl[n:] == MARK).all()      # nothing past the lines
    want_flags = lc.line_flags(data, starts, keys, flags, blank_ok=malformed_at is not None)
    assert np.array_equal(fl[:n], want_flags), np.nonzero(fl[:n] != want_flags)[0][:5]
    if malformed_at is None:
        assert rc == 0 and int(status[0]) == 0xFFFFFFFFFFFFFFFF
    else:
        assert rc == L.E_PILEUP and int(status[0]) == ((malformed_at + 1) << 8 | 1)
    if records:
        lines = lc.lines_of(data, starts)
        near = []                                               # per edge: the line that holds it, six before and six behind
        for e in EDGES:
            at = int(np.searchsorted(starts, e, side="right")) - 1
            near += list(range(max(0, at - 6), min(n, at + 7)))
        rng = random.Random(seed)
        for i in sorted(set(list(range(min(n, 4))) + list(range(max(0, n - 4), n)) + near + rng.sample(range(n), min(n, sample)))):
            if lines[i].split():
                _check_line_record(counts[i], po.parse_record(lines[i].split(), P.min_base_quality), want_flags[i], (i, int(starts[i])))
    if compact and malformed_at is None:
        off2, recs, widx, wide = d.call_all_lines_compact(ss, path, prm, capacity=n)
        assert np.array_equal(off2.astype(np.int64), starts + 1) and np.array_equal(recs["site_flags"], want_flags)
        fl2, counts2 = dev.expand_line_records(recs, widx, wide)
        assert np.array_equal(fl2, want_flags) and counts2.tobytes() == counts[:n].tobytes()
    return starts, want_flags


# ---- a terminator on an edge --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [-2, -1, 0, 1])
@pytest.mark.parametrize("kind", ["lf", "crlf", "cr", "cr_crlf"])
def test_terminator_at_load_thread_and_block_edges(d, prm, tmp_path, kind, delta):
    """The terminator's first byte at E + delta for E = 16 (load), 64 (thread span), 16 384 and 32 768 (block), one file per kind
    and delta.  crlf at -1: '\\r' | '\\n' split by the edge, the '\\n' byte 0 of the next thread or block; cr at -1: a lone '\\r' as the
    last byte of a thread or block, a letter behind it; cr_crlf: '\\r' then '\\r\\n' — a blank line between them, so the library answers
    E_PILEUP with that line's offset (malformed input, reported through status[0]) and the offsets are all there."""
    term = {"lf": lc.LF, "crlf": lc.CRLF, "cr": lc.CR, "cr_crlf": b"\r\r\n"}[kind]
    placements = [(e + delta, term) for e in EDGES]
    specs, targets = lc.plan_terminators(placements, name=b"c", end=2 * BLOCK + 700 + delta, seed=7 + delta)
    data, _ = lc.build_pileup(specs, targets, seed=3)
    for e in EDGES:
        assert data[e + delta:e + delta + len(term)] == term
    _check_file(d, prm, tmp_path, data, seed=delta, malformed_at=16 + delta + 1 if kind == "cr_crlf" else None)


# ---- mixed terminators --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2])
def test_mixed_terminators_over_three_blocks(d, prm, tmp_path, seed):
    """'\\n', '\\r\\n' and lone '\\r' mixed by a seeded choice over three blocks; lines of 14 to 300 bytes put several starts into one
    thread's 64 bytes and lines over several threads."""
    rng = random.Random(seed)
    specs, targets, at = [], {}, 0
    while at < 3 * BLOCK + 100:
        w = rng.choice((14, 14, 15, 16, 17, 30)) if rng.random() < 0.5 else rng.randrange(14, 301)
        term = rng.choice((lc.LF, lc.CRLF, lc.CR))
        specs.append((b"c", 1 + len(specs), term))
        targets[len(specs) - 1] = at + w
        at += w + len(term)
    data, starts = lc.build_pileup(specs, targets, seed=seed)
    assert len(data) > 3 * BLOCK and np.array_equal(lc.line_starts(data), starts)
    per_thread = np.bincount(starts // 64)
    assert per_thread.max() >= 3 and (np.diff(starts) > 128).any()
    _check_file(d, prm, tmp_path, data, seed=seed)


# ---- file ends ----------------------------------------------------------------------------------------------------------------------
SIZES = [BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK - 1, 2 * BLOCK, 2 * BLOCK + 1, 64, 13]


@pytest.mark.parametrize("last", ["none", "lf", "cr", "crlf"])
def test_file_ends_at_and_around_block_edges(d, prm, tmp_path, last):
    """The last line unterminated, or ending in '\\n', '\\r' or '\\r\\n', in files of 16384 k - 1, 16384 k and 16384 k + 1 bytes
    (k = 1, 2), of 64 bytes exactly and of 13: crlf at 16384 k + 1 leaves the '\\n' alone in the last block, which holds no start; a
    terminator as the file's last byte starts no line behind it."""
    term = {"none": b"", "lf": lc.LF, "cr": lc.CR, "crlf": lc.CRLF}[last]
    for size in SIZES:
        specs, targets = lc.plan_terminators([], name=b"c", end=size, last_term=term, seed=size)
        data, starts = lc.build_pileup(specs, targets, seed=5)
        assert len(data) == size and (data.endswith(term) if term else data[-1] not in (10, 13))
        got, _ = _check_file(d, prm, tmp_path, data, seed=size, sample=6, compact=size in (BLOCK + 1, 13))
        assert np.array_equal(got, starts)


def test_empty_file_has_no_lines(d, prm, tmp_path):
    path = _write(tmp_path, b"")
    ss = d.siteset([(b"c", 1)], [1])
    off, flags, counts = d.call_all_lines(ss, path, prm)
    assert len(off) == len(flags) == len(counts) == 0
    off2, recs, widx, wide = d.call_all_lines_compact(ss, path, prm)
    assert len(off2) == len(recs) == len(widx) == len(wide) == 0
    rc, n_lines, off, fl, _, status = _raw_all_lines(d, ss, path, prm, 4)
    assert (rc, n_lines, int(status[1])) == (0, 0, 0) and (off == MARK * 0x0101010101010101).all() and (fl == MARK).all()


# ---- bytes that look like line ends -------------------------------------------------------------------------------------------------
def test_vt_ff_and_fs_inside_the_read_columns_start_no_line(d, prm, tmp_path):
    """'\\v', '\\f' and 0x1c in the read-base or quality column — also as the byte before a terminator of each kind, and as the last
    byte of a thread's 64 and of a block — are not line starts.  (str.split() of the reference cuts such a line's columns there, so
    only the offsets and the flags of those lines are held against the statement; the records of the untouched lines are checked.)"""
    rng = random.Random(9)
    specs, targets, at = [], {}, 0
    while at < 2 * BLOCK + 300:
        w = rng.randrange(40, 120)
        term = rng.choice((lc.LF, lc.CRLF, lc.CR))
        specs.append((b"c", 1 + len(specs), term))
        targets[len(specs) - 1] = at + w
        at += w + len(term)
    data, starts = lc.build_pileup(specs, targets, seed=9)
    text = bytearray(data)
    bounds = starts.tolist() + [len(data)]
    touched = set()

    def column_of(i, off):                                      # which TAB-separated column of line i holds the byte at off
        return bytes(text[bounds[i]:off]).count(b"\t")

    odd = (0x0B, 0x0C, 0x1C)
    for i in range(0, len(specs), 4):                           # the byte before the terminator (a quality) and one base
        end = bounds[i + 1] - len(specs[i][2])
        text[end - 1] = odd[(i // 4) % 3]
        mid = bounds[i] + bytes(text[bounds[i]:end]).rindex(b"\t") - 2
        if column_of(i, mid) == 4:
            text[mid] = odd[(i // 4 + 1) % 3]
        touched.add(i)
    for off in [63, 127, BLOCK - 1, BLOCK, 2 * BLOCK - 1, 2 * BLOCK]:      # the last byte of a thread / a block, the first of the next
        i = int(np.searchsorted(starts, off, side="right")) - 1
        if column_of(i, off) >= 4 and text[off] not in (10, 13):
            text[off] = odd[off % 3]
            touched.add(i)
    data2 = bytes(text)
    assert len(touched) > 90 and all(data2.count(bytes([c])) > 20 for c in odd)
    assert np.array_equal(lc.line_starts(data2), starts)        # the statement: nothing new starts
    keys, flags, ss = _site_set(d, data2, starts, 9)
    path = _write(tmp_path, data2)
    rc, n_lines, off, fl, counts, status = _raw_all_lines(d, ss, path, prm, len(starts))
    assert rc == 0 and n_lines == len(starts)
    assert np.array_equal(off.astype(np.int64), starts + 1)
    want_flags = lc.line_flags(data2, starts, keys, flags)
    assert np.array_equal(fl, want_flags)
    lines = lc.lines_of(data2, starts)
    for i in [i for i in range(len(starts)) if i not in touched][:60]:
        _check_line_record(counts[i], po.parse_record(lines[i].split(), 0), want_flags[i], i)


# ---- blank lines --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edge", [64, 4 * 64, BLOCK, 2 * BLOCK])
@pytest.mark.parametrize("pair", [b"\n\n", b"\r\r", b"\n\r\n"])
def test_blank_line_whose_terminators_straddle_an_edge(d, prm, tmp_path, pair, edge):
    """Two terminators around a thread or block edge: the first one's (last) byte is the last byte before the edge, the blank line is
    the terminator at the edge itself.  The reference's --vcfAllPos reader raises IndexError (a Record cannot be built from []); the
    library reports the line in status[0] — malformed input, not a fault — and the offset it names is the statement's."""
    specs, targets = lc.plan_terminators([(edge - 1, pair)], name=b"c", end=edge + 900, seed=edge)
    data, _ = lc.build_pileup(specs, targets, seed=1)
    assert data[edge - 1:edge - 1 + len(pair)] == pair
    starts = lc.line_starts(data)
    blank = [int(s) for s, ln in zip(starts, lc.lines_of(data, starts)) if not ln.split()]
    assert blank == [edge]
    _check_file(d, prm, tmp_path, data, seed=edge, malformed_at=edge, sample=8)
    keys, flags, ss = _site_set(d, data, starts, edge, blank_ok=True)
    path = _write(tmp_path, data)
    for check in (True, False):
        with pytest.raises(dev.PileupFormatError) as info:
            d.call_all_lines(ss, path, prm, check=check)
        assert int(re.search(r"byte offset (\d+)", str(info.value)).group(1)) == edge
        if check:
            assert info.value.reference_exception is IndexError
    with pytest.raises(dev.PileupFormatError) as info:
        d.call_all_lines_compact(ss, path, prm)
    assert int(re.search(r"byte offset (\d+)", str(info.value)).group(1)) == edge
    with pytest.raises(IndexError):
        po.parse_record(b"".split(), 0)


def test_blank_line_class_through_the_file_to_file_writer(d, prm, tmp_path):
    """The same through snpgpu_write_all_positions_vcf, as tests/test_gpu_all_positions.py asks of its malformed lines: IndexError for
    the reader that builds a Record from every line, nothing written; the reader with a position set (only_listed) fails to unpack
    two values there: ValueError."""
    import argparse

    from snp_pipeline_amd import vcf_writer
    specs, targets = lc.plan_terminators([(BLOCK - 1, b"\n\n")], name=b"c", end=BLOCK + 500)
    data, _ = lc.build_pileup(specs, targets)
    path, out = _write(tmp_path, data), str(tmp_path / "out.vcf")
    ss = d.siteset([(b"c", 7)], [L.SITE_IN_SNPLIST])
    args = argparse.Namespace(minBaseQual=0, minConsFreq=0.6, minConsDpth=1, minConsStrdDpth=0, minConsStrdBias=0.0, vcfRefName="ref.fasta",
                              vcfPreserveRefCase=False, vcfFailedSnpGt=".")
    for only_listed, exc in ((False, IndexError), (True, ValueError)):
        with pytest.raises(dev.PileupFormatError) as info:
            vcf_writer.write_all_positions_vcf_from_pileup(d, ss, out, "s", args, path, prm, only_listed=only_listed, check=not only_listed)
        assert info.value.reference_exception is exc and "byte offset %d" % BLOCK in str(info.value)
        assert not os.path.exists(out)


# ---- capacity -----------------------------------------------------------------------------------------------------------------------
def test_capacity_one_short_writes_nothing(d, prm, tmp_path):
    """snpgpu_call_all_lines_file with room for n_lines - 1: OK, *out_n_lines == n_lines, the output arrays untouched; with room for
    n_lines everything comes back."""
    specs, targets = lc.plan_terminators([(BLOCK - 1, lc.CRLF)], name=b"c", end=BLOCK + 2000)
    data, starts = lc.build_pileup(specs, targets)
    n = len(starts)
    keys, flags, ss = _site_set(d, data, starts, 4)
    path = _write(tmp_path, data)
    rc, n_lines, off, fl, counts, status = _raw_all_lines(d, ss, path, prm, n - 1)
    assert (rc, n_lines, int(status[1])) == (0, n, n)
    assert (off == MARK * 0x0101010101010101).all() and (fl == MARK).all() and set(counts.tobytes()) == {MARK}
    rc, n_lines, off, fl, counts, status = _raw_all_lines(d, ss, path, prm, n)
    assert (rc, n_lines) == (0, n)
    assert np.array_equal(off.astype(np.int64), starts + 1) and np.array_equal(fl, lc.line_flags(data, starts, keys, flags))
    assert (counts["status"] == L.ST_OK).all()


# ---- the second turn of k_lines_flags -----------------------------------------------------------------------------------------------
def test_second_turn_of_the_flags_grid(d, prm, tmp_path):
    """k_lines_flags runs on min(ceil(n_lines / 256), 8 * n_cu) workgroups of 256 lanes, a line per lane and turn: its second turn
    starts at line 8 * n_cu * 256.  This is the one large case and it cannot be smaller: the cap is a property of the device (256 CUs:
    524 288 lines), so reaching the second turn takes 8 * n_cu * 256 + 257 lines whatever they hold — the shortest well-formed ones
    (depth 0, '*' columns, about 15 bytes: roughly 8 MB), 32 bytes a line back through call_all_lines_compact.  Listed positions with
    the three flag values sit throughout, the last 300 lines included; flags and offsets are compared for ALL lines."""
    import torch
    n_cu = int(torch.cuda.get_device_properties(0).multi_processor_count)
    n = 8 * n_cu * 256 + 257
    data = b"".join([b"c\t%d\tA\t0\t*\t*\n" % p for p in range(1, n + 1)])
    rng = random.Random(31)
    listed = sorted(set(rng.sample(range(1, n + 1), 3000)) | set(range(n - 299, n + 1, 2)) | {8 * n_cu * 256, 8 * n_cu * 256 + 1, 8 * n_cu * 256 + 256})
    keys = [(b"c", p) for p in listed]
    flags = [rng.choice(FLAG_VALUES) for _ in keys]
    ss = d.siteset(keys, flags)
    path = _write(tmp_path, data)
    off, recs, widx, wide = d.call_all_lines_compact(ss, path, prm, capacity=n)
    n_lines = len(off)
    assert n_lines > 8 * n_cu * 256 and n_lines == n
    starts = lc.line_starts(data)
    assert np.array_equal(off.astype(np.int64), starts + 1)
    want = lc.line_flags(data, starts, keys, flags)
    # the case's own shape: every listed position is a flagged line, every second one of the last 300 among them (the seeded sample
    # may add a few more there), and all three flag values occur in the second turn
    assert int(np.count_nonzero(want)) == len(listed) and int(np.count_nonzero(want[-300::2])) == 150
    assert int(np.count_nonzero(want[-300:])) == sum(p > n - 300 for p in listed)
    assert set(np.unique(want[8 * n_cu * 256:])) == {0, *FLAG_VALUES}
    got = recs["site_flags"]
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:5]
    assert len(widx) == 0 and (recs["raw_depth"] == 0).all() and (recs["status"] == L.ST_OK).all()
