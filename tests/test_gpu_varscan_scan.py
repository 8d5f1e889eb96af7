"""The line filter of the site-calling scan (phase B of k_varscan_scan) at every line geometry: the families of
tests/varscan_scan_cases.py through Device.varscan_dev at an odd device address (and Device.varscan_file), every record field and
the line count against oracle/threshold_cases.varscan_records.  A line the filter takes for plain and unable to call is dropped
without a trace, so every probe here is TIGHT: exactly min_reads2 letters in its read bases, at the two ends of the interval the
filter counts them in (or one byte inside them), depth equal to min_coverage, letters all around the interval.  That each case
reaches the branch it is named for is shown on the CPU (tests/test_varscan_scan_cpu.py); whether the cases bite, with mutants of
the kernel (profiles/r27/varscan_scan_mutants.md)."""
import re
import time

import pytest

from oracle import varscan_oracle as vo
from tests import varscan_scan_cases as vc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def d():
    from tests.gpu_util import get_device
    return get_device()


def _prm(kw):
    from snp_pipeline_amd import varscan
    return varscan.Options(vc.options_text(kw)).device_params()


def _compare(b, kw, run):
    """run() -> (records, lines) of the device; the oracle's on the same bytes, or its refusal."""
    from snp_pipeline_amd.device import PileupFormatError
    want = vc.expected(b.data, kw, b.__dict__.setdefault("cache", {}))
    if want[0] == "error":
        with pytest.raises(PileupFormatError) as err:
            run()
        assert int(re.search(r"at byte (\d+)", str(err.value)).group(1)) == want[1], (b.name, kw, str(err.value))
        return 0
    recs, n_lines = run()
    got = vc.rec_tuples(recs)
    if got != want[0]:
        lost, extra = sorted(set(want[0]) - set(got)), sorted(set(got) - set(want[0]))
        at = {p.off: p for p in b.probes}
        raise AssertionError("%s %r: %d records lost, %d not expected; the first lost: %r (%r), the first not expected: %r" % (
            b.name, kw, len(lost), len(extra), lost[:1], at[lost[0][0]].expect if lost and lost[0][0] in at else None, extra[:1]))
    assert n_lines == want[1] == b.n_lines, (b.name, kw, n_lines, want[1], b.n_lines)
    return len(got)


def _run_dev(d, files):
    """Every file at an address 5 bytes behind an aligned one, under each of its parameter sets."""
    import torch
    n = 0
    for b in files:
        buf = torch.frombuffer(bytearray(b"\0" * 5 + b.data + b"\0" * 64), dtype=torch.uint8).cuda()
        assert vc.lo_of(buf.data_ptr() + 5) == b.lo == vc.DEV_LO
        for kw in b.params():
            prm = _prm(kw)
            n += _compare(b, kw, lambda: d.varscan_dev(buf.data_ptr() + 5, len(b.data), prm))
        # every probe is called under its own parameter set: nothing of the file is tight for nothing
        cache = b.__dict__["cache"]
        if cache["bad"] is None:
            called = {vc.pkey(kw): {r[0] for r in vc.expected(b.data, kw, cache)[0]} for kw in b.params()}
            for p in b.probes:
                assert not p.expect.get("tight", True) or p.off in called[vc.pkey(p.prm)], (b.name, p.off, p.expect)
    return n


def test_a_head_geometry(d):
    """Name length 1..60 x position digits 1..10 x depth digits 1..4: the fourth TAB at every offset 7..78, so inside the 32-bit
    window, inside the 64-bit one (31 / 32), on its last bit (63) and behind it (64: the walk calls the line); short names around a
    long one; lines of 11..64 bytes."""
    t0 = time.time()
    files = vc.family_a()
    n = _run_dev(d, files)
    print("family A: %d files, %d probes, %d records, %.1f s" % (len(files), sum(len(b.probes) for b in files), n, time.time() - t0))
    assert n > 5000


@pytest.mark.parametrize("eol", [vc.LF, vc.CRLF, vc.CR], ids=["lf", "crlf", "cr"])
def test_b_where_the_line_starts(d, eol):
    """The first byte at every offset 0..127 of a tile and 70 before to 6 behind a tile edge inside a wave's run (odd and even
    tile index), in front of a wave's first tile and of the file's last; r3 = 63 at 4032 / 4033 / 4034 / 4095 / 0; the fourth TAB
    on the first byte of a tile whose ring slot still says TAB one byte earlier.  CR LF and lone CR: family E."""
    t0 = time.time()
    files = vc.family_b(eol)
    n = _run_dev(d, files)
    print("family B %r: %d files, %d probes, %d records, %.1f s" % (eol, len(files), sum(len(b.probes) for b in files), n, time.time() - t0))
    assert n >= sum(len(b.probes) for b in files)


@pytest.mark.parametrize("eol", [vc.LF, vc.CRLF, vc.CR], ids=["lf", "crlf", "cr"])
def test_c_ends_of_the_letter_interval(d, eol, tmp_path):
    """b0 % 32 and t4 % 32 at 0, 1, 30, 31; b0 and t4 in one word, in neighbouring words, in different tiles and ring slots; the
    fifth TAB and the terminator (CR LF: the CR) on the last byte of a tile; one byte of read bases; none.  Also from a file."""
    files = vc.family_c(eol)
    n = _run_dev(d, files)
    assert n >= len(files[0].probes) - 2
    for b in vc.family_c(eol, lo=vc.FILE_LO):
        path = str(tmp_path / "c.pileup")
        with open(path, "wb") as f:
            f.write(b.data)
        for kw in b.params():
            prm = _prm(kw)
            _compare(b, kw, lambda: d.varscan_file(path, prm))


def test_d_lines_for_the_walk(d, tmp_path):
    """Next to tight probes: qualities one short / one long, a sixth TAB, further columns, depth 0 / 00012 / 012 / 12345 (records
    as the oracle's), depth +12, a two-byte reference, an empty name (refused at the oracle's offset)."""
    files = vc.family_d()
    assert _run_dev(d, files) > 1000
    b = vc.family_d(lo=vc.FILE_LO)[1]
    path = str(tmp_path / "d.pileup")
    with open(path, "wb") as f:
        f.write(b.data)
    _compare(b, vc.D2, lambda: d.varscan_file(path, _prm(vc.D2)))


def test_f_long_carried_lines(d):
    """Tight probes of 4 000 .. 8 200 bytes across a tile edge; the terminator on the last byte of the next tile and one later."""
    assert _run_dev(d, vc.family_f()) >= 8


def test_g_running_counts_past_65536(d):
    """The running TAB and letter counts of a wave are kept modulo 2^16.  A pileup built in device memory from one 14-byte
    filler line (5 TABs, 5 letters: plain, cannot call) in which every wave's run passes 65 536 of both: a wave's share is at least
    66 / cum(waves) of the tiles (dealing()), 48 tiles hold 70 217 of each, so the file has ceil(48 * cum(waves) / 66) tiles - for
    256 CUs 227 887 tiles, 933 MB.  Tight probes overwrite fillers in every k-th wave's run, placed with the dealing statement so that
    the letters before b0 are 65 534 or 65 535 (the interval [b0, t4) straddles the wrap), or the TABs before the line 65 531 ..
    65 535 ([p0, le) straddles it), or neither; at least eight of each kind, asserted before the launch.  Expected: the oracle on the
    probe lines; the fillers are inert (test_varscan_scan_cpu.py); the line count by arithmetic.  No host copy of the file exists."""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    lo = vc.DEV_LO
    fl, nbytes, n_tiles, runs, probes, kinds = vc.family_g_plan(n_cu, lo)
    assert kinds["letters"] >= 8 and kinds["tabs"] >= 8 and kinds["neither"] >= 8, kinds
    # the pileup, in device memory only
    block = torch.frombuffer(bytearray(fl * 2048), dtype=torch.uint8).cuda()
    buf = torch.empty(5 + nbytes + 64, dtype=torch.uint8, device="cuda")
    n_blocks = nbytes // len(block)
    buf[5:5 + n_blocks * len(block)].view(n_blocks, len(block)).copy_(block.unsqueeze(0).expand(n_blocks, len(block)))
    rest = nbytes - n_blocks * len(block)
    buf[5 + n_blocks * len(block):5 + nbytes] = block[:rest]
    buf[5 + nbytes:] = 0
    n_lines = nbytes // 14
    want_recs = []
    for o, line in probes:
        buf[5 + o:5 + o + len(line) + 1] = torch.frombuffer(bytearray(line + b"\n"), dtype=torch.uint8).cuda()
        n_lines -= (len(line) + 1) // 14 - 1
        recs, one = vc.expected(line + b"\n", vc.cov(12), {})
        assert one == 1 and len(recs) == 1
        want_recs.append((o,) + recs[0][1:])
    torch.cuda.synchronize()
    assert vc.lo_of(buf.data_ptr() + 5) == lo
    t0 = time.time()
    recs, got_lines = d.varscan_dev(buf.data_ptr() + 5, nbytes, _prm(vc.cov(12)))
    print("family G: %d CUs, %d waves, %d tiles, %d bytes, %d probes, straddling %r, %.2f s" % (n_cu, len(runs), n_tiles, nbytes, len(probes), kinds, time.time() - t0))
    assert vc.rec_tuples(recs) == sorted(want_recs)
    assert got_lines == n_lines
    recs, got_lines = d.varscan_dev(buf.data_ptr() + 5, nbytes, _prm(vo.PIPELINE_DEFAULTS))      # nothing passes min_reads2 5
    assert len(recs) == 0 and got_lines == n_lines
