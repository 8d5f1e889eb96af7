"""The walk of the site-calling scan - the exact read-base automaton behind phase B of k_varscan_scan - on every route a candidate
line can take to one of its three copies (varscan_line byte-wise from global memory; varscan_core_lds behind the VS_W_PLAIN shortcut;
varscan_core_lds behind varscan_parse_lds), with the token catalogue of tests/varscan_walk_cases.py under --min-avg-qual 0, 15 and 100:

  i    the ring's strips out of the wave's LDS list (routes A, B) and out of its stretch of the spill (C): every token x both line
       shapes x 16 line addresses mod 16 x 4 lengths of the read-base column mod 4
  ii   rounds 1 to 3 of a group of 64 (D), in one-wave files
  iii  lines of unknown end, byte-wise in the epilogue (F1): ends LF, CR LF, lone CR, the end of the file
  iv   a shared list that is overfilled by at least 100 000 entries: flush() onto the shared list, the epilogue's strips (E), entries
       walked on the spot (G)
  v    deep lines: round 4, the epilogue's strips (E) and the entries behind its 32 KiB (F2)

Every record field and the line count equal oracle/threshold_cases.varscan_records (through varscan_scan_cases.expected); a refusal is
compared by the oracle's byte offset.  That a case takes the route it is named for is shown with the routing statement
(varscan_walk_cases.plan) BEFORE each launch, for this device's CU count; the statement proves reach, never results.  Whether the
cases bite: profiles/r29/varscan_walk_mutants.md.

NOT exercised here:
  * file offsets beyond 2^32 (the upper half of an entry's offset, e.y & 0xFFFF): a pileup of over 4 GiB in device memory and an
    expected result for it do not fit a test of a few seconds; tests/test_gpu_varscan.py's full-size sample is 432 MB.
  * route G per entry: WHICH entries find the shared list full depends on the order in which the waves' atomics arrive.  Family iv
    covers G by count (the waves' attempts exceed the list by a margin asserted before the launch) and pins that no record is lost or
    doubled at the list's end, not that a given token was walked there; the byte-wise automaton G uses is the one family iii pins
    token by token (walk_entry_global -> varscan_line).
  * routes E and F2 per entry in family v: the list's groups of 64 are cut where the waves' atomics fall, so the statement gives
    bounds by count (at least so many in the strips, at least so many behind them), not names.
  * a launch of several pileups whose waves overfill the list (varscan_batch_dev with a saturated list): the batch case here puts
    lines of unknown end of pileups 1 and 2 on the list, which is what reads files[e.y >> 16]."""
import re
import time

import numpy as np
import pytest

from tests import varscan_scan_cases as vc
from tests import varscan_walk_cases as wc

pytestmark = pytest.mark.gpu

FIELDS = ("line_off", "sdp", "dp", "total", "rdf", "rdr", "ref_qual_sum", "adf", "adr", "alt_qual_sum", "ref_base", "alt_base")
SETS = [wc.Q0, wc.Q15, wc.Q100]


@pytest.fixture(scope="module")
def d():
    from tests.gpu_util import get_device
    return get_device()


@pytest.fixture(scope="module")
def n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _prm(kw):
    from snp_pipeline_amd import varscan
    return varscan.Options(vc.options_text(kw)).device_params()


def _got_array(recs):
    """The device's records as an (n, 12) int64 array sorted by line_off, then allele."""
    a = np.stack([recs[f].astype(np.int64) for f in FIELDS], axis=1) if len(recs) else np.zeros((0, 12), dtype=np.int64)
    return a[np.lexsort((a[:, 11], a[:, 0]))]


def _want_array(tuples):
    a = np.array(sorted(tuples), dtype=np.int64).reshape(-1, 12)
    return a[np.lexsort((a[:, 11], a[:, 0]))]


def _same(got, want, what):
    if got.shape != want.shape or not np.array_equal(got, want):
        g, w = {tuple(r) for r in got.tolist()}, {tuple(r) for r in want.tolist()}
        lost, extra = sorted(w - g), sorted(g - w)
        raise AssertionError("%s: %d records for %d, %d lost, %d not expected; the first lost: %r, the first not expected: %r" % (
            what, len(got), len(want), len(lost), len(extra), lost[:1], extra[:1]))


def _compare(name, data, kw, cache, run):
    """run() -> (records, lines) of the device against the oracle's on the same bytes, or against its refusal."""
    from snp_pipeline_amd.device import PileupFormatError
    want = vc.expected(data, kw, cache)
    if want[0] == "error":
        with pytest.raises(PileupFormatError) as err:
            run()
        assert int(re.search(r"at byte (\d+)", str(err.value)).group(1)) == want[1], (name, kw, str(err.value))
        return 0
    recs, n_lines = run()
    _same(_got_array(recs), _want_array(want[0]), "%s %s" % (name, vc.options_text(kw)))
    assert n_lines == want[1], (name, kw, n_lines, want[1])
    return len(recs)


def _on_device(data):
    import torch
    buf = torch.frombuffer(bytearray(b"\0" * 5 + data + b"\0" * 64), dtype=torch.uint8).cuda()
    assert vc.lo_of(buf.data_ptr() + 5) == vc.DEV_LO
    return buf


def _run_dev(d, texts):
    """Every pileup at an address 5 bytes behind an aligned one, under --min-avg-qual 0, 15 and 100."""
    n = 0
    for b in texts:
        buf = _on_device(b.data)
        cache = {}
        for kw in SETS:
            n += _compare(b.name, b.data, kw, cache, lambda: d.varscan_dev(buf.data_ptr() + 5, len(b.data), _prm(kw)))
    return n


def _run_file(d, texts, tmp_path):
    n = 0
    for b in texts:
        path = str(tmp_path / (b.name + ".pileup"))
        with open(path, "wb") as f:
            f.write(b.data)
        cache = {}
        for kw in SETS:
            n += _compare(b.name, b.data, kw, cache, lambda: d.varscan_file(path, _prm(kw)))
    return n


def test_i_ring_from_the_lds_list_and_from_the_stretch(d, n_cu, tmp_path):
    """Routes A, B, C.  Every token x PLAIN / PARSED x the 16 addresses mod 16 of the line's first byte (the LDS word phase of a
    packed line is its address mod 4, its chunk count hangs on the address mod 16) x 4 lengths of the read-base column mod 4 ('$'
    in front: the quality cursor meets every phase against the base cursor).  The fillers are candidates too, so the waves flush;
    one-wave files of at most 60 candidates keep everything in LDS.  Asserted with the statement before the launch: every (token,
    shape) is walked from the ring out of the LDS list and out of the stretch, at every address mod 16 and every pad."""
    t0 = time.time()
    files = wc.family_i()
    counts = wc.check_family_i(files, n_cu)
    n = _run_dev(d, files)
    from_file = wc.family_i(vc.FILE_LO)
    wc.check_family_i(from_file, n_cu)
    n += _run_file(d, from_file, tmp_path)
    print("family i: %d CUs, %d files, %d bytes, %d lines, walked from the ring by (kind, source): %r, %d records, %.1f s" % (
        n_cu, len(files), sum(len(b.data) for b in files), sum(b.n_lines for b in files), sorted(counts.items()), n, time.time() - t0))
    assert n > 6 * 10000


def test_i_as_pileups_one_and_two_of_a_batch(d, n_cu):
    """varscan_batch_dev over three pileups: pileups 1 and 2 are family-i files with a line of unknown end behind them, which goes
    over the shared list, where k_varscan_finish looks its pileup up as files[e.y >> 16]."""
    files = wc.family_i()
    long_lines = wc.family_iii()[0][0]
    tail = long_lines.chunks[0] + long_lines.chunks[2]           # two lines of over 8 200 bytes
    datas = [wc.family_ii()[0].data, files[0].data + tail, files[-1].data + tail]
    for data in datas[1:]:
        off = len(data) - len(tail)
        n_tiles, runs = vc.dealing(len(data), vc.DEV_LO, n_cu)
        assert vc.locate(off, off + len(long_lines.chunks[0]) - 1, vc.DEV_LO, runs).long_
    bufs = [_on_device(x) for x in datas]
    caches = [{} for _ in datas]
    for kw in SETS:
        got = d.varscan_batch_dev([b.data_ptr() + 5 for b in bufs], [len(x) for x in datas], _prm(kw))
        for i, data in enumerate(datas):
            assert not isinstance(got[i], Exception), got[i]
            _compare("batch pileup %d" % i, data, kw, caches[i], lambda: got[i])


def test_ii_rounds_one_to_three_of_a_group(d, n_cu, tmp_path):
    """Route D.  One-wave files of 40 candidate lines of about 600 bytes, a token at the head of each line's read bases and another
    at their end, every line with counts of its own: the statement shows 18 or so entries in each of rounds 1 and 2 and the rest in
    round 3 (round 4 needs more than a one-wave file holds: family v)."""
    files = wc.family_ii()
    counts = wc.check_family_ii(files, n_cu)
    n = _run_dev(d, files)
    from_file = wc.family_ii(vc.FILE_LO)
    wc.check_family_ii(from_file, n_cu)
    n += _run_file(d, from_file, tmp_path)
    print("family ii: %d files, entries by (kind, round): %r, %d records" % (len(files), sorted(counts.items()), n))
    assert n >= 6 * 4 * 40


def test_iii_lines_of_unknown_end(d, n_cu, tmp_path):
    """Route F1.  Lines of 8 200 to 9 000 bytes and one of 40 000, tokens in the first and in the last 64 bytes of the read bases;
    ends LF, CR LF, lone CR, the end of the file; one behind a lone-CR line in an earlier tile of the same wave.  VS_W_LONG for each
    is asserted with locate() before the launch."""
    t0 = time.time()
    files = wc.family_iii()
    n_long = wc.check_family_iii(files, n_cu)
    n = _run_dev(d, [b for b, _ in files])
    from_file = wc.family_iii(vc.FILE_LO)
    wc.check_family_iii(from_file, n_cu)
    n += _run_file(d, [b for b, _ in from_file], tmp_path)
    print("family iii: %d lines of unknown end in %d files, %d records, %.1f s" % (n_long, len(files), n, time.time() - t0))
    assert n >= 6 * n_long


def test_refusals_of_both_parsers(d, n_cu):
    """A malformed line in the ring (varscan_parse_lds) and a malformed line of unknown end (varscan_line): refused at the oracle's
    byte offset, the earlier of the two where a file holds both."""
    good = wc.family_i()[-1]
    long_good = wc.family_iii()[0][0].chunks[0]
    bad_short = vc.probe(b"c", 9, b"AC", b"8", b"GGG...gg", b"EEEEEEEE") + b"\n"
    cols = long_good.split(b"\t")
    bad_long = b"\t".join(cols[:3] + [b"+" + cols[3]] + cols[4:])                     # a depth that is no plain integer
    for name, data in (("ring", good.data + bad_short + good.data), ("long", good.data + long_good + bad_long + good.data),
                       ("both", good.data + bad_long + bad_short)):
        want = vc.expected(data, wc.Q15, {})
        assert want[0] == "error" and want[1] == len(good.data) + (len(long_good) if name == "long" else 0)
        buf = _on_device(data)
        _compare(name, data, wc.Q15, {}, lambda: d.varscan_dev(buf.data_ptr() + 5, len(data), _prm(wc.Q15)))


def _repeat_on_device(block, reps):
    """The block `reps` times from 5 bytes behind an aligned device address on; no host copy of the pileup exists."""
    import torch
    blk = torch.frombuffer(bytearray(block), dtype=torch.uint8).cuda()
    n = reps * len(block)
    buf = torch.empty(5 + n + 64, dtype=torch.uint8, device="cuda")
    buf[5:5 + n].view(reps, len(block)).copy_(blk.unsqueeze(0).expand(reps, len(block)))
    buf[:5] = 0
    buf[5 + n:] = 0
    torch.cuda.synchronize()
    assert vc.lo_of(buf.data_ptr() + 5) == vc.DEV_LO
    return buf


def _replicated(block, reps, kw):
    """The oracle's records on one block, repeated by arithmetic: (n, 12) int64 in (line_off, allele) order."""
    recs, n_lines = vc.expected(block, kw, {})
    one = _want_array(recs)
    out = np.tile(one, (reps, 1))
    out[:, 0] += np.repeat(np.arange(reps, dtype=np.int64) * len(block), len(one))
    return out, n_lines * reps


def test_iv_a_shared_list_that_is_overfilled(d, n_cu):
    """Routes E and G and the branch of flush() that writes the shared list.  A pileup built in device memory from one block (its
    length no multiple of 16) in which a third of the lines are callable catalogue lines of at most 40 bytes in both shapes and the
    rest `c 1 A 0 * *` (depth 0: a candidate that calls nothing), so every line is a candidate.  Sized with dealing() and the cap
    formula for this device's CU count so that the entries the waves try to put on the shared list exceed shared_cap by at least
    100 000, asserted before the launch.  Which entries are walked on the spot depends on the order of the waves' atomics: G is
    covered by count, not per token.  What the comparison pins: no record is lost or doubled at cand_cap (an off-by-one there would
    write cand[shared_cap], the first entry of wave 0's stretch), and every line is counted once."""
    block, reps, nbytes, waves, attempts, shared_cap, lines, callable_ = wc.family_iv_plan(n_cu)
    assert attempts >= shared_cap + 100000 and len(block) % 16 != 0 and 4 * len(callable_) >= len(lines)
    buf = _repeat_on_device(block, reps)
    for kw in (wc.Q15, wc.Q0):
        want, want_lines = _replicated(block, reps, kw)
        t0 = time.time()
        recs, n_lines = d.varscan_dev(buf.data_ptr() + 5, nbytes, _prm(kw), capacity=len(want) + 64)
        t1 = time.time()
        print("family iv %s: %d CUs, %d waves, %d bytes, %d lines, shared_cap %d, at least %d entries tried on the shared list (%d over), %d records, %.2f s" % (
            vc.options_text(kw), n_cu, waves, nbytes, want_lines, shared_cap, attempts, attempts - shared_cap, len(want), t1 - t0))
        _same(_got_array(recs), want, "family iv %r" % (kw,))
        assert n_lines == want_lines == reps * len(lines)


def test_v_deep_lines_round_four_and_the_epilogue(d, n_cu):
    """Round 4, route E with known-end entries, route F2.  Built in device memory from a block of 64 distinct PLAIN lines of about
    2.5 KB (depth about 1 200, a token at the head and another at the tail) and the same 64 in the PARSED shape, sized so that the
    shortest run of the launch's waves has 16 tiles.  Four such lines fit a round of the ring, so of a wave's group of up to 64
    candidates sixteen are walked in rounds 1 to 4 and the rest go to the shared list, where a group of 64 packs about a dozen into
    the epilogue's 32 KiB and leaves the others behind them (bounds by count: the list's order hangs on the waves' atomics).
    Asserted with the statement for every wave before the launch."""
    t0 = time.time()
    block, blines, reps, nbytes, plans = wc.family_v_plan(n_cu)
    counts = wc.check_family_v(plans, nbytes, vc.DEV_LO, n_cu, blines)
    t1 = time.time()
    buf = _repeat_on_device(block, reps)
    for kw in SETS:
        want, want_lines = _replicated(block, reps, kw)
        recs, n_lines = d.varscan_dev(buf.data_ptr() + 5, nbytes, _prm(kw), capacity=len(want) + 64)
        _same(_got_array(recs), want, "family v %r" % (kw,))
        assert n_lines == want_lines == 128 * reps
    print("family v: %d CUs, %d bytes, routes %r; the statement %.1f s, all %.1f s" % (n_cu, nbytes, sorted(counts.items()), t1 - t0, time.time() - t0))
