"""The per-line records of call_consensus --vcfAllPos at the edges no fuzzed pileup reaches: symbols with 65 535 / 65 536 reads
(the 16-bit counts of the packed record, csrc/lines_out.hip fits_u16) — through the call kernels first, whose records must be what
the oracle's parse_record counts —, and wide lines at the workgroup edges of k_compact_lines / k_gather_wide (256 lines a
workgroup)."""
import numpy as np
import pytest

from oracle import fuzz
from oracle import pileup_oracle as po
from oracle import threshold_cases as tc
from snp_pipeline_amd import _lib as L
from snp_pipeline_amd import device as dev
from tests.gpu_util import check_record as _check_record

pytestmark = pytest.mark.gpu

A, C, G = 0x41, 0x43, 0x47
P = po.CallerParams(tc.MIN_BASE_QUAL, 0.6, 3, 0, 0.0)

# (counts {symbol: (forward, reverse)}, reads below the quality threshold)
DEEP = [({A: (65535, 0)}, 0),
        ({A: (65536, 0)}, 0),
        ({A: (32768, 32767)}, 0),
        ({A: (32768, 32768)}, 0),
        ({A: (65535, 0), C: (0, 65535), G: (1, 1)}, 0),
        ({A: (65536, 0), C: (1, 0)}, 0),
        ({A: (65535, 0)}, 5000)]                  # raw depth above 16 bits, the counts fit


def _lowered(counts, by):
    """The large counts of a case `by` lower (the small ones stay)."""
    return {s: tuple(k - by if k > 100 else k for k in fr) for s, fr in counts.items()}


def _deep_cases():
    return [(_lowered(c, by), low) for by in (0, 3, 4) for c, low in DEEP]


def _is_wide(rec):
    """A line is wide exactly when some total, forward or reverse count is above 65 535 or it has more than three symbols (the lines
    of these tests are well-formed, with a one-byte reference base and a depth of 32 bits)."""
    ranked = rec.most_common_good_bases or []
    big = any(max(rec.base_good_depth[s], rec.forward_base_good_depth.get(s, 0), rec.reverse_base_good_depth.get(s, 0)) > 65535 for s in ranked)
    return big or len(ranked) > dev.LINE_SYMS


@pytest.fixture(scope="module")
def d():
    from tests.gpu_util import get_device
    return get_device()


@pytest.fixture(scope="module")
def deep_file(tmp_path_factory):
    """A pileup of short fuzzed lines with the deep lines of _deep_cases spliced in (every 19th line: both line classes share a
    launch), and the oracle's Record of every line.  Built once for the module: a deep line is 140 to 270 KB."""
    data, _, sites = fuzz.synth_pileup(77, genome_len=420, n_sites=30)
    lines = data.split(b"\n")[:-1]
    cases = _deep_cases()
    assert len(cases) == 21 and len(lines) > 19 * len(cases)
    deep_at = {}
    for k, (counts, low) in enumerate(cases):
        i = 19 * k + 5
        chrom, pos = lines[i].split(b"\t")[:2]
        lines[i] = tc.consensus_line(chrom, int(pos), b"A" if k % 2 == 0 else b"t", counts, low=low, seed=k)
        deep_at[i] = k
    data = b"\n".join(lines) + b"\n"
    records = [po.parse_record(ln.split(), P.min_base_quality) for ln in lines]
    for i, k in deep_at.items():                                           # the builder gave the counts the case asks for
        counts, low = cases[k]
        assert records[i].base_good_depth == {s: f + r for s, (f, r) in counts.items()}
        assert records[i].raw_depth == sum(f + r for f, r in counts.values()) + low
    path = str(tmp_path_factory.mktemp("deep") / "reads.all.pileup")
    with open(path, "wb") as f:
        f.write(data)
    return path, lines, records, deep_at, sites


def test_deep_lines_full_records_equal_the_oracles(d, deep_file):
    """Symbols with up to 131 072 reads on one line through the call kernels: totals, forward and reverse counts per symbol, good
    and raw depth are the oracle's — no counter of 16 bits anywhere on the way."""
    path, lines, records, deep_at, sites = deep_file
    ss = d.siteset(sites, [L.SITE_IN_SNPLIST] * len(sites))
    prm = dev.make_params(P.min_base_quality, P.min_cons_freq, P.min_cons_depth, P.min_cons_strand_depth, P.min_cons_strand_bias)
    off, flags, counts = d.call_all_lines(ss, path, prm)
    assert len(counts) == len(lines) == len(records)
    starts = np.concatenate([[0], np.cumsum([len(ln) + 1 for ln in lines])[:-1]])
    assert np.array_equal(off, starts + 1)
    listed = {(c, p) for c, p in sites}
    for i, (c, rec) in enumerate(zip(counts, records)):
        _check_record(c, rec, P, (i, deep_at.get(i)))
        assert bool(flags[i]) == ((rec.chrom, rec.position) in listed), i
    passes = d.call_pass_counts()
    assert passes["wave"] >= len(deep_at) and sum(passes[k] for k in ("lanes128", "lanes256", "lanes512")) > 0      # both classes, one launch


def test_deep_lines_packed_or_wide_at_the_16_bit_edge(d, deep_file):
    """k_compact_lines on those records: a line is wide exactly when a count is above 65 535 (or it has more than three symbols);
    the packed records are device.pack_line_records' and expand to the full ones."""
    path, lines, records, deep_at, sites = deep_file
    ss = d.siteset(sites, [L.SITE_IN_SNPLIST] * len(sites))
    prm = dev.make_params(P.min_base_quality, P.min_cons_freq, P.min_cons_depth, P.min_cons_strand_depth, P.min_cons_strand_bias)
    off, flags, counts = d.call_all_lines(ss, path, prm)
    want_wide = [i for i, rec in enumerate(records) if _is_wide(rec)]
    by_case = {k: i in want_wide for i, k in deep_at.items()}
    assert [by_case[k] for k in range(7)] == [False, True, False, True, False, True, False]      # the cases at the edge itself
    assert not any(by_case[k] for k in range(7, 21))                                              # 3 and 4 below it: everything fits
    for wcap in (1, len(want_wide)):
        off2, recs, widx, wide = d.call_all_lines_compact(ss, path, prm, wide_capacity=wcap)
        assert np.array_equal(off2, off)
        assert widx.tolist() == want_wide
        assert (recs["n_symbols"] == dev.LINE_WIDE).nonzero()[0].tolist() == want_wide
        assert wide.tobytes() == counts[want_wide].tobytes()
        recs_np, widx_np, wide_np = dev.pack_line_records(counts, flags)
        assert widx_np.tolist() == want_wide and recs.tobytes() == recs_np.tobytes()
        flags2, counts2 = dev.expand_line_records(recs, widx, wide)
        assert np.array_equal(flags2, flags) and counts2.tobytes() == counts.tobytes()
    # the packed 16-bit counts themselves, against the oracle: 65 535 is held exactly
    for i, k in deep_at.items():
        if i in want_wide:
            continue
        rec = records[i]
        for r, sym in enumerate(rec.most_common_good_bases):
            assert (int(recs["sym"][i][r]), int(recs["total"][i][r]), int(recs["fwd"][i][r]), int(recs["rev"][i][r])) == \
                (sym, rec.base_good_depth[sym], rec.forward_base_good_depth.get(sym, 0), rec.reverse_base_good_depth.get(sym, 0)), (k, r)
        assert int(recs["raw_depth"][i]) == rec.raw_depth and int(recs["n_symbols"][i]) == len(rec.most_common_good_bases)


# ---- wide lines at the workgroup edges ------------------------------------------------------------------------------------------
def _short_file(n_lines, wide_at):
    """n_lines short lines of one to three symbols; those at the indices of wide_at have four."""
    out = []
    for i in range(n_lines):
        nf, nr, ng = 1 + i % 7, (i // 7) % 5, (i // 3) % 3
        bases = b"CcGgTt.,"[:8 - i % 2] if i in wide_at else b"." * nf + b"," * nr + b"G" * ng + b"t" * (i % 2)
        out.append(b"ctg\t%d\tA\t%d\t%s\t%s" % (i + 1, len(bases), bases, b"I" * len(bases)))
    return b"\n".join(out) + b"\n"


BLOCK_CASES = [(1, "edges"), (255, "edges"), (256, "edges"), (257, "edges"), (511, "edges"), (513, "edges"), (513, "none"), (257, "all")]


@pytest.mark.parametrize("n_lines, which", BLOCK_CASES)
def test_wide_lines_at_workgroup_edges(d, tmp_path, n_lines, which):
    """k_compact_lines counts the wide lines per workgroup of 256, k_gather_wide places them behind the scan of those counts: wide
    lines at line 0, 255, 256 and the last one, none at all, every line; with room for one wide line (the wrapper asks again) and
    for exactly as many as there are."""
    wide_at = {"edges": sorted({i for i in (0, 255, 256, n_lines - 1) if i < n_lines}), "none": [], "all": list(range(n_lines))}[which]
    data = _short_file(n_lines, set(wide_at))
    path = str(tmp_path / "reads.all.pileup")
    with open(path, "wb") as f:
        f.write(data)
    listed = [(b"ctg", p) for p in range(1, n_lines + 1, 3)]
    ss = d.siteset(listed, [L.SITE_IN_SNPLIST] * len(listed))
    prm = dev.make_params(0, 0.6, 1, 0, 0.0)
    off, flags, counts = d.call_all_lines(ss, path, prm)
    assert len(counts) == n_lines
    records = [po.parse_record(ln.split(), 0) for ln in data.split(b"\n")[:-1]]
    for i, (c, rec) in enumerate(zip(counts, records)):
        _check_record(c, rec, po.CallerParams(0, 0.6, 1, 0, 0.0), i)
    assert [i for i, rec in enumerate(records) if _is_wide(rec)] == wide_at
    assert flags.astype(bool).tolist() == [i % 3 == 0 for i in range(n_lines)]
    for wcap in (1, len(wide_at)):
        off2, recs, widx, wide = d.call_all_lines_compact(ss, path, prm, capacity=n_lines, wide_capacity=wcap)
        assert np.array_equal(off2, off) and len(recs) == n_lines
        assert widx.tolist() == wide_at and (len(widx) < 2 or np.all(np.diff(widx.astype(np.int64)) > 0))
        assert wide.tobytes() == counts[wide_at].tobytes()
        recs_np, widx_np, _ = dev.pack_line_records(counts, flags)
        assert widx_np.tolist() == wide_at and recs.tobytes() == recs_np.tobytes()
        flags2, counts2 = dev.expand_line_records(recs, widx, wide)
        assert np.array_equal(flags2, flags) and counts2.tobytes() == counts.tobytes()
