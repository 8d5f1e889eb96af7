"""Every call kernel at the rounding edges of its thresholds (oracle/threshold_cases.py): the consensus cases at line lengths
that pick each parser — k_call_lanes<128/256/512>, k_call_sites wave-parallel and serial — in shallow and deep files
(k_call_mode), through every entry point; the VarScan cases in the LDS walk and the global-memory walk, with --min-avg-qual
below and at or above 95."""
import argparse
import random

import numpy as np
import pytest

from oracle import pileup_oracle as po
from oracle import threshold_cases as tc
from oracle import varscan_oracle as vo
from oracle import vcf_oracle as vco
from snp_pipeline_amd import _lib as L
from snp_pipeline_amd import device as dev

pytestmark = pytest.mark.gpu

CHROM = b"chrT"
# (name, shortest line, longest line, longest read-base field): which parser a line of that size reaches
# (the last two take every third case: their shallow files need ~50 short lines per case)
CLASSES = (("lanes128", 1, 128, 64), ("lanes256", 129, 256, 128), ("lanes512", 257, 512, 255), ("wave", 513, 4224, 2048),
           ("serial", 4225, 5000, None))
CASES = tc.consensus_cases()
PARAMS = sorted({p for _, _, p in CASES})
MBQ = tc.MIN_BASE_QUAL


@pytest.fixture(scope="module")
def d():
    from tests.gpu_util import get_device
    return get_device()


def _case_pos(i):
    return 10 * (i + 1)


def _build(cls, deep, seed):
    """One pileup: every case whose counts fit the class, at a length inside it; shallow files put short unlisted lines between
    them (mean line under 100 bytes), deep ones long unlisted lines (over 100)."""
    name, lo, hi, max_bases = cls
    rng = random.Random(seed)
    lines, placed = [], 0
    for i, (_, counts, _) in enumerate(CASES):
        if lo > 512 and i % 3:
            continue
        ref = b"ACGT"[i % 4:i % 4 + 1]
        base = tc.consensus_line(CHROM, _case_pos(i), ref, counts, low=i % 3, seed=i)
        nb = len(po.split_fields(base)[4])
        top = hi if max_bases is None else min(hi, len(base) - nb + max_bases)
        if max(lo, len(base)) > top:
            continue
        length = rng.randint(max(lo, len(base)), top)
        lines.append(tc.consensus_line(CHROM, _case_pos(i), ref, counts, low=i % 3, length=length, seed=seed + i))
        placed += 1
        if deep:
            lines.append(tc.consensus_line(CHROM, _case_pos(i) + 1, b"A", {0x41: (2, 1)}, length=rng.randint(300, 700), seed=i))
        else:
            for k in range(1 + length // 25):
                lines.append(b"%s\t%d\tA\t3\t.,G\tII5" % (CHROM, 2 * (10 ** 7 + len(lines)) + 1))     # (odd: never a case position)
    data = b"\n".join(lines) + b"\n"
    assert (len(data) > 100 * len(lines)) == deep
    return data, placed


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """[(name, bytes, path, {key: Record}, [Record of every line])] for every class and mode; the Records parsed once (the oracle
    is slow on long lines)."""
    tmp = tmp_path_factory.mktemp("thr")
    out = []
    for c, cls in enumerate(CLASSES):
        for deep in (False, True):
            data, placed = _build(cls, deep, 1000 * c + deep)
            path = str(tmp / ("%s_%s.pileup" % (cls[0], "deep" if deep else "shallow")))
            with open(path, "wb") as f:
                f.write(data)
            every = [po.parse_record(po.split_fields(line), MBQ) for _, line in po.iter_lines(data)]
            recs = {(r.chrom, r.position): r for r in every if r.position % 10 == 0}
            assert placed == len(recs) and placed > 0
            out.append((cls[0] + ("_deep" if deep else "_shallow"), data, path, recs, every))
    return out


KEYS = [(CHROM, _case_pos(i)) for i in range(len(CASES))]


def _excluded(shift):
    return {k for j, k in enumerate(KEYS) if (j + shift) % 7 == 0}


def _expect(recs, p, excluded):
    """po.call_consensus_sites for the listed positions, from the Records parsed once: (bases, filter masks) in KEYS order."""
    bases, masks = np.full(len(KEYS), 0x2D, np.uint8), np.zeros(len(KEYS), np.uint8)
    for j, k in enumerate(KEYS):
        if k not in recs:
            continue
        b, m = po.call_record(recs[k], p)
        if k in excluded:
            m |= po.F_REGION
        bases[j], masks[j] = (0x2D if (m or b == 0x2A) else b), m
    return bases, masks


def _cp(params):
    f, dmin, sdmin, b = params
    return po.CallerParams(MBQ, f, dmin, sdmin, b)


def _dp(p):
    return dev.make_params(p.min_base_quality, p.min_cons_freq, p.min_cons_depth, p.min_cons_strand_depth, p.min_cons_strand_bias)


def _siteset(d, excluded):
    return d.siteset(KEYS, [L.SITE_IN_SNPLIST | (L.SITE_EXCLUDED if k in excluded else 0) for k in KEYS])


def _check(got_bases, got_filters, want, what):
    gb, gf = np.asarray(got_bases), np.asarray(got_filters)
    bad = np.nonzero((gb != want[0]) | (gf != want[1]))[0]
    if len(bad):
        j = int(bad[0])
        raise AssertionError("%s: %d sites differ; first %s: got %r/%d, want %r/%d (%s)" % (
            what, len(bad), KEYS[j], chr(gb[j]), gf[j], chr(want[0][j]), want[1][j], CASES[j][0]))


def test_the_oracle_shortcut_is_call_consensus_sites(files):
    name, data, _, recs, _ = files[0]
    excl = _excluded(0)
    for params in PARAMS[:4]:
        p = _cp(params)
        cons, detail = po.call_consensus_sites(data, KEYS, excl, p)
        b, m = _expect(recs, p, excl)
        assert bytes(b) == cons and all(m[j] == (detail[k][2] if k in detail else 0) for j, k in enumerate(KEYS))


def test_host_buffer_and_streamed_files(d, files):
    """call_consensus (lane kernels without per-site records, the record-writing chain with them) and call_consensus_files with
    raise_file_errors, every class and mode, every parameter set of the cases."""
    excl = _excluded(0)
    ss = _siteset(d, excl)
    seen = {}
    for params in PARAMS:
        p = _cp(params)
        prm = _dp(p)
        want = {name: _expect(recs, p, excl) for name, _, _, recs, _ in files}
        for name, data, _, recs, _ in files:
            for wc in (False, True):
                res = d.call_consensus(ss, data, prm, want_counts=wc)
                _check(res.bases, res.filters, want[name], "%s counts=%s %s" % (name, wc, params))
            seen[name] = len(recs)
        results, rcs, _ = d.call_consensus_files(ss, [f[2] for f in files], prm, want_line_offsets=True)
        for (name, _, path, _, _), r, rc in zip(files, results, rcs):
            d.raise_file_errors(ss, path, prm, int(rc), r)
            _check(r.bases, r.filters, want[name], "files %s %s" % (name, params))
    print("consensus cases per file:", seen)


def test_resident_batches_at_odd_offsets(d, files):
    """call_consensus_batch_dev (one site set) and call_consensus_many_dev with per-sample exclude flags, the samples at odd
    addresses."""
    import torch
    n, S = len(files), len(KEYS)
    offs, at = [], 0
    for _, data, _, _, _ in files:
        at = (at + 255) // 256 * 256 + 3 + 2 * len(offs)
        offs.append(at)
        at += len(data)
    buf = torch.full((at + 64,), 0x0A, dtype=torch.uint8)
    for o, (_, data, _, _, _) in zip(offs, files):
        buf[o:o + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    gbuf = buf.cuda()
    sizes = np.asarray([len(f[1]) for f in files], dtype=np.uint64)
    excl0 = _excluded(0)
    ss = _siteset(d, excl0)
    per_sample = [_excluded(s + 1) for s in range(n)]
    flags = np.asarray([[L.SITE_IN_SNPLIST | (L.SITE_EXCLUDED if k in per_sample[s] else 0) for k in KEYS] for s in range(n)], dtype=np.uint8)
    gflags = torch.from_numpy(flags).cuda()
    for params in PARAMS:
        p = _cp(params)
        prm = _dp(p)
        bases = torch.zeros((n, S), dtype=torch.uint8, device="cuda")
        filt = torch.zeros((n, S), dtype=torch.uint8, device="cuda")
        status = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
        d.call_consensus_batch_dev(ss, gbuf.data_ptr(), np.asarray(offs, dtype=np.uint64), prm, bases.data_ptr(), filt.data_ptr(),
                                   status.data_ptr(), sizes=sizes)
        torch.cuda.synchronize()
        bh, fh = bases.cpu().numpy(), filt.cpu().numpy()
        for s, (name, _, _, recs, _) in enumerate(files):
            _check(bh[s], fh[s], _expect(recs, p, excl0), "batch %s %s" % (name, params))
        bases.zero_()
        filt.zero_()
        d.call_consensus_many_dev(ss, [gbuf.data_ptr() + o for o in offs], sizes, prm, bases.data_ptr(), filt.data_ptr(), status.data_ptr(),
                                  d_site_flags=gflags.data_ptr())
        torch.cuda.synchronize()
        bh, fh = bases.cpu().numpy(), filt.cpu().numpy()
        for s, (name, _, _, recs, _) in enumerate(files):
            _check(bh[s], fh[s], _expect(recs, p, per_sample[s]), "many %s %s" % (name, params))


def test_every_line_records(d, files):
    """call_all_lines and call_all_lines_compact: the consensus base and the filters of every line (listed or not) against
    po.call_record."""
    excl = _excluded(0)
    ss = _siteset(d, excl)
    parsed = {f[0]: f[4] for f in files}
    for params in PARAMS:
        p = _cp(params)
        prm = _dp(p)
        for name, data, path, _, _ in files:
            off, flags, counts = d.call_all_lines(ss, path, prm)
            want = [po.call_record(r, p) for r in parsed[name]]
            assert len(off) == len(want)
            wb = np.asarray([b for b, _ in want], np.uint8)
            wm = np.asarray([m for _, m in want], np.uint8)
            bad = np.nonzero((counts["cons_base"] != wb) | ((counts["filters"] & 0x1F) != wm))[0]
            assert not len(bad), (name, params, int(bad[0]), parsed[name][int(bad[0])].position)
            off2, recs, widx, wide = d.call_all_lines_compact(ss, path, prm)
            flags2, counts2 = dev.expand_line_records(recs, widx, wide)
            assert np.array_equal(off2, off) and np.array_equal(flags2, flags)
            assert np.array_equal(counts2["cons_base"], counts["cons_base"]) and np.array_equal(counts2["filters"], counts["filters"]), (name, params)


def _vcf_rows(data, recs_by_line, p, names, excluded=frozenset(), listed=None):
    rows = []
    for (_, line), rec in zip(po.iter_lines(data), recs_by_line):
        key = (rec.chrom, rec.position)
        if listed is not None and key not in listed:
            continue
        _, m = po.call_record(rec, p)
        if key in excluded:
            m |= po.F_REGION
        rows.append(vco.vcf_row(rec, [names[i] for i in range(6) if m >> i & 1] or None))
    return rows


def test_all_positions_writer_and_console_script(d, files, tmp_path, monkeypatch):
    """--vcfAllPos from file to file, and the call_consensus command, with --minConsFreq 0.55 --minConsStrdBias 0.15 and with
    filter names that int(100 * f) rounds down (0.57 -> VarFreq56, 0.29 -> StrBias28 / VarFreq28; the command takes a
    --minConsFreq above 0.5 only, so 0.29 goes through the writer alone): consensus.fasta and consensus.vcf, FT names included."""
    from snp_pipeline_amd import cfsan_snp_pipeline as cli
    from snp_pipeline_amd import vcf_writer
    monkeypatch.setattr("sys.argv", ["cfsan_snp_pipeline", "test"])
    for (f, b, vf, sb) in ((0.55, 0.15, "VarFreq55", "StrBias15"), (0.57, 0.29, "VarFreq56", "StrBias28"), (0.29, 0.0, "VarFreq28", "StrBias0")):
        p = po.CallerParams(MBQ, f, 1, 0, b)
        names = po.filter_names(p)
        assert (names[1], names[4]) == (vf, sb)
        for name, data, path, _, parsed in files[::3]:
            args = argparse.Namespace(minBaseQual=MBQ, minConsFreq=f, minConsDpth=1, minConsStrdDpth=0, minConsStrdBias=b,
                                      vcfRefName="ref.fasta", vcfPreserveRefCase=False, vcfFailedSnpGt=".")
            ss = _siteset(d, set())
            out = str(tmp_path / ("all_%s.vcf" % name))
            vcf_writer.write_all_positions_vcf_from_pileup(d, ss, out, "s", args, path, _dp(p))
            got = [ln for ln in open(out).read().split("\n") if ln and not ln.startswith("#")]
            assert got == _vcf_rows(data, parsed, p, names), name
            assert any(vf in ln for ln in got) and (b == 0 or any(sb in ln for ln in got))
            if f < 0.5:
                continue
            # the console command, snplist and exclude list
            sdir = tmp_path / ("cli_%s_%d" % (name, int(100 * f)))
            sdir.mkdir()
            pile = str(sdir / "reads.all.pileup")
            with open(pile, "wb") as fh:
                fh.write(data)
            excl = _excluded(3)
            with open(str(sdir / "snplist.txt"), "w") as fh:
                fh.write("".join("%s\t%d\t1\tsampleX\n" % (c.decode(), q) for c, q in KEYS))
            with open(str(sdir / "var.flt_removed.vcf"), "w") as fh:
                fh.write("##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS\n")
                fh.write("".join("%s\t%d\t.\tA\tC\t.\tPASS\t.\tGT\t1/1\n" % (c.decode(), q) for c, q in sorted(excl)))
            line = ("call_consensus -l %s/snplist.txt -o %s/consensus.fasta -e %s/var.flt_removed.vcf --vcfRefName ref.fasta "
                    "--vcfFileName consensus.vcf -q %d --minConsFreq %r --minConsDpth 1 --minConsStrdBias %r %s"
                    % (sdir, sdir, sdir, MBQ, f, b, pile))
            a = cli.parse_command_line(line)
            a.verbose = 0
            assert cli.run_command_from_args(a) == 0
            want, _ = po.call_consensus_sites(data, KEYS, excl, p)
            assert (sdir / "consensus.fasta").read_text() == ">%s\n" % sdir.name + "".join(
                want.decode()[i:i + 60] + "\n" for i in range(0, len(want), 60)), name
            got = [ln for ln in (sdir / "consensus.vcf").read_text().split("\n") if ln and not ln.startswith("#")]
            assert got == _vcf_rows(data, parsed, p, names, excl, set(KEYS)), name
            assert any(names[1] in ln for ln in got) and (b == 0 or any(names[4] in ln for ln in got))


# ---- VarScan ----------------------------------------------------------------------------------------------------------------
VS_PARAMS = {m: sorted({tuple(sorted(kw.items())) for _, _, kw in tc.varscan_cases(m)}) for m in (15, 100)}


def _varscan_file(m, walk, seed):
    """All VarScan cases for --min-avg-qual m: short lines (the LDS walk, in the strips of the ring) or lines of 8.4-8.8 KiB (the
    global-memory walk).  Those are walked byte-wise because the scan does not know their end: a line that does not end in the tile
    after the one that owns it becomes a VS_W_LONG entry, which walk_in_strips never takes and the epilogue kernel walks with
    walk_entry_global (route F1 of tests/varscan_walk_cases.py) - not because of the size of the ring, which holds 11 424 bytes."""
    rng = random.Random(seed)
    lines = []
    for i, (kind, spec, kw) in enumerate(tc.varscan_cases(m)):
        if walk == "global" and i % 2 and not (kind == "VarFreq" and kw["min_var_freq"] == 0.55):
            continue                                          # (half the cases: the Python restatement is slow on 8 KiB lines)
        spec = dict(spec)
        if m > 0:
            spec.setdefault("low", i % 3)
        base = tc.varscan_line(b"ctgV", i + 1, b"ACGT"[i % 4:i % 4 + 1] if i % 5 else b"A", min_avg_qual=m, seed=i, **spec)
        length = len(base) + rng.randint(0, 60) if walk == "lds" else rng.randint(8400, 8800)
        lines.append(tc.varscan_line(b"ctgV", i + 1, b"ACGT"[i % 4:i % 4 + 1] if i % 5 else b"A", min_avg_qual=m, length=length,
                                     seed=i, **spec))
    return b"\n".join(lines) + b"\n"


def _rec_tuples(recs):
    return sorted((int(r["line_off"]), int(r["sdp"]), int(r["dp"]), int(r["total"]), int(r["rdf"]), int(r["rdr"]), int(r["ref_qual_sum"]),
                   int(r["adf"]), int(r["adr"]), int(r["alt_qual_sum"]), int(r["ref_base"]), int(r["alt_base"])) for r in recs)


def test_varscan_walks_at_the_edges(d, tmp_path):
    """Every VarScan case in the LDS walk and in the global-memory walk, --min-avg-qual 15 and 100 (quality bytes >= 0x80): records
    (every field) through varscan_file, varscan_files, varscan_dev and varscan_batch_dev, and var.flt.vcf against vo.mpileup2snp."""
    import torch
    from snp_pipeline_amd import varscan
    blobs, paths = [], []
    for m in (15, 100):
        for walk in ("lds", "global"):
            data = _varscan_file(m, walk, 7 * m + len(walk))
            path = str(tmp_path / ("vs_%d_%s.pileup" % (m, walk)))
            with open(path, "wb") as f:
                f.write(data)
            blobs.append((m, walk, data))
            paths.append(path)
    gpu = [torch.frombuffer(bytearray(b"\0" * 5 + data), dtype=torch.uint8).cuda() for _, _, data in blobs]     # odd addresses
    n_kept = {}
    for i, (m, walk, data) in enumerate(blobs):
        cache = {}
        for kw in VS_PARAMS[m]:
            kw = dict(kw)
            extra = "--min-coverage %d --min-reads2 %d --min-avg-qual %d --min-var-freq %r" % (kw["min_coverage"], kw["min_reads2"], m, kw["min_var_freq"])
            opts = varscan.Options(extra)
            prm = opts.device_params()
            want = tc.varscan_records(data, vo.Params(**kw), cache)
            n_kept[(m, walk)] = n_kept.get((m, walk), 0) + len(want)
            recs, _ = d.varscan_file(paths[i], prm)
            assert _rec_tuples(recs) == want, (m, walk, kw)
            got = d.varscan_files([paths[i], paths[i ^ 1]], prm)
            assert _rec_tuples(got[0][0]) == want, (m, walk, kw)
            r_dev, _ = d.varscan_dev(gpu[i].data_ptr() + 5, len(data), prm)
            assert _rec_tuples(r_dev) == want, (m, walk, kw)
            batch = d.varscan_batch_dev([g.data_ptr() + 5 for g in gpu], [len(b[2]) for b in blobs], prm)
            assert _rec_tuples(batch[i][0]) == want, (m, walk, kw)
            if kw["min_var_freq"] not in (0.55, 0.05):
                continue
            out = str(tmp_path / "var.flt.vcf")
            varscan.mpileup2snp(d, paths[i], out, opts)
            assert open(out, encoding="latin-1").read() == vo.mpileup2snp(data, vo.Params(**kw)), (m, walk, kw)
    print("VarScan records kept per file:", n_kept)
    assert all(v > 0 for v in n_kept.values())
