"""collect_metrics_batch without a GPU: the counting rule as plain text processing against every recorded value that has its
VCF bundled, the table against the bundled one, every row shape by hand, the fastq and table restatements against the live
reference where it is present."""
import argparse
import io
import lzma
import os
import sys
import tarfile
import types

import pytest

from conftest import GOLD

REFERENCE = "/root/reference"


def _cm():
    from snp_pipeline_amd import collect_metrics
    return collect_metrics


def _archive(dataset):
    with open(os.path.join(GOLD, "fixtures", dataset, "expected.tar.xz"), "rb") as f:
        raw = lzma.decompress(f.read())
    with tarfile.open(fileobj=io.BytesIO(raw)) as tar:
        return {m.name: tar.extractfile(m).read() for m in tar.getmembers() if m.isfile()}


def _properties(text):
    return dict(line.split("=", 1) for line in text.decode().split("\n") if "=" in line)


def test_rule_gives_all_seventy_recorded_counts():
    cm = _cm()
    checked = n_files = n_lines = 0
    files = _archive("lambdaVirus")
    for i in range(1, 5):
        props = _properties(files["samples/sample%d/metrics" % i])
        for key, name in (("phase1Snps", "var.flt.vcf"), ("phase1SnpsPreserved", "var.flt_preserved.vcf"), ("snps", "consensus.vcf"),
                          ("snpsPreserved", "consensus_preserved.vcf")):
            assert str(cm.count_snps_text(files["samples/sample%d/%s" % (i, name)])[0]) == props[key], (i, key)
            checked += 1
    every = [files]
    for dataset in ("agona", "listeria"):
        files = _archive(dataset)
        every.append(files)
        rows = files["metrics.tsv"].decode().split("\n")
        head = rows[0].split("\t")
        for row in rows[1:]:
            if not row:
                continue
            cells = dict(zip(head, row.split("\t")))
            for col, name in (("Phase1_SNPs", "var.flt.vcf"), ("Phase1_Preserved_SNPs", "var.flt_preserved.vcf")):
                path = "samples/%s/%s" % (cells["Sample"].strip('"'), name)
                if path in files:
                    assert str(cm.count_snps_text(files[path])[0]) == cells[col], (dataset, path)
                    checked += 1
    assert checked == 70
    # ... and none of the bundled data lines is outside the grammar the kernel judges
    for files in every:
        for name, data in files.items():
            if name.endswith(".vcf"):
                snps, n_data, unusual, usual = cm.count_snps_text(data)
                assert unusual == 0 and usual == snps, name
                n_files += 1
                n_lines += n_data
    assert (n_files, n_lines) == (74, 70426)


def test_combine_gives_the_bundled_table(tmp_path, monkeypatch):
    cm = _cm()
    files = _archive("lambdaVirus")
    dirs = []
    for i in (1, 2, 4, 3):                                          # the order of the bundled table
        d = tmp_path / "samples" / ("sample%d" % i)
        d.mkdir(parents=True)
        (d / "metrics").write_bytes(files["samples/sample%d/metrics" % i])
        dirs.append(str(d))
    out = str(tmp_path / "metrics.tsv")
    cm.combine(dirs, "metrics", out)
    assert open(out, "rb").read() == files["metrics.tsv"]
    log = str(tmp_path / "error.log")
    monkeypatch.setenv("errorOutputFile", log)
    gone, empty = str(tmp_path / "samples" / "gone"), tmp_path / "samples" / "empty"
    empty.mkdir()
    (empty / "metrics").write_bytes(b"")
    cm.combine([dirs[0], gone, str(empty)], "metrics", out, space_headings=True)
    rows = open(out).read().split("\n")
    assert rows[0].split("\t")[:3] == ["Sample", "Fastq Files", "Fastq File Size"] and rows[0].endswith("\tWarnings and Errors")
    assert rows[0].replace(" ", "_") == files["metrics.tsv"].decode().split("\n")[0]
    assert rows[1] == files["metrics.tsv"].decode().split("\n")[1]
    assert rows[2] == "Sample metrics file %s does not exist." % os.path.join(gone, "metrics")
    assert rows[3] == "Sample metrics file %s is empty." % os.path.join(str(empty), "metrics")
    assert rows[2] in open(log).read() and "warning:" in open(log).read()


def _row(gt, ft="PASS", alt="G", fmt=None, ref="A", extra=b""):
    fmt = fmt if fmt is not None else ("GT:SDP:FT" if ft is not None else "GT:SDP")
    sample = "%s:12%s" % (gt, ":" + ft if ft is not None else "")
    return ("chr1\t5\t.\t%s\t%s\t.\tPASS\tNS=1\t%s\t%s" % (ref, alt, fmt, sample)).encode() + extra


@pytest.mark.parametrize("row, count", [
    (_row("0"), 0), (_row("1"), 1), (_row("."), 0), (_row("0/1"), 1), (_row("1/1"), 1), (_row("1|0"), 1), (_row("./."), 0), (_row("./1"), 0),
    (_row("0/0"), 0), (_row("0|0"), 0),
    (_row("1", ft="PASS"), 1), (_row("1", ft="VarFreq60"), 0), (_row("1", ft="PASS;Depth2"), 0), (_row("1", ft=None), 1), (_row("0", ft=None), 0),
    (_row("1", alt="."), 0), (_row("0", alt="."), 0), (_row("1", alt="A,C,T"), 1), (_row("3", alt="A,C,T"), 1), (_row("2/3", alt="A,C,T"), 1),
    (_row("1", alt="*"), 0), (_row("2", alt="G,*"), 0), (_row("1/2", alt="G,*"), 1), (_row("0/1", alt="*"), 1),    # (0/1 with *: REF is a letter)
    (_row("1", alt="GT"), 0), (_row("1", alt="g"), 0), (_row("1", alt="N"), 1), (_row("1", ref="AC", alt="A"), 1),
    (_row("1", ft="Depth2"), 0),                                                                     # --vcfFailedSnpGt 1: GT=1, FT failed
    (_row("1", fmt="SDP:GT:FT").replace(b"\t1:12:PASS", b"\t12:1:PASS"), 1), (_row("1", fmt="FT:SDP:GT").replace(b"\t1:12:PASS", b"\tDepth2:12:1"), 0),
])
def test_row_shapes(row, count):
    cm = _cm()
    assert cm.count_snps_line(row) == count
    assert not cm.is_unusual_line(row)
    header = b"##fileformat=VCFv4.1\n#CHROM\tPOS\n"
    assert cm.count_snps_text(header + row + b"\n") == (count, 1, 0, count)
    assert cm.count_snps_text(header + row) == (count, 1, 0, count)                         # no final newline
    assert cm.count_snps_text((header + row + b"\n" + row + b"\n").replace(b"\n", b"\r\n")) == (2 * count, 2, 0, 2 * count)   # CR LF


def test_rows_outside_the_grammar():
    cm = _cm()
    two = _row("1") + b"\t0:12:PASS"
    assert cm.is_unusual_line(two) and cm.count_snps_line(two) == 1
    both = _row("1") + b"\t1/1:12:PASS"
    assert cm.is_unusual_line(both) and cm.count_snps_line(both) == 2
    for row in (_row("1").rsplit(b"\t", 1)[0], _row("1", fmt="GT:FT"), _row("1", fmt="SDP:DP:FT"), _row("x"), _row("2"), _row(""), _row("1/"),
                _row("1", extra=b"x" * 4096)):
        assert cm.is_unusual_line(row), row
    assert cm.count_snps_line(_row("1").rsplit(b"\t", 1)[0]) == 0 and cm.count_snps_line(_row("2")) == 0 and cm.count_snps_line(_row("x")) == 0
    assert cm.count_snps_text(b"") == (0, 0, 0, 0) and cm.count_snps_text(b"#only\n") == (0, 0, 0, 0) and cm.count_snps_text(b"\n\n") == (0, 0, 0, 0)
    long_ok = _row("1", extra=b"x" * (4095 - len(_row("1"))))
    assert len(long_ok) == 4095 and not cm.is_unusual_line(long_ok) and cm.is_unusual_line(long_ok + b"x")
    assert cm.is_unusual_line(long_ok, raw=4096)                                             # the CR of CR LF counts


def test_collect_one_with_known_values_and_exclusion(tmp_path):
    """collect_one with everything handed in (no device): spelling and order of the file, maxSnps, reuse of fresh values."""
    cm = _cm()
    d = tmp_path / "samples" / "s1"
    d.mkdir(parents=True)
    ref = tmp_path / "ref.fasta"
    ref.write_text(">c1\nACGTACGTAC\n")
    (d / "s1_1.fastq").write_text("@HWI-ST741:189:C0GU5ACXX:8:1101:1219:1953 1:N:0:\nACGT\n+\nIIII\n")
    for name in ("var.flt.vcf", "var.flt_preserved.vcf", "consensus.vcf", "consensus_preserved.vcf", "reads.all.pileup"):
        (d / name).write_text("x\n")
    (d / "consensus.fasta").write_text(">s1\nAC-T-\n")
    (d / "consensus_preserved.fasta").write_text(">other\n---\n")
    counts = {str(d / "var.flt.vcf"): 7, str(d / "var.flt_preserved.vcf"): 3, str(d / "consensus.vcf"): 6, str(d / "consensus_preserved.vcf"): 2}
    known = {"depth_sum": 125, "snp_counts": counts}
    rows = cm.collect_one(str(d), str(ref), cm.Options(maxSnps=5), known)
    assert [name for name, _ in rows] == list(cm.METRIC_NAMES)
    text = (d / "metrics").read_text()
    assert text.split("\n")[:5] == ['sample="s1"', 'fastqFileList="s1_1.fastq"', "fastqFileSize=%d" % os.path.getsize(str(d / "s1_1.fastq")),
                                   "machine=HWI-ST741", "flowcell=C0GU5ACXX"]
    m = cm.read_properties(str(d / "metrics"))
    assert m["avePileupDepth"] == "12.50" and m["phase1Snps"] == "7" and m["phase1SnpsPreserved"] == "3"
    assert m["excludedSample"] == "Excluded" and m["snps"] == "" and m["missingPos"] == ""
    assert m["excludedSamplePreserved"] == "" and m["snpsPreserved"] == "2" and m["missingPosPreserved"] == "0"
    assert m["errorList"] == "SAM file reads.sam was not found. Deduped BAM file reads.sorted.deduped.bam was not found. Excluded: exceeded 5 maxsnps."
    # the file is now newer than its inputs: everything is reused, the reused phase1Snps is compared as a number
    assert cm.stale_inputs(str(d), cm.Options(maxSnps=5)) == (None, [])      # (consensus.vcf of the excluded flow is not counted for nothing)
    assert cm.stale_inputs(str(d), cm.Options()) == (None, [str(d / "consensus.vcf")])                # ... without --maxsnps its count is wanted
    again = cm.collect_one(str(d), str(ref), cm.Options(maxSnps=5), {"snp_counts": {}})
    assert again == rows
    with pytest.raises(RuntimeError):                                                          # no quiet count on the host
        cm.collect_one(str(d), str(ref), cm.Options(forceFlag=True), {"depth_sum": 1})
    cm.collect_one(str(d), str(ref), cm.Options(forceFlag=True), {"depth_sum": 0, "snp_counts": counts})
    m = cm.read_properties(str(d / "metrics"))
    assert m["missingPos"] == "2" and m["snps"] == "6" and "Cannot calculate mean pileup depth." in m["errorList"] and m["avePileupDepth"] == ""


def test_subcommand_is_there_with_the_reference_defaults():
    from snp_pipeline_amd import cfsan_snp_pipeline
    args = cfsan_snp_pipeline.parse_argument_list(["collect_metrics_batch", "dirs.txt", "ref.fasta"])
    assert (args.forceFlag, args.metricsFile, args.maxSnps, args.verbose, args.mergedMetricsFile, args.spaceHeadings) == (False, "metrics", -1, 1, None, False)
    assert (args.consensusFastaFileName, args.consensusPreservedFastaFileName, args.consensusVcfFileName, args.consensusPreservedVcfFileName) == \
        ("consensus.fasta", "consensus_preserved.fasta", "consensus.vcf", "consensus_preserved.vcf")
    args = cfsan_snp_pipeline.parse_argument_list(["collect_metrics_batch", "-f", "-o", "m2", "-m", "9", "-c", "a", "-C", "b", "-v", "c", "-V", "d", "--verbose", "0",
                                                   "--mergedMetricsFile", "t.tsv", "-s", "dirs.txt", "ref.fasta"])
    assert (args.forceFlag, args.metricsFile, args.maxSnps, args.consensusFastaFileName, args.consensusPreservedFastaFileName, args.consensusVcfFileName,
            args.consensusPreservedVcfFileName, args.verbose, args.mergedMetricsFile, args.spaceHeadings) == (True, "m2", 9, "a", "b", "c", "d", 0, "t.tsv", True)


# ---- against the live reference, where it is present ---------------------------------------------------------------------------
def _reference_module(name):
    """A module of the reference loaded on its own, with a stand-in for the package (utils needs nothing else)."""
    import importlib.util
    pkg = types.ModuleType("snppipeline")
    pkg.__path__ = [os.path.join(REFERENCE, "snppipeline")]
    pkg.__version__ = "test"
    stand_ins = ("Bio", "Bio.SeqIO", "Bio.Seq", "Bio.SeqRecord", "vcf")        # what utils imports and these two modules never call
    saved = {k: sys.modules.get(k) for k in ("snppipeline", "snppipeline.utils", "snppipeline." + name) + stand_ins}
    sys.modules["snppipeline"] = pkg
    for k in stand_ins:
        if k not in sys.modules:
            sys.modules[k] = types.ModuleType(k)
            if "." in k:
                setattr(sys.modules[k.split(".")[0]], k.split(".")[1], sys.modules[k])
                setattr(sys.modules[k], k.split(".")[1], object)              # (from Bio.Seq import Seq ...)
    try:
        mods = {}
        for mod in ("utils", name):
            spec = importlib.util.spec_from_file_location("snppipeline." + mod, os.path.join(REFERENCE, "snppipeline", mod + ".py"))
            m = importlib.util.module_from_spec(spec)
            sys.modules["snppipeline." + mod] = m
            spec.loader.exec_module(m)
            mods[mod] = m
        return mods[name]
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "snppipeline")), reason="the reference tree is not on this machine")
def test_fastq_and_table_restatements_against_the_live_reference(tmp_path):
    cm = _cm()
    fastq = _reference_module("fastq")
    combine_metrics = _reference_module("combine_metrics")
    lines = ["@SRR1206159_1/1", "@SRR498276.1 HWI-M00229:9:000000000-A1474:1:1:15012:1874 length=151",
             "@SRR498276.1 HWI-M00229:9:000100000-A1474:1:1:15012:1874 length=151", "@SRR498423_HWI-M00229:7:000000000-A0WG8:1:1:12203:2225/1",
             "@HWI-ST741:189:C0GU5ACXX:8:1101:1219:1953 1:N:0:", '@ERR178930.1 HWI-ST322_0214_"AC0HTNACXX":8:1101:1555:2158#ATCACG length=101',
             "@HWUSI:189:0000-FLOW:8:1101:1219:1953 1:N:0:", "@FCC3NWVACXX:3:1101:1161:2200#AACCGAGAA/2", "@SRR1840614.1 FCC1KPRACXX:1:1101:1291:2172 length=200",
             "@SRR1166969.1 HWI-ST406:204:d1cywacxx:7:1101:1292:1941 length=100", "@r1", "", "@MISEQ:6:000000000-A1445:1:1:16976:1440 2:N:0:CGTACTAGTAGATCGC"]
    import json
    with open(os.path.join(GOLD, "lambda_fastq_first_lines.json")) as f:
        for per_sample in json.load(f).values():
            lines.extend(per_sample.values())
    d = tmp_path / "fq"
    d.mkdir()
    import gzip
    for k, line in enumerate(lines):
        path = str(d / ("f%02d.fastq" % k)) + (".gz" if k % 2 else "")
        with (gzip.open(path, "wt") if k % 2 else open(path, "w")) as f:
            f.write(line + "\nACGT\n+\nIIII\n")
        want = fastq.extract_metadata_tags(path)
        got = cm.extract_metadata_tags(path)
        assert (got is None) == (want is None), line
        if want is not None:
            assert got == (want.instrument, want.flow_cell), line
    for name in ("a.fq", "b.fq.gz", "c.notfastq", "d.fastq.not"):
        (d / name).write_text("")
    assert cm.list_fastq_files(str(d)) == fastq.list_fastq_files(str(d))
    # the table
    dirs = []
    for k in range(3):
        s = tmp_path / "samples" / ("s%d" % k)
        s.mkdir(parents=True)
        dirs.append(str(s))
    with open(os.path.join(dirs[0], "metrics"), "w") as f:
        f.write('sample="s0"\nfastqFileList="a.fastq, b.fastq"\nfastqFileSize=12\nmachine=M1\nflowcell=\nnumberReads=5\nerrorList="No fastq files were found. x"\n')
    with open(os.path.join(dirs[1], "metrics"), "w") as f:
        f.write("")
    listing = str(tmp_path / "dirs.txt")
    with open(listing, "w") as f:
        f.write("\n".join(dirs) + "\n")
    for spaces in (False, True):
        want_path, got_path = str(tmp_path / "want.tsv"), str(tmp_path / "got.tsv")
        combine_metrics.combine_metrics(argparse.Namespace(sampleDirsFile=listing, metricsFileName="metrics", mergedMetricsFile=want_path, forceFlag=True,
                                                           spaceHeadings=spaces, verbose=0))
        cm.combine(dirs, "metrics", got_path, spaces)
        assert open(got_path).read() == open(want_path).read()
