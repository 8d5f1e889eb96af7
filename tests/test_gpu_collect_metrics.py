"""The VCF count kernel and collect_metrics_batch on the device, against the Python statement of the counting rule
(snp_pipeline_amd.collect_metrics.count_snps_text, itself pinned by tests/test_collect_metrics.py)."""
import os
import shutil
import time

import pytest

from conftest import GOLD, extract_fixture

pytestmark = pytest.mark.gpu

TILE = 16384
STEP = (16 << 20) - 4096 - 16           # new bytes per streamed piece of a file (csrc/stream.hip: vcf_count_stream)
K_SCAN, K_VCF_COUNT = 0, 4


@pytest.fixture(scope="module")
def dev():
    from gpu_util import get_device
    return get_device()


def _cm():
    from snp_pipeline_amd import collect_metrics
    return collect_metrics


HEADER = b"##fileformat=VCFv4.1\n##source=test\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tsample\n"
ROWS = [  # the shapes this build's consensus writer and VarScan emit
    b"chr1\t%d\t.\tA\tG\t.\tPASS\tNS=1\tGT:SDP:RD:AD:RDF:RDR:ADF:ADR:FT\t1:33:0:33:0:0:17:16:PASS\n",
    b"chr1\t%d\t.\tA\t.\t.\tPASS\tNS=1\tGT:SDP:RD:AD:RDF:RDR:ADF:ADR:FT\t0:30:30:0:14:16:0:0:PASS\n",
    b"chr1\t%d\t.\tC\tT\t.\tVarFreq60\tNS=1\tGT:SDP:RD:AD:RDF:RDR:ADF:ADR:FT\t.:10:5:5:2:3:3:2:VarFreq60\n",
    b"chr1\t%d\t.\tC\tT\t.\tDepth2\tNS=1\tGT:SDP:RD:AD:RDF:RDR:ADF:ADR:FT\t1:1:0:1:0:0:1:0:Depth2\n",
    b"chr1\t%d\t.\tG\tA,*\t.\tPASS\tNS=1\tGT:SDP:FT\t2:12:PASS\n",
    b"chr1\t%d\t.\tT\tC\t.\tPASS\tADP=52;WT=0;HET=0;HOM=1;NC=0\tGT:GQ:SDP:DP:RD:AD:FREQ:PVAL:RBQ:ABQ:RDF:RDR:ADF:ADR\t1/1:255:52:52:0:52:100%%:6.3E-31:0:38:0:0:27:25\n",
    b"chr1\t%d\t.\tT\tC\t.\tPASS\tADP=52\tGT:GQ\t0/1:255\n",
]


def _rows(start, n):
    return b"".join(ROWS[(start + i) % len(ROWS)] % (start + i) for i in range(n))


def _file_with_row_ends_at(targets, delta):
    """VCF text in which, for every byte offset T of `targets`, a row's terminator is the byte T - 1 + delta (delta 0: the row
    ends ON the edge, the next one starts at T)."""
    block = _rows(1, 7000)
    out = [HEADER]
    size = len(HEADER)
    for t in sorted(targets):
        want = t - 1 + delta                        # where the LF goes
        while want - size > len(block) + 400:
            out.append(block)
            size += len(block)
        fill = _rows(1, max(0, (want - size - 300) // 60))
        while fill and len(fill) > want - size - 150:
            fill = fill[:fill.rfind(b"\n", 0, len(fill) - 1) + 1]
        out.append(fill)
        size += len(fill)
        pad = want - size - len(b"chr1\t7\t.\tA\tG\t.\tPASS\tNS=1;X=\tGT:FT\t1:PASS")
        assert pad >= 0
        out.append(b"chr1\t7\t.\tA\tG\t.\tPASS\tNS=1;X=" + b"x" * pad + b"\tGT:FT\t1:PASS\n")
        size = want + 1
    out.append(_rows(1, 50))
    data = b"".join(out)
    for t in targets:
        assert data[t - 1 + delta:t + delta] == b"\n"
    return data


def _check(dev, tmp_path, name, data, unusual=0):
    """The kernel's three counts on `data` equal the Python statement's, with exactly `unusual` unusual lines; the count the
    host makes of it is the statement's total."""
    cm = _cm()
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(data)
    snps, n_data, n_unusual, usual_snps = cm.count_snps_text(data)
    got = dev.vcf_count_snps_file(path)
    print(name, len(data), "kernel", got[:3], "statement", (usual_snps, n_data, n_unusual))
    assert n_unusual == unusual
    assert got[:3] == (usual_snps, n_data, n_unusual)
    if n_unusual <= cm.UNUSUAL_CAPACITY and not got[4]:
        assert got[3] == [off for off, line, raw in cm.data_lines(data) if cm.is_unusual_line(line, raw)]
    assert cm.count_snps_files(dev, [path]) == [snps]
    return got


def _bundled_vcfs(tmp_path_factory):
    out = []
    for ds in ("lambdaVirus", "agona", "listeria"):
        dest = str(tmp_path_factory.mktemp("vcf_" + ds))
        extract_fixture(ds, dest)
        for dirpath, _, names in sorted(os.walk(dest)):
            out.extend(os.path.join(dirpath, n) for n in sorted(names) if n.endswith(".vcf"))
    return out


def test_kernel_counts_every_bundled_vcf_with_no_unusual_line(dev, tmp_path_factory):
    cm = _cm()
    paths = _bundled_vcfs(tmp_path_factory)
    assert len(paths) == 74
    results = dev.vcf_count_snps_files(paths)                       # one stream
    lines = 0
    for path, got in zip(paths, results):
        with open(path, "rb") as f:
            snps, n_data, n_unusual, usual = cm.count_snps_text(f.read())
        assert got[:3] == (snps, n_data, 0), path
        assert n_unusual == 0 and usual == snps
        lines += n_data
    assert lines == 70426
    assert cm.count_snps_files(dev, paths[:5]) == [r[0] for r in results[:5]]


def test_small_shapes(dev, tmp_path):
    body = _rows(1, 40)
    _check(dev, tmp_path, "plain.vcf", HEADER + body)
    _check(dev, tmp_path, "no_final_newline.vcf", HEADER + body[:-1])
    _check(dev, tmp_path, "header_only.vcf", HEADER)
    _check(dev, tmp_path, "header_no_newline.vcf", HEADER[:-1])
    _check(dev, tmp_path, "empty.vcf", b"")
    _check(dev, tmp_path, "one_byte.vcf", b"\n")
    _check(dev, tmp_path, "crlf.vcf", (HEADER + body).replace(b"\n", b"\r\n"))
    _check(dev, tmp_path, "blank_lines.vcf", HEADER + b"\n\n" + body + b"\n")
    _check(dev, tmp_path, "no_header.vcf", body)


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_rows_at_every_tile_and_chunk_edge(dev, tmp_path, delta):
    """A row ending one byte before, on and one byte after: the lane edges, the tile edges, the edge of a streamed piece, the
    start of the look-back of the next piece, and 16 MiB; the file itself ends on / around an edge as well."""
    targets = [64 * 3, TILE, 2 * TILE, 5 * TILE + 64, STEP - 4096, STEP - TILE, STEP, STEP + TILE, 16 << 20]
    data = _file_with_row_ends_at(targets, delta)
    _check(dev, tmp_path, "edges.vcf", data)
    short = _file_with_row_ends_at([TILE, 3 * TILE], delta)
    end = 3 * TILE + delta
    _check(dev, tmp_path, "ends_at_edge.vcf", short[:end])               # the file ends with that row's LF
    _check(dev, tmp_path, "ends_before_lf.vcf", short[:end - 1])         # ... without it
    whole = _file_with_row_ends_at([STEP], delta)
    _check(dev, tmp_path, "ends_at_piece.vcf", whole[:STEP + delta])
    _check(dev, tmp_path, "ends_at_piece_no_lf.vcf", whole[:STEP + delta - 1])


def test_forty_megabytes_of_writer_rows(dev, tmp_path):
    block = _rows(1, 70000)
    data = HEADER + block * (40 * 1000 * 1000 // len(block) + 1)
    assert len(data) > 40 * 1000 * 1000
    _check(dev, tmp_path, "big.vcf", data)


def test_unusual_lines_go_to_the_host_and_are_counted_exactly(dev, tmp_path):
    cm = _cm()
    good = _rows(1, 30)
    unusual = [
        b"chr1\t5\t.\tA\tG\t.\tPASS\tNS=1\tGT:FT\n",                                  # nine columns
        b"chr1\t5\t.\tA\tG\t.\tPASS\tNS=2\tGT:FT\t1:PASS\t0:PASS\n",                  # two samples: one counts
        b"chr1\t5\t.\tA\tG\t.\tPASS\tNS=2\tGT:FT\t1:PASS\t1:PASS\n",                  # two samples: both count
        b"chr1\t5\t.\tA\tG\t.\tPASS\tNS=1\tGT:SDP:FT\t1:PASS\n",                      # field counts differ
        b"chr1\t5\t.\tA\tG\t.\tPASS\tNS=1\tSDP:FT\t4:PASS\n",                         # no GT
        b"chr1\t5\t.\tA\tG\t.\tPASS\tNS=1\tGT:FT\tx:PASS\n",                          # not a number
        b"chr1\t5\t.\tA\tG\t.\tPASS\tNS=1\tGT:FT\t2:PASS\n",                          # past the list
        b"chr1\t5\t.\tA\tG\t.\tPASS\tNS=1\tGT:FT\t:PASS\n",                           # empty GT
    ]
    data = HEADER + good + b"".join(unusual) + good
    got = _check(dev, tmp_path, "unusual.vcf", data, unusual=8)
    assert got[4] == 0
    snps = cm.count_snps_text(data)
    assert snps[0] == snps[3] + 3                                  # the host adds 1 + 2 for the two-sample rows
    # a line longer than the kernel's window: reported by its terminator, the host counts the whole file
    long_row = b"chr1\t9\t.\tA\tG\t.\tPASS\tNS=1;X=" + b"x" * 5000 + b"\tGT:FT\t1:PASS\n"
    from snp_pipeline_amd import _lib as L
    got = _check(dev, tmp_path, "long.vcf", HEADER + good + long_row + good, unusual=1)
    assert got[4] & L.VCF_LONG_LINE and got[3][0] >> 63
    # a HEADER line that long is reported the same way (the kernel has not seen its first byte); the host finds that it counts nothing
    text = HEADER + b"##long=" + b"x" * 6000 + b"\n" + good + long_row + good
    path = str(tmp_path / "long_header.vcf")
    with open(path, "wb") as f:
        f.write(text)
    got = dev.vcf_count_snps_file(path)
    assert got[2] == 2 and got[4] == L.VCF_LONG_LINE and got[0] == cm.count_snps_text(text)[3]
    assert cm.count_snps_files(dev, [path]) == [cm.count_snps_text(text)[0]]
    ends = (b"chr1\t9\t.\tA\tG\t.\tPASS\tNS=1;X=", b"\tGT:FT\t1:PASS\n")
    edge = ends[0] + b"x" * (4096 - len(ends[0]) - len(ends[1])) + ends[1]
    assert len(edge) == 4096                                       # 4095 bytes + LF: the longest line the kernel judges
    _check(dev, tmp_path, "window.vcf", HEADER + good + edge + good, unusual=0)
    _check(dev, tmp_path, "window1.vcf", HEADER + good + edge[:30] + b"x" + edge[30:] + good, unusual=1)
    # more unusual lines than the capacity: the host counts the whole file
    many = HEADER + good + unusual[2] * (cm.UNUSUAL_CAPACITY + 5) + good
    got = _check(dev, tmp_path, "many.vcf", many, unusual=cm.UNUSUAL_CAPACITY + 5)
    assert got[4] & L.VCF_MORE_UNUSUAL
    with pytest.raises(IOError):
        dev.vcf_count_snps_file(str(tmp_path / "missing.vcf"))
    mixed = dev.vcf_count_snps_files([str(tmp_path / "unusual.vcf"), str(tmp_path / "missing.vcf"), str(tmp_path / "window.vcf")])
    assert isinstance(mixed[1], IOError) and mixed[0][2] == 8 and mixed[2][2] == 0


# ---- end to end ----------------------------------------------------------------------------------------------------------------
LAMBDA_FASTQ_FIRST_LINES = os.path.join(GOLD, "lambda_fastq_first_lines.json")


def _lambda_tree(tmp_path):
    """The bundled ExpectedResults of lambdaVirus as a tree collect_metrics can run on: tiny fastq files with the real first
    lines, placeholder reads.sam / BAM / pileup OLDER than a metrics file that holds only the bundled samtools and depth
    values."""
    import json
    cm = _cm()
    want = str(tmp_path / "want")
    extract_fixture("lambdaVirus", want)
    work = str(tmp_path / "work")
    shutil.copytree(want, work)
    with open(LAMBDA_FASTQ_FIRST_LINES) as f:
        first = json.load(f)
    old = time.time() - 1000
    dirs = []
    for i in (1, 2, 4, 3):                                          # (the order of the bundled table)
        d = os.path.join(work, "samples", "sample%d" % i)
        dirs.append(d)
        for name, line in first["sample%d" % i].items():
            with open(os.path.join(d, name), "w") as f:
                f.write(line + "\nACGT\n+\nIIII\n")
        for name in ("reads.sam", "reads.sorted.deduped.bam", "reads.all.pileup"):
            with open(os.path.join(d, name), "w") as f:
                f.write("placeholder\n")
            os.utime(os.path.join(d, name), (old, old))
        bundled = cm.read_properties(os.path.join(want, "samples", "sample%d" % i, "metrics"))
        os.remove(os.path.join(d, "metrics"))
        with open(os.path.join(d, "metrics"), "w") as f:
            for key in ("numberReads", "numberDupReads", "percentReadsMapped", "percentProperPair", "aveInsertSize", "avePileupDepth"):
                f.write("%s=%s\n" % (key, bundled[key]))
        os.utime(os.path.join(d, "metrics"), (old + 500, old + 500))
    listing = os.path.join(work, "sampleDirectories.txt")
    with open(listing, "w") as f:
        f.write("\n".join(dirs) + "\n")
    return want, work, dirs, listing


def _without_size(text, d):
    """The metrics text with the fastqFileSize value replaced by a mark, after checking it against the files on disk."""
    cm = _cm()
    out = []
    for line in text.split("\n"):
        if line.startswith("fastqFileSize=") and d is not None:
            assert int(line.split("=")[1]) == sum(os.path.getsize(p) for p in cm.list_fastq_files(d))
            line = "fastqFileSize=*"
        out.append(line)
    return "\n".join(out)


def test_lambda_end_to_end_gives_the_bundled_metrics_and_table(dev, tmp_path):
    from snp_pipeline_amd import cfsan_snp_pipeline
    cm = _cm()
    want, work, dirs, listing = _lambda_tree(tmp_path)
    merged = os.path.join(work, "metrics_out.tsv")
    reference = os.path.join(GOLD, "fixtures", "lambdaVirus", "lambda_virus.fasta")
    cfsan_snp_pipeline.run_command_from_arg_list(["collect_metrics_batch", "--mergedMetricsFile", merged, "--verbose", "0", listing, reference])
    sizes = {}
    for i, d in enumerate(dirs, 1):
        got = open(os.path.join(d, "metrics")).read()
        bundled = os.path.join(want, "samples", os.path.basename(d), "metrics")
        exp = open(bundled).read()
        assert _without_size(got, d) == "\n".join("fastqFileSize=*" if ln.startswith("fastqFileSize=") else ln for ln in exp.split("\n"))
        sizes[i] = (cm.read_properties(os.path.join(d, "metrics"))["fastqFileSize"], cm.read_properties(bundled)["fastqFileSize"])
    got_rows = open(merged).read().split("\n")
    exp_rows = open(os.path.join(want, "metrics.tsv")).read().split("\n")
    assert len(got_rows) == len(exp_rows) and got_rows[0] == exp_rows[0]
    for i in range(1, 5):
        g, e = got_rows[i].split("\t"), exp_rows[i].split("\t")
        assert (g[2], e[2]) == sizes[i]
        assert g[:2] + g[3:] == e[:2] + e[3:]
    # a second run without -f reuses every value: nothing goes to the device
    dev.kernel_timing(True)
    try:
        dev.kernel_time_ms(K_SCAN), dev.kernel_time_ms(K_VCF_COUNT)
        before = {d: open(os.path.join(d, "metrics")).read() for d in dirs}
        done = cm.run_batch(dirs, reference, cm.Options(), devices=[dev])
        assert (done["failed"], done["pileups_summed"], done["vcf_files_counted"], done["errors"]) == (0, 0, 0, {})
        assert dev.kernel_time_ms(K_SCAN)[1] == 0 and dev.kernel_time_ms(K_VCF_COUNT)[1] == 0
        assert before == {d: open(os.path.join(d, "metrics")).read() for d in dirs}
        # ... and with -f the VCF files are counted again on this device (the placeholder pileup has no depth: that text is recorded)
        done = cm.run_batch(dirs, reference, cm.Options(forceFlag=True, maxSnps=40), devices=[dev])
        assert done["vcf_files_counted"] == 16 and done["pileups_summed"] == 4
        assert dev.kernel_time_ms(K_VCF_COUNT)[1] >= 16
    finally:
        dev.kernel_timing(False)
    for d in dirs:
        m = cm.read_properties(os.path.join(d, "metrics"))
        exp = cm.read_properties(os.path.join(want, "samples", os.path.basename(d), "metrics"))
        assert "Cannot calculate mean pileup depth." in m["errorList"]
        assert m["phase1Snps"] == exp["phase1Snps"] and m["phase1SnpsPreserved"] == exp["phase1SnpsPreserved"]
        for key, excl, missing, text, snps in (("phase1Snps", "excludedSample", "missingPos", "Excluded: exceeded 40 maxsnps.", "snps"),
                                               ("phase1SnpsPreserved", "excludedSamplePreserved", "missingPosPreserved",
                                                "Excluded: preserved exceeded 40 maxsnps.", "snpsPreserved")):
            if int(exp[key]) > 40:
                assert m[excl] == "Excluded" and m[snps] == "" and m[missing] == "" and text in m["errorList"]
            else:
                assert m[excl] == "" and m[snps] == exp[snps] and text not in m["errorList"]


def test_missing_sample_directory_is_a_sample_error_and_the_others_go_on(dev, tmp_path, monkeypatch):
    cm = _cm()
    want, work, dirs, listing = _lambda_tree(tmp_path)
    log = str(tmp_path / "error.log")
    monkeypatch.setenv("errorOutputFile", log)
    monkeypatch.setenv("StopOnSampleError", "false")
    reference = os.path.join(GOLD, "fixtures", "lambdaVirus", "lambda_virus.fasta")
    gone = os.path.join(work, "samples", "sample9")
    merged = str(tmp_path / "m.tsv")
    done = cm.run_batch(dirs[:2] + [gone], reference, cm.Options(), merged_path=merged, devices=[dev])
    assert done["failed"] == 1 and done["vcf_files_counted"] == 8
    assert "Sample directory %s does not exist." % gone in open(log).read()
    rows = open(merged).read().split("\n")
    assert rows[3] == "Sample metrics file %s does not exist." % os.path.join(gone, "metrics")


# ---- the synthetic outbreak: the separate subcommands, then collect_metrics_batch; and the same inside hot_path_batch -----------
FILTER_EXTRA = "--edge_length 100 --window_size 1000 125 15 --max_snp 3 2 1 --mode all"
VCF_NAMES = ("var.flt.vcf", "var.flt_preserved.vcf", "consensus.vcf", "consensus_preserved.vcf")
COUNT_KEYS = ("phase1Snps", "phase1SnpsPreserved", "snps", "snpsPreserved")


def _statement_counts(sdir):
    cm = _cm()
    return [cm.count_snps_text(open(os.path.join(sdir, n), "rb").read())[0] for n in VCF_NAMES]


def test_synthetic_outbreak_through_the_separate_subcommands(dev, tmp_path, monkeypatch):
    import test_gpu_pipeline as tp
    cm = _cm()
    work = tmp_path
    ref_path, dirs, dirs_file, piles = tp._outbreak_tree(work)
    monkeypatch.setenv("VarscanMpileup2snp_ExtraParams", tp.VARSCAN_EXTRA)
    monkeypatch.setenv("StopOnSampleError", "false")
    monkeypatch.setenv("errorOutputFile", str(work / "error.log"))
    monkeypatch.chdir(work)
    tp._separate_steps(work, ref_path, dirs, dirs_file, FILTER_EXTRA, "", tp.CONSENSUS_EXTRA + " --amdMetricsRefFasta " + ref_path)
    by_product = {}
    for sdir in dirs:                                           # what call_consensus --amdMetricsRefFasta left behind
        by_product[sdir] = cm.read_properties(os.path.join(sdir, "metrics"))
        assert float(by_product[sdir]["avePileupDepth"]) > 5
        os.remove(os.path.join(sdir, "metrics"))
    # the kernel on the files this build's own writers have just produced: no unusual line
    paths = [os.path.join(sdir, n) for sdir in dirs for n in VCF_NAMES]
    for path, got in zip(paths, dev.vcf_count_snps_files(paths)):
        snps, n_data, n_unusual, usual = cm.count_snps_text(open(path, "rb").read())
        print(path, got[:3])
        assert got[:3] == (snps, n_data, 0) and n_unusual == 0 and n_data > 5, path
    merged = str(work / "metrics.tsv")
    tp._run("collect_metrics_batch --mergedMetricsFile %s --verbose 0 %s %s" % (merged, dirs_file, ref_path))
    phase1 = []
    for sdir in dirs:
        m = cm.read_properties(os.path.join(sdir, "metrics"))
        assert m["avePileupDepth"] == by_product[sdir]["avePileupDepth"], sdir          # the device depth-sum route
        assert m["missingPos"] == by_product[sdir]["missingPos"] and m["missingPosPreserved"] == by_product[sdir]["missingPosPreserved"]
        assert [m[k] for k in COUNT_KEYS] == [str(c) for c in _statement_counts(sdir)], sdir
        assert m["excludedSample"] == "" and m["excludedSamplePreserved"] == "" and "Cannot calculate mean" not in m["errorList"]
        phase1.append(int(m["phase1Snps"]))
    rows = open(merged).read().split("\n")
    assert len(rows) == len(dirs) + 2 and [r.split("\t")[0] for r in rows[1:-1]] == ['"%s"' % os.path.basename(d) for d in reversed(dirs)]
    # in-process with -f: every pileup through the scan (none refused), every VCF file through the count kernel
    dev.kernel_timing(True)
    try:
        dev.kernel_time_ms(K_SCAN), dev.kernel_time_ms(K_VCF_COUNT)
        done = cm.run_batch(dirs, ref_path, cm.Options(forceFlag=True), devices=[dev])
        assert (done["failed"], done["pileups_summed"], done["vcf_files_counted"], done["depth_fallbacks"]) == (0, len(dirs), 4 * len(dirs), 0)
        assert dev.kernel_time_ms(K_SCAN)[1] > 0 and dev.kernel_time_ms(K_VCF_COUNT)[1] >= 4 * len(dirs)
        # --maxsnps small enough to exclude some samples: their snps and missingPos are blank, both texts recorded per flow
        limit = sorted(phase1)[len(phase1) // 2]
        assert min(phase1) <= limit < max(phase1)
        done = cm.run_batch(dirs, ref_path, cm.Options(forceFlag=True, maxSnps=limit), devices=[dev])
        n_excluded = 0
        for sdir in dirs:
            m = cm.read_properties(os.path.join(sdir, "metrics"))
            counts = _statement_counts(sdir)
            for flow, (excl, snps, missing, text) in enumerate((("excludedSample", "snps", "missingPos", "Excluded: exceeded %d maxsnps." % limit),
                                                                ("excludedSamplePreserved", "snpsPreserved", "missingPosPreserved",
                                                                 "Excluded: preserved exceeded %d maxsnps." % limit))):
                assert m[COUNT_KEYS[flow]] == str(counts[flow])
                if counts[flow] > limit:
                    n_excluded += 1
                    assert m[excl] == "Excluded" and m[snps] == "" and m[missing] == "" and text in m["errorList"], sdir
                else:
                    assert m[excl] == "" and m[snps] == str(counts[2 + flow]) and m[missing] == by_product[sdir][missing] and text not in m["errorList"], sdir
        assert n_excluded > 0
        # a second run without -f reuses everything: no device call
        dev.kernel_time_ms(K_SCAN), dev.kernel_time_ms(K_VCF_COUNT)
        before = {d: open(os.path.join(d, "metrics")).read() for d in dirs}
        done = cm.run_batch(dirs, ref_path, cm.Options(maxSnps=limit), devices=[dev])
        assert (done["pileups_summed"], done["vcf_files_counted"]) == (0, 0)
        assert dev.kernel_time_ms(K_SCAN)[1] == 0 and dev.kernel_time_ms(K_VCF_COUNT)[1] == 0
        assert before == {d: open(os.path.join(d, "metrics")).read() for d in dirs}
    finally:
        dev.kernel_timing(False)


def test_hot_path_batch_collect_metrics_equals_the_separate_route(dev, tmp_path, monkeypatch):
    import test_gpu_pipeline as tp
    from snp_pipeline_amd import hot_path
    cm = _cm()
    work = tmp_path
    ref_path, dirs, dirs_file, piles = tp._outbreak_tree(work)
    monkeypatch.setenv("VarscanMpileup2snp_ExtraParams", tp.VARSCAN_EXTRA)
    monkeypatch.chdir(work)
    line = ("hot_path_batch -f %s %s --filterRegionsExtraParams=%s --callConsensusExtraParams=%s"
            % (dirs_file, ref_path, FILTER_EXTRA.replace(" ", "\x00"), tp.CONSENSUS_EXTRA.replace(" ", "\x00")))
    tp._run(line)                                               # the job as it is without the option ...
    assert hot_path.hot_path_batch.last_stats["collect_metrics"] is None
    assert not any(os.path.exists(os.path.join(d, "metrics")) for d in dirs) and not os.path.exists(str(work / "metrics.tsv"))
    merged = str(work / "metrics.tsv")
    tp._run("collect_metrics_batch --mergedMetricsFile %s --verbose 0 %s %s" % (merged, dirs_file, ref_path))       # ... then the subcommand
    want_metrics = {d: open(os.path.join(d, "metrics")).read() for d in dirs}
    want_table = open(merged).read()
    for d in dirs:
        os.remove(os.path.join(d, "metrics"))
    os.remove(merged)
    want = tp._snapshot(work, dirs)
    tp._run(line + " --collectMetrics --mergedMetricsFile " + merged)
    tp._compare(tp._snapshot(work, dirs, remove=False), want)   # the job's other outputs: byte for byte
    assert {d: open(os.path.join(d, "metrics")).read() for d in dirs} == want_metrics
    assert open(merged).read() == want_table
    for d in dirs:
        m = cm.read_properties(os.path.join(d, "metrics"))
        assert float(m["avePileupDepth"]) > 5 and [m[k] for k in COUNT_KEYS] == [str(c) for c in _statement_counts(d)]
    st = hot_path.hot_path_batch.last_stats
    total = sum(len(p) for p in piles)
    assert st["h2d_bytes"] == total and st["file_bytes"] == total          # no pileup is read a second time
    assert st["collect_metrics"] == {"failed": 0, "pileups_summed": 0, "vcf_files_counted": 4 * len(dirs), "depth_fallbacks": 0}
    assert "collect_metrics" in st["phases"]
