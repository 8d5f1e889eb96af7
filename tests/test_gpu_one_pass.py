"""hot_path_batch --pileupRoute: every pileup crosses the host link once at ANY size where the device does not write var.flt.vcf.

With ``--siteCalling existing`` (and ``varscan``) both site lists are known before the first pileup byte moves, so route
``stream`` keeps nothing resident: stage 1 only opens the pileups, and the consensus stage is one streamed call per group of
samples whose kernels leave their rows where the flow kernels read them (Device.call_consensus_files_dev).  Every file must be
what the separate subcommands write, whatever the route; ``auto`` takes the stream route exactly where the resident route would
read files a second time.
"""
import json
import os
import socket
import subprocess
import sys

import pytest

import test_gpu_pipeline as tp

pytestmark = pytest.mark.gpu

FILTER_EXTRA = "--edge_length 100 --window_size 1000 125 15 --max_snp 3 2 1 --mode all"
OUTPUTS = tuple(n for n in tp.PER_SAMPLE if n != "var.flt.vcf")          # what a job in mode ``existing`` writes per sample


def _line(dirs_file, ref_path, more=""):
    return ("hot_path_batch -f %s %s --filterRegionsExtraParams=%s --callConsensusExtraParams=%s --siteCalling existing%s"
            % (dirs_file, ref_path, FILTER_EXTRA.replace(" ", "\x00"), tp.CONSENSUS_EXTRA.replace(" ", "\x00"), more))


def _clear_outputs(work, dirs):
    """Everything a job writes goes away (var.flt.vcf stays: in mode ``existing`` it is an input), so that no file of an earlier
    run can stand in for one this run should have written."""
    for sdir in dirs:
        for name in OUTPUTS + ("metrics",):
            if os.path.exists(os.path.join(sdir, name)):
                os.remove(os.path.join(sdir, name))
    for name in tp.TOP_LEVEL + ("metrics.tsv", "error.log"):
        if os.path.exists(os.path.join(str(work), name)):
            os.remove(os.path.join(str(work), name))


class _Tree(object):
    pass


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """The outbreak tree (6 samples, 12 kbp) and what the separate subcommands write for it: made once, shared by the tests that
    only run jobs on it (a job in mode ``existing`` never touches its inputs)."""
    t = _Tree()
    t.work = tmp_path_factory.mktemp("one_pass")
    t.ref_path, t.dirs, t.dirs_file, t.piles = tp._outbreak_tree(t.work)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("VarscanMpileup2snp_ExtraParams", tp.VARSCAN_EXTRA)
        mp.chdir(t.work)
        tp._separate_steps(t.work, t.ref_path, t.dirs, t.dirs_file, FILTER_EXTRA, "")
    t.want = tp._snapshot(t.work, t.dirs, remove=False)
    t.total = sum(len(p) for p in t.piles)
    assert len(t.want["snplist.txt"].splitlines()) > len(t.want["snplist_preserved.txt"].splitlines()) > 10
    return t


def _job(tree, monkeypatch, more):
    from snp_pipeline_amd import hot_path
    monkeypatch.chdir(tree.work)
    _clear_outputs(tree.work, tree.dirs)
    tp._run(_line(tree.dirs_file, tree.ref_path, more))
    return dict(hot_path.hot_path_batch.last_stats)


def test_stream_route_equals_the_separate_steps(tree, monkeypatch):
    st = _job(tree, monkeypatch, " --pileupRoute stream")
    tp._compare(tp._snapshot(tree.work, tree.dirs, remove=False), tree.want)
    assert st["pileup_route"] == "stream"
    assert st["h2d_bytes"] == st["file_bytes"] == tree.total          # every pileup crossed the host link exactly once
    assert st["resident_files"] == 0 and st["files"] == len(tree.dirs) and st["vcf_again"] == 0


def test_auto_takes_the_stream_route_past_the_budget(tree, monkeypatch):
    """Two of the six pileups fit the budget: the resident route would read the other four a second time."""
    st = _job(tree, monkeypatch, " --pileupRoute auto --residentBytes %d" % int(2.5 * max(len(p) for p in tree.piles)))
    tp._compare(tp._snapshot(tree.work, tree.dirs, remove=False), tree.want)
    assert st["pileup_route"] == "stream"
    assert st["h2d_bytes"] == tree.total and st["file_bytes"] == tree.total and st["resident_files"] == 0


def test_auto_from_the_environment_keeps_the_resident_route_when_everything_fits(tree, monkeypatch):
    monkeypatch.setenv("SNPGPU_PILEUP_ROUTE", "auto")
    st = _job(tree, monkeypatch, "")
    tp._compare(tp._snapshot(tree.work, tree.dirs, remove=False), tree.want)
    assert st["pileup_route"] == "resident"
    assert st["resident_files"] == len(tree.dirs) and st["h2d_bytes"] == tree.total
    # the variable alone picks the route, and an explicit resident route past the budget is today's job
    monkeypatch.setenv("SNPGPU_PILEUP_ROUTE", "stream")
    assert _job(tree, monkeypatch, "")["pileup_route"] == "stream"
    monkeypatch.delenv("SNPGPU_PILEUP_ROUTE")
    st = _job(tree, monkeypatch, " --pileupRoute resident --residentBytes %d" % int(2.5 * max(len(p) for p in tree.piles)))
    assert st["pileup_route"] == "resident" and 0 < st["resident_files"] < len(tree.dirs) and st["h2d_bytes"] > tree.total
    tp._compare(tp._snapshot(tree.work, tree.dirs, remove=False), tree.want)


def test_stream_route_is_refused_in_mode_device(tree, monkeypatch, capfd):
    monkeypatch.chdir(tree.work)
    monkeypatch.setenv("errorOutputFile", str(tree.work / "refused.log"))
    line = _line(tree.dirs_file, tree.ref_path, " --pileupRoute stream").replace("--siteCalling existing", "--siteCalling device")
    with pytest.raises(SystemExit) as ei:
        tp._run(line)
    assert ei.value.code == 100
    assert "--pileupRoute stream" in capfd.readouterr().err
    if os.path.exists(str(tree.work / "refused.log")):
        os.remove(str(tree.work / "refused.log"))


def test_collect_metrics_on_the_stream_route_equals_the_resident_route(tree, monkeypatch):
    merged = str(tree.work / "metrics.tsv")
    got = {}
    for route in ("resident", "stream"):
        st = _job(tree, monkeypatch, " --pileupRoute %s --collectMetrics --mergedMetricsFile %s" % (route, merged))
        assert st["pileup_route"] == route
        tp._compare(tp._snapshot(tree.work, tree.dirs, remove=False), tree.want)
        got[route] = ({d: open(os.path.join(d, "metrics")).read() for d in tree.dirs}, open(merged).read(), st["collect_metrics"])
    assert got["stream"][0] == got["resident"][0] and got["stream"][1] == got["resident"][1]
    assert "avePileupDepth=" in got["stream"][0][tree.dirs[0]]
    assert got["stream"][2] == got["resident"][2] and got["stream"][2]["depth_fallbacks"] == 0 and got["stream"][2]["pileups_summed"] == 0
    _clear_outputs(tree.work, tree.dirs)


def test_stream_route_sharded_over_two_ranks_writes_the_same_files(tree, monkeypatch):
    """Two ranks on the one GPU of the test box with gloo moving the bytes (as the sharded test of the resident route): every
    rank streams its own block of samples."""
    _clear_outputs(tree.work, tree.dirs)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    stats_dir = tree.work / "stats"
    stats_dir.mkdir()
    env = dict(os.environ, SNPGPU_PIPELINE_ONE_GPU="1", MASTER_ADDR="127.0.0.1", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""),
               SNPGPU_HOT_PATH_STATS=str(stats_dir))
    line = _line(tree.dirs_file, tree.ref_path, " --pileupRoute stream")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "bin", "cfsan_snp_pipeline")] + [w.replace("\x00", " ") for w in line.split()] + ["-v", "0"]
    r = subprocess.run(cmd, cwd=str(tree.work), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    tp._compare(tp._snapshot(tree.work, tree.dirs, remove=False), tree.want)
    per_rank = [json.load(open(str(stats_dir / ("rank%d.json" % k)))) for k in range(2)]
    assert [st["pileup_route"] for st in per_rank] == ["stream", "stream"]
    assert sum(st["h2d_bytes"] for st in per_rank) == tree.total and [st["files"] for st in per_rank] == [3, 3]


def test_many_symbols_on_the_stream_route_need_no_second_read(tmp_path, monkeypatch):
    """A listed position with 24 distinct symbols in two samples (the scenario of the partly resident job in test_gpu_pipeline):
    the spill records of all files of a streamed group are one arena, so the group writes those samples' VCF rows itself."""
    from snp_pipeline_amd import hot_path
    work = tmp_path
    ref_path, dirs, dirs_file, piles = tp._outbreak_tree(work)
    monkeypatch.setenv("VarscanMpileup2snp_ExtraParams", tp.VARSCAN_EXTRA)
    monkeypatch.chdir(work)
    for sdir in dirs:
        tp._run("call_sites %s %s" % (ref_path, sdir))
    tp._run("merge_sites -f -n var.flt.vcf -o %s/probe.txt %s %s.probe" % (work, dirs_file, dirs_file))
    chrom, pos = next((f[0], int(f[1])) for f in (ln.split("\t") for ln in open(str(work / "probe.txt"))) if int(f[2]) >= 3)
    for sdir in (dirs[-1], dirs[0]):
        path = os.path.join(sdir, "reads.all.pileup")
        lines = open(path, "rb").read().split(b"\n")
        k = next(i for i, ln in enumerate(lines) if ln.startswith(b"%s\t%d\t" % (chrom.encode(), pos)))
        f = lines[k].split(b"\t")
        f[3], f[4], f[5] = b"24", b"ACGTNRYKMSWBacgtnrykmswb", b"I" * 24
        lines[k] = b"\t".join(f)
        open(path, "wb").write(b"\n".join(lines))
    tp._separate_steps(work, ref_path, dirs, dirs_file, FILTER_EXTRA, "")
    want = tp._snapshot(work, dirs, remove=False)
    row = next(ln for ln in want[os.path.join(os.path.basename(dirs[-1]), "consensus.vcf")].split(b"\n") if ln.startswith(b"%s\t%d\t" % (chrom.encode(), pos)))
    assert row.split(b"\t")[4].count(b",") >= 9                   # ten or more ALT alleles in that row
    _clear_outputs(work, dirs)
    tp._run(_line(dirs_file, ref_path, " --pileupRoute stream"))
    tp._compare(tp._snapshot(work, dirs, remove=False), want)
    st = hot_path.hot_path_batch.last_stats
    assert st["pileup_route"] == "stream" and st["vcf_again"] == 0 and st["h2d_bytes"] == st["file_bytes"]


def test_an_unreadable_pileup_fails_its_sample_before_the_site_union_on_either_route(tmp_path, monkeypatch):
    """StopOnSampleError=false.  The resident route learns from the ingest that a pileup cannot be read and goes on without the
    sample: its records are in neither site list.  The stream route reads no pileup before the lists are written, so it opens
    every one in stage 1: same error log, same files."""
    from snp_pipeline_amd import cfsan_snp_pipeline as cli
    work = tmp_path
    ref_path, dirs, dirs_file, piles = tp._outbreak_tree(work)
    monkeypatch.setenv("VarscanMpileup2snp_ExtraParams", tp.VARSCAN_EXTRA)
    monkeypatch.setenv("StopOnSampleError", "false")
    log = work / "error.log"
    monkeypatch.setenv("errorOutputFile", str(log))
    monkeypatch.chdir(work)
    for sdir in dirs:
        tp._run("call_sites %s %s" % (ref_path, sdir))
    bad = os.path.join(dirs[2], "reads.all.pileup")
    stamp = os.stat(bad)
    os.chmod(bad, 0)
    readable_anyway = os.access(bad, os.R_OK)                    # (a privileged user reads every file: a directory in its place then)
    if readable_anyway:
        os.remove(bad)
        os.mkdir(bad)
        os.utime(bad, ns=(stamp.st_atime_ns, stamp.st_mtime_ns))
    good = [d for d in dirs if d != dirs[2]]

    def run(more):
        _clear_outputs(work, dirs)
        args = cli.parse_argument_list([w.replace("\x00", " ") for w in _line(dirs_file, ref_path, more).split()])
        args.verbose = 0
        try:
            rc = cli.run_command_from_args(args)
        except SystemExit as e:
            rc = e.code
        assert rc in (0, 98), rc                                 # 98 = "a sample failed, the others went on"
        files = tp._snapshot(work, good, remove=False)
        left = sorted(n for n in os.listdir(dirs[2]) if n in OUTPUTS)
        return files, log.read_text(), left

    try:
        want_files, want_log, want_left = run(" --pileupRoute resident")
        got_files, got_log, got_left = run(" --pileupRoute stream")
    finally:
        if not readable_anyway:
            os.chmod(bad, 0o644)
    assert os.path.basename(dirs[2]) in want_log
    assert got_log == want_log
    tp._compare(got_files, want_files)
    assert got_left == want_left
    assert os.path.basename(dirs[2]).encode() not in got_files["snpma.fasta"]
