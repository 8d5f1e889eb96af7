"""The timing helpers of tools/ at toy sizes: they are the lab notebook behind DESIGN.md's numbers and had no test (VERDICT r3 weak
#9); a helper that no longer runs against the current library is found here, not in the next tuning session."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("argv, expect", [
    (["scan_tune.py", "3", "60000", "batch", "20"], "scan "),
    (["scan_tune.py", "2", "60000", "single", "20"], "scan "),
    (["varscan_kernel_time.py", "200000", "30", "2"], "records:"),
    (["varscan_kernel_time.py", "200000", "30", "2", "3"], "batch of 3 samples"),
    (["varscan_time.py", "200000", "30", "1"], ""),
    (["varscan_files_time.py", "3", "1"], ""),
    (["pipeline_time.py", "--samples", "4", "--genome", "60000", "--sites", "600", "--separate", "--resident-frac", "0.5"], "outputs_identical_to_fully_resident\": true"),
    (["host_steps_time.py", "30", "2000"], ""),
    (["merge_scale.py", "50", "60", "2000"], ""),
    (["distance_cli_time.py", "60", "900"], ""),
    (["scan_multi_contig.py", "5", "20000", "2"], ""),
    (["scan_multi_contig.py", "6", "20000", "2", "draft", "all"], "names draft"),
    (["k2_exp.py"], "call kernels"),
    (["scan_crlf.py"], ""),
    (["scan_sweep.py", "3", "20", "", "OVERSUB=1"], "GB/s"),
])
def test_tool_runs_at_toy_size(argv, expect, tmp_path):
    env = dict(os.environ, TMPDIR=str(tmp_path), SWEEP_GENOME="60000")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", argv[0])] + argv[1:], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (argv, r.stdout[-1500:], r.stderr[-2500:])
    assert expect in r.stdout, (argv, r.stdout[-1500:])


def test_bench_prints_one_compact_line_last(tmp_path):
    """The driver parses a bounded tail of bench.py's stdout (BENCH_r05: a 20 KB line came back as `parsed: null`).  With every side
    row switched on, at toy sizes: the LAST stdout line is one JSON object under 4 KB that carries the contract's keys, `roofline`
    and `cpu_baseline`; the detail file holds the side rows the compact line quotes from."""
    import json
    detail = str(tmp_path / "detail.json")
    argv = ["--steps", "2", "--warmup", "1", "--samples", "4", "--genome", "60000", "--sites", "600", "--vcf-records", "60", "--dist-samples", "300",
            "--dist-sites", "2000", "--dist-reps", "1", "--cpu-samples", "2", "--cpu-procs", "2", "--cpu-dist-samples", "20", "--site-files", "2", "--e2e-files", "2",
            "--pipeline-files", "4", "--shape-samples", "2", "--detail", detail, "--full"]
    env = dict(os.environ, TMPDIR=str(tmp_path))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-2500:])
    lines = r.stdout.splitlines()
    assert len(lines[-1].encode()) < 4096
    line = json.loads(lines[-1])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
                "roofline", "cpu_baseline"):
        assert key in line, key
    assert line["n_gpus"] == 1 and line["steps"] == 2 and line["warmup"] == 1 and line["value"] > 0 and line["vs_baseline"] is None
    assert "workload" in line["config"] and "model" not in line["config"]
    roof = line["roofline"]
    assert roof["bound"] == "hbm" and roof["unit"] == "GB/s" and roof["peak"] == 8000.0 and roof["frac"] == pytest.approx(roof["achieved"] / roof["peak"], rel=1e-4)
    assert roof["launches"] == 2 and roof["avg_launch_ms"] > 0
    # the scan's HBM traffic is measured in the run itself (two child runs under rocprofv3 --pmc): at least the bytes of the text, and not
    # the multiple a re-reading kernel would show; where rocprofv3 cannot run the line says why and carries no live figure
    with open(detail) as f:
        roof_full = json.load(f)["roofline"]
    if "traffic_live_error" in roof_full:
        print("live traffic not measured here:", roof_full["traffic_live_error"])
        assert roof.get("traffic_is") != "measured in this run"
    else:
        assert roof["traffic_is"] == "measured in this run" and roof_full["traffic_launches_measured"] == 4
        assert 0.9 < roof["traffic_over_algorithmic"] < 3.0           # (toy samples: the edge tiles and the site set weigh more than at full size)
    cb = line["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] == 1 and cb["value"] > 0 and cb["matches_gpu"] is True and cb["sample"]
    assert cb["parallel"]["matches_gpu"] is True and cb["distance"]["matches_gpu"] is True
    assert "side_rows_with_errors" not in line, line["side_rows_with_errors"]
    with open(detail) as f:
        full = json.load(f)
    for row in ("pipeline_from_files", "secondary", "aux_steps_ms", "scan_shapes", "end_to_end", "call_variants", "site_calling", "cpu_baseline", "north_star"):
        assert row in full and "error" not in full[row], (row, full.get(row))
    assert line["value"] == pytest.approx(full["value"], rel=1e-5) and line["k2_frac"] == pytest.approx(full["call_variants"]["strict"]["roofline"]["frac"], rel=1e-5)
    assert line["site_calling_frac"] == pytest.approx(full["site_calling"]["roofline"]["frac"], rel=1e-5)


def test_plain_bench_run_is_the_headline_alone_and_dumps_its_outputs(tmp_path):
    """Without --full the run is the headline and nothing else: no side row, no detail file; --steps sets the timed steps and
    --dump-outputs writes what the last step computed.  Two runs with the same arguments dump the same arrays."""
    import json
    import numpy as np
    argv = ["--steps", "3", "--warmup", "1", "--samples", "4", "--genome", "60000", "--sites", "600", "--vcf-records", "60",
            "--detail", str(tmp_path / "detail.json")]
    env = dict(os.environ, TMPDIR=str(tmp_path))
    dumped = []
    for k in range(2):
        out = tmp_path / ("out%d" % k)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv + ["--dump-outputs", str(out)], cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-2500:])
        line = json.loads(r.stdout.splitlines()[-1])
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
        assert line["roofline"]["launches"] == 3
        for key in ("cpu_baseline", "secondary", "pipeline_from_files", "end_to_end", "scan_shapes", "detail"):
            assert key not in line, key
        assert not os.path.exists(str(tmp_path / "detail.json"))
        dumped.append({f: np.load(str(out / f)) for f in sorted(os.listdir(str(out)))})
    assert sorted(dumped[0]) == ["consensus_bases.npy", "consensus_filters.npy", "distance_rows.npy", "site_union_carriers.npy",
                                 "site_union_keys.npy", "site_union_offsets.npy"]
    for name, a in dumped[0].items():
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, dumped[1][name]), name
    bases = dumped[0]["consensus_bases.npy"]
    assert bases.shape == (4, line["config"]["snp_sites"]) and 33 <= bases.min() and bases.max() <= 126          # printable bytes: bases or '-'
    assert dumped[0]["distance_rows.npy"].shape == (4, 4)
    assert len(dumped[0]["site_union_offsets.npy"]) == len(dumped[0]["site_union_keys.npy"]) + 1 <= line["config"]["snp_sites"] + 1
