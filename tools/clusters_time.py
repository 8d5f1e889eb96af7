#!/usr/bin/env python3
"""What the close-pairs and clusters outputs of the distance step cost on one GPU (profiles/r16/clusters.md):

  1. the two kernels of csrc/clusters.hip alone on a planted-groups matrix (events around the calls): the thresholded rows
     (count pass + scan, then count + emit) and the connected components at six thresholds;
  2. wall time of `distance` (a fresh process per run, the input in the page cache) with only the new outputs, against the same
     command with `-p -m`: medians of --runs runs after a warm-up, with the spread.

    python tools/clusters_time.py [--samples 10000] [--sites 200000] [--group 25] [--runs 3] [--out result.json]

Planted groups: every group of --group samples shares a centre that differs from the base sequence at 1 % of the sites; a member
differs from its centre at 0 ... 12 sites — so pairs inside a group lie within about 24 SNPs and pairs across groups thousands apart.
"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
THRESHOLDS = [0, 2, 5, 10, 20, 50]


def _spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": xs}


def planted(n, s, group, seed=1):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    base = rng.integers(0, 4, size=s, dtype=np.uint8)
    code = np.empty((n, s), dtype=np.uint8)
    for g0 in range(0, n, group):
        centre = base.copy()
        at = rng.choice(s, size=max(1, s // 100), replace=False)
        centre[at] = (centre[at] + rng.integers(1, 4, size=len(at), dtype=np.uint8)) & 3
        code[g0:g0 + group] = centre
        for r in range(g0, min(n, g0 + group)):
            at = rng.integers(0, s, size=int(rng.integers(0, 13)))
            code[r, at] = (code[r, at] + 1) & 3
    return acgt[code]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--sites", type=int, default=200000)
    ap.add_argument("--group", type=int, default=25)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--skip-tables", action="store_true", help="do not time the -p -m run (3 GB of text at 10 000 samples)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from snp_pipeline_amd import device as dev
    n, s = a.samples, a.sites
    sym = planted(n, s, a.group)
    print("planted %d x %d" % (n, s), file=sys.stderr, flush=True)
    result = {"samples": n, "sites": s, "group": a.group, "runs": a.runs, "thresholds": THRESHOLDS}
    d = dev.Device(0)
    d.use_torch_stream()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    # ---- the kernels alone ------------------------------------------------------------------------------------------------
    sym_t = torch.from_numpy(sym).cuda()
    packed = torch.zeros((n, d.packed_row_bytes(s)), dtype=torch.uint8, device="cuda")
    d.pack_matrix_dev(sym_t.data_ptr(), n, s, s, packed.data_ptr())
    del sym_t
    mat = torch.zeros((n, n), dtype=torch.int32, device="cuda")
    ms_dist = [timed(lambda: d.distance_packed_dev(packed.data_ptr(), n, s, mat.data_ptr()))[0] for _ in range(a.runs + 1)]
    widest = max(THRESHOLDS)
    total = d.close_pairs_dev(mat.data_ptr(), n, n, 0, n, widest)
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    col = torch.zeros(max(total, 1), dtype=torch.int32, device="cuda")
    dist = torch.zeros(max(total, 1), dtype=torch.int32, device="cuda")
    numbers = torch.zeros((len(THRESHOLDS), n), dtype=torch.int32, device="cuda")
    ms_count, ms_emit, ms_cc = [], [], []
    for rep in range(a.runs + 1):
        ms_count.append(timed(lambda: d.close_pairs_dev(mat.data_ptr(), n, n, 0, n, widest))[0])
        ms_emit.append(timed(lambda: d.close_pairs_dev(mat.data_ptr(), n, n, 0, n, widest, total, off.data_ptr(), col.data_ptr(), dist.data_ptr()))[0])
        ms, counts = timed(lambda: d.clusters_dev(n, off.data_ptr(), col.data_ptr(), dist.data_ptr(), total, THRESHOLDS, numbers.data_ptr()))
        ms_cc.append(ms)
    result.update(distance_kernel_ms=_spread(ms_dist[1:]), entries_within_widest=int(total), clusters_per_threshold=[int(c) for c in counts],
                  rows_count_and_scan_ms=_spread(ms_count[1:]), rows_count_scan_emit_ms=_spread(ms_emit[1:]), components_ms=_spread(ms_cc[1:]),
                  matrix_GB_per_s_count_pass=n * n * 4 / (statistics.median(ms_count[1:]) * 1e-3) / 1e9)
    del mat, packed, off, col, dist, numbers
    print("kernels timed", file=sys.stderr, flush=True)
    d.close()

    # ---- the command ------------------------------------------------------------------------------------------------------
    tmp = tempfile.mkdtemp(prefix="snpclusters_")
    try:
        fasta = os.path.join(tmp, "snpma.fasta")
        with open(fasta, "wb") as f:
            for r in range(n):
                f.write(b">s%06d\n" % r)
                f.write(sym[r].tobytes())
                f.write(b"\n")
        exe = os.path.join(ROOT, "bin", "cfsan_snp_pipeline")
        new = ["--amdClosePairs", os.path.join(tmp, "close.tsv"), "--amdMaxPairDistance", "20", "--amdClusters", os.path.join(tmp, "clusters.tsv"),
               "--amdClusterThresholds"] + [str(t) for t in THRESHOLDS]
        tables = ["-p", os.path.join(tmp, "pairwise.tsv"), "-m", os.path.join(tmp, "matrix.tsv")]
        for label, opts in (("new_outputs_only", new),) + (() if a.skip_tables else (("tables_p_m", tables),)):
            cmd = [sys.executable, exe, "distance", "-v", "0", "-f", fasta] + opts
            wall = []
            for rep in range(a.runs + 1):
                t0 = time.perf_counter()
                r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, SNPGPU_DEVICE="0"))
                wall.append(time.perf_counter() - t0)
                assert r.returncode == 0, r.stderr[-2000:]
                print("%s run %d: %.2f s" % (label, rep, wall[-1]), file=sys.stderr, flush=True)
            result["distance_wall_s_" + label] = _spread(wall[1:])
            result["bytes_written_" + label] = sum(os.path.getsize(p) for p in opts if p.startswith(tmp))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    text = json.dumps(result, indent=1, sort_keys=True)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
