#!/usr/bin/env python3
"""What the minimum spanning tree of the distance step costs on one GPU (profiles/r17/mst.md):

  0. outside every timed region, at --check-samples samples: the device tree must equal snpgpu_mst_of_edges (Kruskal on the host)
     over the CSR of every entry of the matrix (the close-pairs rows at INT_MAX);
  1. the call snpgpu_mst_dev alone on a planted-groups matrix (events around the call, its waits for the stream included) and
     its round count, beside k_distance in the same run; the whole matrix, and the first third of its rows as a band;
  2. wall time of `distance` (a fresh process per run, the input in the page cache) with only --amdMst --amdDendrogram, against
     the same command with `-p -m`: medians of --runs runs after a warm-up, with the spread.

    python tools/mst_time.py [--samples 10000] [--sites 200000] [--group 25] [--runs 3] [--out result.json]

The planted groups are those of tools/clusters_time.py."""
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
INT_MAX = 2 ** 31 - 1


def _spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": xs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--sites", type=int, default=200000)
    ap.add_argument("--group", type=int, default=25)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--check-samples", type=int, default=1500)
    ap.add_argument("--skip-tables", action="store_true", help="do not time the -p -m run (3 GB of text at 10 000 samples)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    import torch
    from clusters_time import planted
    from snp_pipeline_amd import device as dev
    from snp_pipeline_amd import distance as dmod
    n, s = a.samples, a.sites
    sym = planted(n, s, a.group)
    print("planted %d x %d" % (n, s), file=sys.stderr, flush=True)
    result = {"samples": n, "sites": s, "group": a.group, "runs": a.runs}
    d = dev.Device(0)
    d.use_torch_stream()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    def matrix_of(rows):
        k = len(rows)
        sym_t = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
        packed = torch.zeros((k, d.packed_row_bytes(s)), dtype=torch.uint8, device="cuda")
        d.pack_matrix_dev(sym_t.data_ptr(), k, s, s, packed.data_ptr())
        mat = torch.zeros((k, k), dtype=torch.int32, device="cuda")
        return packed, mat

    def tree_of(mat, k, lo, hi, out):
        return d.mst_dev(mat.data_ptr(), k, k, lo, hi, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr())

    # ---- the check, outside every timed region ------------------------------------------------------------------------------
    k = min(a.check_samples, n)
    packed, mat = matrix_of(sym[:: max(n // k, 1)][:k])
    d.distance_packed_dev(packed.data_ptr(), k, s, mat.data_ptr())
    out = [torch.zeros(max(k - 1, 1), dtype=torch.int32, device="cuda") for _ in range(3)]
    n_edges, rounds = tree_of(mat, k, 0, k, out)
    total = d.close_pairs_dev(mat.data_ptr(), k, k, 0, k, INT_MAX)
    assert total == k * k
    off = torch.zeros(k + 1, dtype=torch.int64, device="cuda")
    col = torch.zeros(total, dtype=torch.int32, device="cuda")
    dist = torch.zeros(total, dtype=torch.int32, device="cuda")
    d.close_pairs_dev(mat.data_ptr(), k, k, 0, k, INT_MAX, total, off.data_ptr(), col.data_ptr(), dist.data_ptr())
    h_col, h_dist = col.cpu().numpy().view(np.uint32), dist.cpu().numpy()
    h_row = np.repeat(np.arange(k, dtype=np.uint32), np.diff(off.cpu().numpy()))
    off_diagonal = h_row != h_col
    want = dmod.mst_of_edges(k, h_row[off_diagonal], h_col[off_diagonal], h_dist[off_diagonal])
    got = [o[:n_edges].cpu().numpy() for o in out]
    assert n_edges == k - 1 and rounds <= max(k - 1, 0).bit_length()
    assert np.array_equal(got[0].view(np.uint32), want[0]) and np.array_equal(got[1].view(np.uint32), want[1]) and np.array_equal(got[2], want[2])
    result.update(check_samples=k, check_rounds=rounds, check_tree_weight=int(want[2].astype(np.int64).sum()))
    print("device tree == host Kruskal over the full CSR at %d samples (%d rounds)" % (k, rounds), file=sys.stderr, flush=True)
    del packed, mat, out, off, col, dist

    # ---- the call alone -------------------------------------------------------------------------------------------------------
    packed, mat = matrix_of(sym)
    out = [torch.zeros(max(n - 1, 1), dtype=torch.int32, device="cuda") for _ in range(3)]
    band_hi = (n + 2) // 3
    ms_dist, ms_tree, ms_band, ms_tree_cold = [], [], [], []
    for rep in range(a.runs + 1):
        ms_dist.append(timed(lambda: d.distance_packed_dev(packed.data_ptr(), n, s, mat.data_ptr()))[0])
        ms, (n_edges, rounds) = timed(lambda: tree_of(mat, n, 0, n, out))              # right behind k_distance: part of the matrix is still in cache
        ms_tree_cold.append(ms)
        ms, (n_edges, rounds) = timed(lambda: tree_of(mat, n, 0, n, out))
        ms_tree.append(ms)
        ms, (band_edges, band_rounds) = timed(lambda: tree_of(mat, n, 0, band_hi, out))
        ms_band.append(ms)
    n_edges, rounds = tree_of(mat, n, 0, n, out)
    weight = int(out[2][:n_edges].cpu().numpy().astype(np.int64).sum())
    assert n_edges == n - 1 and band_edges == n - 1
    result.update(distance_kernel_ms=_spread(ms_dist[1:]), mst_call_after_distance_ms=_spread(ms_tree_cold[1:]), mst_call_ms=_spread(ms_tree[1:]),
                  mst_rounds=rounds, mst_edges=n_edges, mst_weight=weight, band_rows=band_hi, mst_band_call_ms=_spread(ms_band[1:]), mst_band_rounds=band_rounds,
                  matrix_GB_read_per_round=n * n * 4 / 1e9)
    del mat, packed, out
    print("call timed", file=sys.stderr, flush=True)
    d.close()

    # ---- the command ------------------------------------------------------------------------------------------------------------
    tmp = tempfile.mkdtemp(prefix="snpmst_")
    try:
        fasta = os.path.join(tmp, "snpma.fasta")
        with open(fasta, "wb") as f:
            for r in range(n):
                f.write(b">s%06d\n" % r)
                f.write(sym[r].tobytes())
                f.write(b"\n")
        exe = os.path.join(ROOT, "bin", "cfsan_snp_pipeline")
        new = ["--amdMst", os.path.join(tmp, "mst.tsv"), "--amdDendrogram", os.path.join(tmp, "dendrogram.nwk")]
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
