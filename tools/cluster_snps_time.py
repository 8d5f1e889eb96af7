#!/usr/bin/env python3
"""What the per-site allele counts and the cluster-defining SNPs of the distance step cost on one GPU (profiles/r23/cluster_snps.md):

  0. outside every timed region, at --check-samples samples: the counts and the cluster SNPs must be what NumPy finds column by
     column;
  1. events around each call, in one run: k_distance (snpgpu_distance_packed_dev), the site counts (snpgpu_site_counts_dev), and
     snpgpu_cluster_snps_dev for the single-linkage clusters of that matrix at every threshold of tools/clusters_time.py —
     the count alone (capacity 0) and the count with the emit — each beside its bound: the sweeps over the packed matrix times
     its bytes over the 6.3 TB/s copy ceiling.  A call of snpgpu_cluster_snps_dev allocates and frees its workspace and waits for
     the stream three times; all of that is inside its events;
  2. wall time of `distance` (a fresh process per run, the input in the page cache) with only --amdSiteCounts, with only
     --amdClusterSnps, and (unless --skip-tables) with -p -m: medians of --runs runs after a warm-up, with the spread.

    python tools/cluster_snps_time.py [--samples 10000] [--sites 200000] [--group 25] [--runs 3] [--out result.json]

The planted groups are those of tools/clusters_time.py (--group 25: 400 groups of 10 000 samples); every sample then loses up to
--missing of its columns to '-' and 'N'."""
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
HBM_BYTES_PER_S = 6.3e12                # the measured copy ceiling
SWEEPS = {"site_counts": 1, "cluster_snps": 1}      # passes over the packed matrix per call (csrc/cluster_snps.hip)


def _spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": xs}


def codes_of(sym):
    up = np.where((sym >= 97) & (sym <= 122), sym - 32, sym).astype(np.uint8)
    code = np.full(sym.shape, -1, dtype=np.int8)
    for b, letter in enumerate(b"ACGT"):
        code[up == letter] = b
    return code


def snps_of(code, labels, n_clusters):
    """[(cluster, site, base, members)] by cluster, then site: the statement of csrc/cluster_snps.hip, column-wise in NumPy."""
    holds = np.stack([code == b for b in range(4)])
    everywhere = holds.sum(axis=1)
    out = []
    for c in range(1, n_clusters + 1):
        inside = holds[:, labels == c, :].sum(axis=1)
        cols = np.flatnonzero((inside > 0).sum(axis=0) == 1)
        b = np.argmax(inside[:, cols], axis=0)
        keep = inside[b, cols] == everywhere[b, cols]
        out += [(c, int(s), int(x), int(m)) for s, x, m in zip(cols[keep], b[keep], inside[b, cols][keep])]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--sites", type=int, default=200000)
    ap.add_argument("--group", type=int, default=25)
    ap.add_argument("--missing", type=float, default=0.1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--check-samples", type=int, default=200)
    ap.add_argument("--skip-command", action="store_true")
    ap.add_argument("--skip-tables", action="store_true", help="do not time the -p -m run (3 GB of text at 10 000 samples)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    import torch
    from clusters_time import THRESHOLDS, planted
    from compared_time import with_missing
    from snp_pipeline_amd import device as dev
    n, s = a.samples, a.sites
    sym = with_missing(planted(n, s, a.group), a.missing)
    print("planted %d x %d, up to %.0f %% of a row missing" % (n, s, 100 * a.missing), file=sys.stderr, flush=True)
    result = {"samples": n, "sites": s, "group": a.group, "missing": a.missing, "runs": a.runs, "thresholds": THRESHOLDS, "sweeps": SWEEPS}
    d = dev.Device(0)
    d.use_torch_stream()
    packed_row = d.packed_row_bytes(s)
    result.update(cu=torch.cuda.get_device_properties(0).multi_processor_count, packed_bytes=n * packed_row)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    def several(fn):
        return _spread([timed(fn)[0] for _ in range(a.runs + 1)][1:])

    def pack(rows):
        k = len(rows)
        sym_t = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
        packed = torch.zeros((k, packed_row), dtype=torch.uint8, device="cuda")
        d.pack_matrix_dev(sym_t.data_ptr(), k, s, s, packed.data_ptr())
        torch.cuda.synchronize()
        return packed

    def clusters_of(packed, k):
        """(numbers (T, k) on the host, clusters per threshold, the distance matrix on the device)."""
        mat = torch.zeros((k, k), dtype=torch.int32, device="cuda")
        d.distance_packed_dev(packed.data_ptr(), k, s, mat.data_ptr())
        widest = max(THRESHOLDS)
        total = d.close_pairs_dev(mat.data_ptr(), k, k, 0, k, widest)
        off = torch.zeros(k + 1, dtype=torch.int64, device="cuda")
        col = torch.zeros(max(total, 1), dtype=torch.int32, device="cuda")
        dist = torch.zeros(max(total, 1), dtype=torch.int32, device="cuda")
        d.close_pairs_dev(mat.data_ptr(), k, k, 0, k, widest, total, off.data_ptr(), col.data_ptr(), dist.data_ptr())
        numbers = torch.zeros((len(THRESHOLDS), k), dtype=torch.int32, device="cuda")
        counts = d.clusters_dev(k, off.data_ptr(), col.data_ptr(), dist.data_ptr(), total, THRESHOLDS, numbers.data_ptr())
        torch.cuda.synchronize()
        return numbers, [int(c) for c in counts], mat

    def snps(packed, k, labels_t, n_clusters, capacity=0, out=None):
        args = (out["off"].data_ptr(), out["site"].data_ptr(), out["base"].data_ptr(), out["members"].data_ptr()) if capacity else (0, 0, 0, 0)
        return d.cluster_snps_dev(packed.data_ptr(), k, s, labels_t.data_ptr(), n_clusters, capacity, *args)

    def room(n_clusters, total):
        return {"off": torch.zeros(n_clusters + 1, dtype=torch.int64, device="cuda"), "site": torch.zeros(max(total, 1), dtype=torch.int32, device="cuda"),
                "base": torch.zeros(max(total, 1), dtype=torch.uint8, device="cuda"), "members": torch.zeros(max(total, 1), dtype=torch.int32, device="cuda")}

    # ---- the check, outside every timed region ------------------------------------------------------------------------------
    k = min(a.check_samples, n)
    rows = sym[:: max(n // k, 1)][:k]
    code = codes_of(rows)
    pk = pack(rows)
    counts_t = torch.full((s, 4), -1, dtype=torch.int32, device="cuda")
    d.site_counts_dev(pk.data_ptr(), k, s, counts_t.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(counts_t.cpu().numpy(), np.stack([(code == b).sum(axis=0) for b in range(4)], axis=1))
    numbers, n_clusters, _ = clusters_of(pk, k)
    for t in (0, len(THRESHOLDS) - 1):
        labels = numbers[t].cpu().numpy()
        want = snps_of(code, labels, n_clusters[t])
        total = snps(pk, k, numbers[t], n_clusters[t])
        out = room(n_clusters[t], total)
        assert snps(pk, k, numbers[t], n_clusters[t], max(total, 1), out) == total == len(want)
        off = out["off"].cpu().numpy()
        got = list(zip(np.repeat(np.arange(1, n_clusters[t] + 1), np.diff(off)).tolist(), out["site"].cpu().numpy()[:total].tolist(),
                       out["base"].cpu().numpy()[:total].tolist(), out["members"].cpu().numpy()[:total].tolist()))
        assert got == want
    result.update(check_samples=k)
    print("counts and cluster SNPs == NumPy at %d samples" % k, file=sys.stderr, flush=True)
    del pk, counts_t, numbers

    # ---- the calls alone ------------------------------------------------------------------------------------------------------
    pk = pack(sym)
    bound_ms = n * packed_row / HBM_BYTES_PER_S * 1e3
    result["sweep_bound_ms"] = bound_ms
    mat = torch.zeros((n, n), dtype=torch.int32, device="cuda")
    result["k_distance_ms"] = several(lambda: d.distance_packed_dev(pk.data_ptr(), n, s, mat.data_ptr()))
    del mat
    counts_t = torch.zeros((s, 4), dtype=torch.int32, device="cuda")
    result["site_counts_ms"] = several(lambda: d.site_counts_dev(pk.data_ptr(), n, s, counts_t.data_ptr()))
    result["site_counts_bound_ms"] = SWEEPS["site_counts"] * bound_ms
    numbers, n_clusters, mat = clusters_of(pk, n)
    del mat
    per = []
    for t, thr in enumerate(THRESHOLDS):
        total = snps(pk, n, numbers[t], n_clusters[t])
        out = room(n_clusters[t], total)
        ms_count = several(lambda: snps(pk, n, numbers[t], n_clusters[t]))
        ms_emit = several(lambda: snps(pk, n, numbers[t], n_clusters[t], max(total, 1), out))
        sizes = np.bincount(numbers[t].cpu().numpy())[1:]
        per.append({"threshold": thr, "clusters": n_clusters[t], "singletons": int((sizes == 1).sum()), "largest": int(sizes.max()), "rows": int(total),
                    "count_ms": ms_count, "count_and_emit_ms": ms_emit, "bound_ms": SWEEPS["cluster_snps"] * bound_ms,
                    "presence_bytes": n_clusters[t] * ((s + 2047) // 2048) * 1024})
        print("T = %d: %d clusters, %d rows, %.2f ms" % (thr, n_clusters[t], total, ms_emit["median"]), file=sys.stderr, flush=True)
        del out
    result["cluster_snps"] = per
    result["cluster_snps_all_thresholds_ms"] = sum(p["count_and_emit_ms"]["median"] for p in per)
    result["cluster_snps_all_thresholds_bound_ms"] = len(per) * SWEEPS["cluster_snps"] * bound_ms
    result["cluster_snps_all_thresholds_rows"] = sum(p["rows"] for p in per)
    del pk, counts_t, numbers
    d.close()

    # ---- the command ------------------------------------------------------------------------------------------------------------
    if not a.skip_command:
        tmp = tempfile.mkdtemp(prefix="snpclustersnps_")
        try:
            fasta = os.path.join(tmp, "snpma.fasta")
            with open(fasta, "wb") as f:
                for r in range(n):
                    f.write(b">s%06d\n" % r)
                    f.write(sym[r].tobytes())
                    f.write(b"\n")
            exe = os.path.join(ROOT, "bin", "cfsan_snp_pipeline")
            out = os.path.join(tmp, "out.tsv")
            thresholds = [str(t) for t in THRESHOLDS]
            cases = [("site_counts_only", ["--amdSiteCounts", out]), ("cluster_snps_only", ["--amdClusterSnps", out, "--amdClusterThresholds"] + thresholds),
                     ("clusters_only", ["--amdClusters", out, "--amdClusterThresholds"] + thresholds)]
            if not a.skip_tables:
                cases.append(("tables_p_m", ["-p", out, "-m", os.path.join(tmp, "matrix.tsv")]))
            for key, extra in cases:
                cmd = [sys.executable, exe, "distance", "-v", "0", "-f", fasta] + extra
                wall = []
                for rep in range(a.runs + 1):
                    t0 = time.perf_counter()
                    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, SNPGPU_DEVICE="0"))
                    wall.append(time.perf_counter() - t0)
                    assert r.returncode == 0, r.stderr[-2000:]
                    print("%s run %d: %.2f s" % (key, rep, wall[-1]), file=sys.stderr, flush=True)
                result["distance_wall_s_" + key] = _spread(wall[1:])
                result["bytes_written_" + key] = os.path.getsize(out)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    text = json.dumps(result, indent=1, sort_keys=True)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
