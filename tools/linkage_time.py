#!/usr/bin/env python3
"""What the complete- and average-linkage trees of the distance step cost on one GPU (profiles/r20/linkage.md):

  0. outside every timed region, at --check-samples samples: the keys of the device tree ascend, the host forms on the symbols and
     on the matrix give the same merges, and every complete-linkage cluster at a threshold has its diameter within it;
  1. the call snpgpu_linkage_dev alone on a planted-groups matrix, both kinds (events around the call, its waits for the stream
     and the final ordering on the host included; a first call warms the caches and is not counted) and its round count, beside
     k_distance in the same run — and the bound the design implies: a round reads at most the n columns of n rows of the working
     matrix, 8 n^2 bytes, against the 6.3 TB/s the copy kernel reaches on this part;
  2. the worst case for the round count: --identical identical samples, n - 1 rounds of one merge each, a launch and wait figure;
  3. wall time of `distance` (a fresh process per run, the input in the page cache) with only the three new outputs, against the
     same command with `-p -m`: medians of --runs runs after a warm-up, with the spread.

    python tools/linkage_time.py [--samples 10000] [--sites 200000] [--group 25] [--runs 3] [--out result.json]

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
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KINDS = ("complete", "average")
COPY_CEILING_TB_S = 6.3


def _spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": xs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--sites", type=int, default=200000)
    ap.add_argument("--group", type=int, default=25)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--check-samples", type=int, default=1200)
    ap.add_argument("--identical", type=int, default=2000)
    ap.add_argument("--skip-command", action="store_true", help="time the calls only")
    ap.add_argument("--skip-tables", action="store_true", help="do not time the -p -m run (3 GB of text at 10 000 samples)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    import torch
    from clusters_time import planted
    from snp_pipeline_amd import device as dev
    n, s = a.samples, a.sites
    sym = planted(n, s, a.group)
    print("planted %d x %d" % (n, s), file=sys.stderr, flush=True)
    result = {"samples": n, "sites": s, "group": a.group, "groups": (n + a.group - 1) // a.group, "runs": a.runs}
    d = dev.Device(0)
    d.use_torch_stream()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    def room(k):
        m = max(k - 1, 1)
        return [torch.zeros(m, dtype=torch.int32, device="cuda") for _ in range(4)] + [torch.zeros(m, dtype=torch.int64, device="cuda")]

    def tree_of(mat, k, kind, out):
        return d.linkage_dev(mat.data_ptr(), k, k, kind, *(o.data_ptr() for o in out))

    # ---- the check, outside every timed region ------------------------------------------------------------------------------
    k = min(a.check_samples, n)
    rows = np.ascontiguousarray(sym[:: max(n // k, 1)][:k])
    checked = {}
    for kind in KINDS:
        got = d.linkage(rows, kind, want_matrix=True)
        merges, mat = list(zip(*(x.tolist() for x in got[:5]))), got[5]
        again = d.linkage_of_matrix(mat, kind)
        assert all(np.array_equal(x, y) for x, y in zip(got[:5], again))
        keys = [(Fraction(num, sa * sb) if kind == "average" else num, x, y) for x, y, sa, sb, num in merges]
        assert keys == sorted(keys) and len(merges) == k - 1
        if kind == "complete":
            t = 30
            parent = list(range(k))
            for x, y, _, _, num in merges:
                if num > t:
                    break
                parent[y] = x
            label = np.asarray([i for i in range(k)])
            for i in range(k):
                label[i] = label[parent[i]] if parent[i] != i else i
            same = label[:, None] == label[None, :]
            assert int(mat[same].max()) <= t                          # every two members of a cluster within t
            checked["complete_clusters_at_%d" % t] = len(set(label.tolist()))
    result.update(check_samples=k, **checked)
    print("checks passed at %d samples" % k, file=sys.stderr, flush=True)

    # ---- the call alone -------------------------------------------------------------------------------------------------------
    sym_t = torch.from_numpy(np.ascontiguousarray(sym)).cuda()
    packed = torch.zeros((n, d.packed_row_bytes(s)), dtype=torch.uint8, device="cuda")
    d.pack_matrix_dev(sym_t.data_ptr(), n, s, s, packed.data_ptr())
    del sym_t
    mat = torch.zeros((n, n), dtype=torch.int32, device="cuda")
    out = room(n)
    ms_dist = []
    ms_tree = {kind: [] for kind in KINDS}
    rounds = {}
    for rep in range(a.runs + 1):
        ms_dist.append(timed(lambda: d.distance_packed_dev(packed.data_ptr(), n, s, mat.data_ptr()))[0])
        for kind in KINDS:
            ms, (n_merges, rounds[kind]) = timed(lambda: tree_of(mat, n, kind, out))
            assert n_merges == n - 1
            ms_tree[kind].append(ms)
    result.update(distance_kernel_ms=_spread(ms_dist[1:]), working_matrix_GB=n * n * 8 / 1e9)
    for kind in KINDS:
        bound_ms = rounds[kind] * n * n * 8 / (COPY_CEILING_TB_S * 1e12) * 1e3
        result["linkage_call_ms_" + kind] = _spread(ms_tree[kind][1:])
        result["linkage_rounds_" + kind] = rounds[kind]
        result["bound_ms_every_row_every_round_" + kind] = bound_ms
    del mat, packed, out
    print("call timed", file=sys.stderr, flush=True)

    # ---- identical samples: n - 1 rounds --------------------------------------------------------------------------------------
    z = a.identical
    if z > 1:
        zero = torch.zeros((z, z), dtype=torch.int32, device="cuda")
        out = room(z)
        for kind in KINDS:
            ms = []
            for rep in range(a.runs + 1):
                t, (n_merges, r) = timed(lambda: tree_of(zero, z, kind, out))
                assert n_merges == z - 1 and r == z - 1
                ms.append(t)
            result["identical_%d_call_ms_%s" % (z, kind)] = _spread(ms[1:])
            result["identical_%d_ms_per_round_%s" % (z, kind)] = statistics.median(ms[1:]) / (z - 1)
        del zero, out
    d.close()

    # ---- the command ------------------------------------------------------------------------------------------------------------
    if not a.skip_command:
        tmp = tempfile.mkdtemp(prefix="snplinkage_")
        try:
            fasta = os.path.join(tmp, "snpma.fasta")
            with open(fasta, "wb") as f:
                for r in range(n):
                    f.write(b">s%06d\n" % r)
                    f.write(sym[r].tobytes())
                    f.write(b"\n")
            exe = os.path.join(ROOT, "bin", "cfsan_snp_pipeline")
            new = {kind: ["--amdLinkage", kind, "--amdLinkageMerges", os.path.join(tmp, "merges.tsv"), "--amdLinkageDendrogram", os.path.join(tmp, "tree.nwk"),
                          "--amdLinkageClusters", os.path.join(tmp, "clusters.tsv"), "--amdClusterThresholds", "5", "20", "100"] for kind in KINDS}
            tables = ["-p", os.path.join(tmp, "pairwise.tsv"), "-m", os.path.join(tmp, "matrix.tsv")]
            runs = [("new_outputs_only_" + kind, new[kind]) for kind in KINDS] + ([] if a.skip_tables else [("tables_p_m", tables)])
            for label, opts in runs:
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
