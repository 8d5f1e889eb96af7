#!/usr/bin/env python3
"""What the query-against-database nearest neighbours of the distance step cost on one GPU (profiles/r21/nearest.md):

  0. outside every timed region, at --check-samples database samples: both routes of snpgpu_distance_rect_packed_dev must give
     the off-diagonal block of snpgpu_distance over the stacked samples, and snpgpu_nearest_dev the stable NumPy sort of its rows;
  1. the call snpgpu_distance_rect_packed_dev alone on each route for every q of --queries against the planted-groups database
     (events around the call), beside what the same answer cost before: k_distance over the n + q stacked rows, in the same run,
     and beside the two derived bounds — the database bytes of every sweep over 6.3 TB/s, the word-pairs x 4 lane-ops over
     3.9e13 lane-ops/s;
  2. the selection snpgpu_nearest_dev at K = 10 over the q x n matrix (count, scan, emit, sort; its waits included);
  3. wall time of `distance` (a fresh process per run, the inputs in the page cache) with only --amdQuery / --amdNearest:
     medians of --runs runs after a warm-up, with the spread.

    python tools/nearest_time.py [--samples 10000] [--sites 200000] [--group 25] [--runs 3] [--out result.json]

The planted groups are those of tools/clusters_time.py; a query is a database sample with a few sites changed."""
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
VALU_LANE_OPS_PER_S = 3.9e13            # integer lane-ops; a word-pair costs 4
SHAPE = {"narrow": (16, 64), "tile": (128, 128)}       # query rows x database rows of a tile (csrc/nearest.hip)


def _spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": xs}


def queries_of(sym, q, seed=2):
    rng = np.random.default_rng(seed)
    rows = sym[rng.integers(0, len(sym), size=q)].copy()
    for r in range(q):
        at = rng.integers(0, sym.shape[1], size=int(rng.integers(0, 13)))
        rows[r, at] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=len(at))]
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--sites", type=int, default=200000)
    ap.add_argument("--group", type=int, default=25)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 16, 32, 64, 128, 1000])
    ap.add_argument("--count", type=int, default=10)
    ap.add_argument("--check-samples", type=int, default=1500)
    ap.add_argument("--command-queries", type=int, default=16)
    ap.add_argument("--skip-command", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    import torch
    from clusters_time import planted
    from snp_pipeline_amd import device as dev
    n, s = a.samples, a.sites
    sym = planted(n, s, a.group)
    q_max = max(a.queries + [a.command_queries])
    q_sym = queries_of(sym, q_max)
    print("planted %d x %d, %d queries" % (n, s, q_max), file=sys.stderr, flush=True)
    result = {"samples": n, "sites": s, "group": a.group, "runs": a.runs, "count": a.count}
    d = dev.Device(0)
    d.use_torch_stream()
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    words = d.packed_row_bytes(s) // 16
    result.update(cu=cu, words=words)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    def pack(rows):
        k = len(rows)
        sym_t = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
        packed = torch.zeros((k, d.packed_row_bytes(s)), dtype=torch.uint8, device="cuda")
        d.pack_matrix_dev(sym_t.data_ptr(), k, s, s, packed.data_ptr())
        torch.cuda.synchronize()
        return packed

    def select(mat, q, k_db, count):
        total = d.nearest_dev(mat.data_ptr(), q, k_db, k_db, count, None)
        off = torch.zeros(q + 1, dtype=torch.int64, device="cuda")
        col = torch.zeros(max(total, 1), dtype=torch.int32, device="cuda")
        dist = torch.zeros(max(total, 1), dtype=torch.int32, device="cuda")
        ms, _ = timed(lambda: d.nearest_dev(mat.data_ptr(), q, k_db, k_db, count, None, max(total, 1), off.data_ptr(), col.data_ptr(), dist.data_ptr()))
        return ms, off.cpu().numpy(), col[:total].cpu().numpy().view(np.uint32), dist[:total].cpu().numpy()

    # ---- the check, outside every timed region ------------------------------------------------------------------------------
    k = min(a.check_samples, n)
    qc = min(40, q_max)
    db_rows = sym[:: max(n // k, 1)][:k]
    square = d.distance(np.concatenate((q_sym[:qc], db_rows)))[:qc, qc:]
    pk_q, pk_db = pack(q_sym[:qc]), pack(db_rows)
    for route in ("narrow", "tile"):
        mat = torch.full((qc, k), -1, dtype=torch.int32, device="cuda")
        d.distance_rect_dev(pk_q.data_ptr(), qc, pk_db.data_ptr(), k, s, mat.data_ptr(), route=route)
        torch.cuda.synchronize()
        assert np.array_equal(mat.cpu().numpy(), square), route
    _, off, col, dist = select(mat, qc, k, a.count)
    order = np.argsort(square, axis=1, kind="stable")[:, :a.count]
    assert list(off) == [a.count * i for i in range(qc + 1)] and np.array_equal(col.reshape(qc, -1), order)
    assert np.array_equal(dist.reshape(qc, -1), np.take_along_axis(square, order, axis=1))
    result.update(check_samples=k, check_queries=qc)
    print("both routes == the block of snpgpu_distance, the selection == the stable sort, at %d x %d" % (qc, k), file=sys.stderr, flush=True)
    del pk_q, pk_db, mat

    # ---- the calls alone ------------------------------------------------------------------------------------------------------
    pk_db, pk_q = pack(sym), pack(q_sym)
    db_bytes = n * words * 16
    rows = []
    for q in a.queries:
        entry = {"q": q}
        mat = torch.zeros((q, n), dtype=torch.int32, device="cuda")
        for route, (tq, tn) in SHAPE.items():
            ms = [timed(lambda: d.distance_rect_dev(pk_q.data_ptr(), q, pk_db.data_ptr(), n, s, mat.data_ptr(), route=route))[0] for _ in range(a.runs + 1)]
            sweeps = (q + tq - 1) // tq
            entry[route + "_ms"] = _spread(ms[1:])
            entry[route + "_bound_hbm_ms"] = sweeps * db_bytes / HBM_BYTES_PER_S * 1e3
            entry[route + "_bound_valu_ms"] = sweeps * tq * ((n + tn - 1) // tn * tn) * words * 4 / VALU_LANE_OPS_PER_S * 1e3
        entry["select_ms"] = _spread([select(mat, q, n, a.count)[0] for _ in range(a.runs + 1)][1:])
        del mat
        # what the same answer cost before: the symmetric matrix over the stacked rows
        both = torch.cat((pk_db, pk_q[:q]))
        full = torch.zeros((n + q, n + q), dtype=torch.int32, device="cuda")
        ms = [timed(lambda: d.distance_packed_dev(both.data_ptr(), n + q, s, full.data_ptr()))[0] for _ in range(a.runs + 1)]
        entry["stacked_k_distance_ms"] = _spread(ms[1:])
        del both, full
        rows.append(entry)
        print("q = %d timed: narrow %.3f ms, tile %.3f ms, select %.3f ms, stacked %.3f ms" % (
            q, entry["narrow_ms"]["median"], entry["tile_ms"]["median"], entry["select_ms"]["median"], entry["stacked_k_distance_ms"]["median"]), file=sys.stderr, flush=True)
    result["calls"] = rows
    del pk_db, pk_q
    d.close()

    # ---- the command ------------------------------------------------------------------------------------------------------------
    if not a.skip_command:
        tmp = tempfile.mkdtemp(prefix="snpnearest_")
        try:
            fasta, query = os.path.join(tmp, "snpma.fasta"), os.path.join(tmp, "query.fasta")
            for path, block, prefix in ((fasta, sym, b"s"), (query, q_sym[:a.command_queries], b"q")):
                with open(path, "wb") as f:
                    for r in range(len(block)):
                        f.write(b">%s%06d\n" % (prefix, r))
                        f.write(block[r].tobytes())
                        f.write(b"\n")
            exe = os.path.join(ROOT, "bin", "cfsan_snp_pipeline")
            out = os.path.join(tmp, "nearest.tsv")
            cmd = [sys.executable, exe, "distance", "-v", "0", "-f", fasta, "--amdQuery", query, "--amdNearest", out, "--amdNearestCount", str(a.count)]
            wall = []
            for rep in range(a.runs + 1):
                t0 = time.perf_counter()
                r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, SNPGPU_DEVICE="0"))
                wall.append(time.perf_counter() - t0)
                assert r.returncode == 0, r.stderr[-2000:]
                print("command run %d: %.2f s" % (rep, wall[-1]), file=sys.stderr, flush=True)
            result["distance_wall_s_nearest_only"] = _spread(wall[1:])
            result["command_queries"] = a.command_queries
            result["bytes_written_nearest_only"] = os.path.getsize(out)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    text = json.dumps(result, indent=1, sort_keys=True)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
