#!/usr/bin/env python3
"""What the compared-site counts of the distance step cost on one GPU (profiles/r22/compared.md):

  0. outside every timed region, at --check-samples samples: the plane, the compared matrix and the listed pairs must be what
     NumPy counts site by site, and Distance <= Compared;
  1. events around each call, in one run: k_distance (snpgpu_distance_packed_dev), the plane extraction
     (snpgpu_valid_plane_dev), the compared matrix (snpgpu_compared_rect_dev, the same plane twice), and
     snpgpu_compared_pairs_dev for the n - 1 edges of the spanning tree and for the pairs within --within SNPs — each beside its
     derived floor: half of k_distance's vector work over 3.93e13 lane-ops/s, the packed bytes over the 6.3 TB/s copy ceiling,
     two plane rows per pair over the same ceiling;
  2. wall time of `distance` (a fresh process per run, the input in the page cache) with only --amdComparedMatrix and with
     --amdClosePairs --amdCompared: medians of --runs runs after a warm-up, with the spread.

    python tools/compared_time.py [--samples 10000] [--sites 200000] [--group 25] [--runs 3] [--out result.json]

The planted groups are those of tools/clusters_time.py; every sample then loses up to --missing of its columns to '-' and 'N'."""
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
VALU_LANE_OPS_PER_S = 3.93e13           # integer lane-ops; a word-pair costs k_distance 4, the compared matrix 2
TILE = 128


def _spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": xs}


def with_missing(sym, share, seed=3):
    """Every row loses a random share in [0, share) of its columns, half of them to '-' and half to 'N'."""
    rng = np.random.default_rng(seed)
    s = sym.shape[1]
    for r in range(len(sym)):
        at = rng.integers(0, s, size=int(rng.random() * share * s))
        sym[r, at[::2]] = 0x2D
        sym[r, at[1::2]] = 0x4E
    return sym


def valid_of(sym):
    up = np.where((sym >= 97) & (sym <= 122), sym - 32, sym).astype(np.uint8)
    return np.isin(up, np.frombuffer(b"ACGT", dtype=np.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--sites", type=int, default=200000)
    ap.add_argument("--group", type=int, default=25)
    ap.add_argument("--missing", type=float, default=0.1)
    ap.add_argument("--within", type=int, default=50)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--check-samples", type=int, default=200)
    ap.add_argument("--skip-command", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    import torch
    from clusters_time import planted
    from snp_pipeline_amd import device as dev
    n, s = a.samples, a.sites
    sym = with_missing(planted(n, s, a.group), a.missing)
    print("planted %d x %d, up to %.0f %% of a row missing" % (n, s, 100 * a.missing), file=sys.stderr, flush=True)
    result = {"samples": n, "sites": s, "group": a.group, "missing": a.missing, "within": a.within, "runs": a.runs}
    d = dev.Device(0)
    d.use_torch_stream()
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    packed_row, plane_row = d.packed_row_bytes(s), d.valid_plane_row_bytes(s)
    result.update(cu=cu, packed_words=packed_row // 16, plane_words=plane_row // 4)

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

    def plane_of(packed, k):
        plane = torch.full((k, plane_row), 0xA5, dtype=torch.uint8, device="cuda")
        d.valid_plane_dev(packed.data_ptr(), k, s, plane.data_ptr())
        torch.cuda.synchronize()
        return plane

    def listed(plane, k, pa, pb):
        a_t, b_t = torch.from_numpy(pa.astype(np.int32)).cuda(), torch.from_numpy(pb.astype(np.int32)).cuda()
        out = torch.full((len(pa),), -1, dtype=torch.int32, device="cuda")
        ms = several(lambda: d.compared_pairs_dev(plane.data_ptr(), k, plane.data_ptr(), k, s, a_t.data_ptr(), b_t.data_ptr(), len(pa), out.data_ptr()))
        return ms, out.cpu().numpy()

    # ---- the check, outside every timed region ------------------------------------------------------------------------------
    k = min(a.check_samples, n)
    rows = sym[:: max(n // k, 1)][:k]
    valid = valid_of(rows)
    want = (valid.astype(np.float32) @ valid.astype(np.float32).T).astype(np.int32)      # counts up to 2e5: exact in float32
    pk = pack(rows)
    pl = plane_of(pk, k)
    got = torch.full((k, k), -1, dtype=torch.int32, device="cuda")
    d.compared_rect_dev(pl.data_ptr(), k, pl.data_ptr(), k, s, got.data_ptr())
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert np.array_equal(got, want) and np.array_equal(np.diag(got), valid.sum(axis=1)) and (d.distance(rows) <= got).all()
    pa, pb = np.arange(k)[::-1].copy(), (np.arange(k) * 7) % k
    assert np.array_equal(listed(pl, k, pa, pb)[1], want[pa, pb])
    result.update(check_samples=k, compared_min=int(np.diag(got).min()), compared_max=int(np.diag(got).max()))
    print("plane, matrix and pairs == NumPy at %d samples; own counts %d ... %d of %d" % (k, np.diag(got).min(), np.diag(got).max(), s), file=sys.stderr, flush=True)
    del pk, pl

    # ---- the calls alone ------------------------------------------------------------------------------------------------------
    pk = pack(sym)
    mat = torch.zeros((n, n), dtype=torch.int32, device="cuda")
    result["k_distance_ms"] = several(lambda: d.distance_packed_dev(pk.data_ptr(), n, s, mat.data_ptr()))
    plane = torch.full((n, plane_row), 0xA5, dtype=torch.uint8, device="cuda")
    result["valid_plane_ms"] = several(lambda: d.valid_plane_dev(pk.data_ptr(), n, s, plane.data_ptr()))
    cmp_mat = torch.zeros((n, n), dtype=torch.int32, device="cuda")
    result["compared_matrix_ms"] = several(lambda: d.compared_rect_dev(plane.data_ptr(), n, plane.data_ptr(), n, s, cmp_mat.data_ptr()))
    tiles = (n + TILE - 1) // TILE
    pairs_of_tiles = tiles * (tiles + 1) // 2 * TILE * TILE
    result["k_distance_floor_ms"] = pairs_of_tiles * (packed_row // 16) * 4 / VALU_LANE_OPS_PER_S * 1e3
    result["compared_matrix_floor_ms"] = pairs_of_tiles * (plane_row // 4) * 2 / VALU_LANE_OPS_PER_S * 1e3
    result["valid_plane_floor_ms"] = (n * packed_row + n * plane_row) / HBM_BYTES_PER_S * 1e3
    host_mat, host_cmp = mat.cpu().numpy(), cmp_mat.cpu().numpy()
    assert (host_mat <= host_cmp).all() and np.array_equal(host_cmp, host_cmp.T)
    # the tree's edges and the pairs within the threshold, from the matrix of this run
    u = torch.zeros(max(n - 1, 1), dtype=torch.int32, device="cuda")
    v, w = torch.zeros_like(u), torch.zeros_like(u)
    n_edges, _ = d.mst_dev(mat.data_ptr(), n, n, 0, n, u.data_ptr(), v.data_ptr(), w.data_ptr())
    torch.cuda.synchronize()
    eu, ev = u[:n_edges].cpu().numpy(), v[:n_edges].cpu().numpy()
    ci, cj = np.nonzero(np.triu(host_mat <= a.within, 1))
    for name, (pa, pb) in (("tree_edges", (eu, ev)), ("pairs_within", (ci, cj))):
        ms, counts = listed(plane, n, pa, pb)
        assert np.array_equal(counts, host_cmp[pa, pb])
        result["compared_pairs_%s" % name] = {"pairs": int(len(pa)), "ms": ms, "floor_ms": len(pa) * 2 * plane_row / HBM_BYTES_PER_S * 1e3}
    print("timed: k_distance %.2f ms, plane %.3f ms, compared matrix %.2f ms, pairs %.3f / %.3f ms" % (
        result["k_distance_ms"]["median"], result["valid_plane_ms"]["median"], result["compared_matrix_ms"]["median"],
        result["compared_pairs_tree_edges"]["ms"]["median"], result["compared_pairs_pairs_within"]["ms"]["median"]), file=sys.stderr, flush=True)
    del pk, mat, plane, cmp_mat, host_mat, host_cmp
    d.close()

    # ---- the command ------------------------------------------------------------------------------------------------------------
    if not a.skip_command:
        tmp = tempfile.mkdtemp(prefix="snpcompared_")
        try:
            fasta = os.path.join(tmp, "snpma.fasta")
            with open(fasta, "wb") as f:
                for r in range(n):
                    f.write(b">s%06d\n" % r)
                    f.write(sym[r].tobytes())
                    f.write(b"\n")
            exe = os.path.join(ROOT, "bin", "cfsan_snp_pipeline")
            out = os.path.join(tmp, "out.tsv")
            for key, extra in (("compared_matrix_only", ["--amdComparedMatrix", out]),
                               ("close_pairs_with_compared", ["--amdClosePairs", out, "--amdMaxPairDistance", str(a.within), "--amdCompared"]),
                               ("close_pairs_without", ["--amdClosePairs", out, "--amdMaxPairDistance", str(a.within)])):
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
