#!/usr/bin/env python3
"""What the bootstrap of the neighbour-joining tree costs on one GPU (profiles/r30/nj_bootstrap.md).  The parent process never
touches the GPU: it plants the symbols, keeps them in a temporary file, and runs every step below as a child process of its own
under a time limit of its own; the first step that fails ends the run.

  check    outside every timed region, at --check-samples samples and 4 replicates: Device.nj_bootstrap gives the tree and the
           counts of the statement (tests/nj_bootstrap_cases.py);
  phases   per replicate, events around each device step as the host form enqueues them (one warm-up replicate is not counted):
           columns + sort, resample, k_distance, the NJ rounds; then the bipartitions and the support counts over the trees of
           those replicates.  The resample kernel is given as a ratio to its bound, one read and one write of the pack at the
           6.3 TB/s the copy kernel reaches on this part;
  call     the whole of Device.nj_bootstrap on the host symbols, upload and pack included (wall clock, one warm-up call);
  old      the only way there was before, per replicate: the statement's columns and sym[:, cols] on the host, Device.nj on the
           gathered symbols, the bipartitions in Python; --old-replicates of them are timed and the figure is scaled to B.

    python tools/nj_bootstrap_time.py [--samples 1000] [--sites 200000] [--groups 400] [--replicates 100] [--runs 2] [--out result.json]
"""
import argparse
import collections
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
COPY_CEILING_TB_S = 6.3
STEP_LIMIT_S = {"check": 120, "phases": 240, "call": 300, "old": 420}


def planted(n, s, groups, seed=1):
    """`groups` groups of samples a few sites from their centre, the centres s / 100 sites from a common base (as tools/clusters_time.py)."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    base = rng.integers(0, 4, size=s, dtype=np.uint8)
    code = np.empty((n, s), dtype=np.uint8)
    of = np.arange(n) * min(groups, n) // max(n, 1)
    for g in range(min(groups, n)):
        centre = base.copy()
        at = rng.choice(s, size=max(1, s // 100), replace=False)
        centre[at] = (centre[at] + rng.integers(1, 4, size=len(at), dtype=np.uint8)) & 3
        rows = np.flatnonzero(of == g)
        code[rows] = centre
        for r in rows:
            at = rng.integers(0, s, size=int(rng.integers(0, 13)))
            code[r, at] = (code[r, at] + 1) & 3
    return acgt[code]


def _spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": xs}


def step_check(a, sym):
    from snp_pipeline_amd import device as dev
    from tests import nj_bootstrap_cases as bc
    from tests import nj_cases as nc
    k = min(a.check_samples, a.samples)
    rows = np.ascontiguousarray(sym[:: max(a.samples // k, 1)][:k, :min(a.sites, 20000)])
    d = dev.Device(0)
    got = d.nj_bootstrap(rows, 4, a.seed)
    want = bc.bootstrap(rows, 4, a.seed)
    assert nc.tree_of_arrays(*got[:6]) == want[0] and got[6].tolist() == want[1]
    d.close()
    return {"check_samples": k, "check_sites": rows.shape[1], "check_support_histogram": dict(collections.Counter(int(x) for x in got[6]))}


def step_phases(a, sym):
    import torch
    from snp_pipeline_amd import device as dev
    n, s, reps = a.samples, a.sites, min(a.replicates, a.phase_replicates)
    k, w = n - 3, (n + 63) // 64
    d = dev.Device(0)
    d.use_torch_stream()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    row_bytes = d.packed_row_bytes(s)
    sym_t = torch.from_numpy(sym).cuda()
    packed = torch.zeros(n * row_bytes + 256, dtype=torch.uint8, device="cuda")
    d.pack_matrix_dev(sym_t.data_ptr(), n, s, s, packed.data_ptr())
    torch.cuda.synchronize()
    del sym_t
    resampled = torch.zeros(n * row_bytes + 256, dtype=torch.uint8, device="cuda")
    cols = torch.zeros(s, dtype=torch.int32, device="cuda")
    mat = torch.zeros((n, n), dtype=torch.int32, device="cuda")
    rec_a, rec_b = (torch.zeros((reps + 1) * k, dtype=torch.int32, device="cuda") for _ in range(2))
    lens = [torch.zeros(k, dtype=torch.int64, device="cuda") for _ in range(2)]
    ms = collections.defaultdict(list)
    for rep in range(reps + 1):                                      # (replicate 0 twice: the first time warms up)
        b = max(rep - 1, 0)
        at = rep * k * 4
        t = {"columns_and_sort": timed(lambda: d.bootstrap_columns_dev(a.seed, b, s, cols.data_ptr(), ascending=True)),
             "resample": timed(lambda: d.resample_packed_dev(packed.data_ptr(), n, s, cols.data_ptr(), s, resampled.data_ptr())),
             "k_distance": timed(lambda: d.distance_packed_dev(resampled.data_ptr(), n, s, mat.data_ptr())),
             "nj_rounds": timed(lambda: d.nj_dev(mat.data_ptr(), n, n, rec_a.data_ptr() + at, rec_b.data_ptr() + at, lens[0].data_ptr(), lens[1].data_ptr()))}
        if rep:
            for name, v in t.items():
                ms[name].append(v)
    # the main tree behind the replicates' records, then bipartitions and counts over all of them
    d.distance_packed_dev(packed.data_ptr(), n, s, mat.data_ptr())
    d.nj_dev(mat.data_ptr(), n, n, rec_a.data_ptr(), rec_b.data_ptr(), lens[0].data_ptr(), lens[1].data_ptr())
    rows = torch.zeros((reps + 1) * k * w, dtype=torch.int64, device="cuda")
    ms_splits, ms_support = [], []
    counts = torch.zeros(k, dtype=torch.int32, device="cuda")
    for run in range(a.runs + 1):
        ms_splits.append(timed(lambda: d.nj_splits_dev(rec_a.data_ptr(), rec_b.data_ptr(), n, reps + 1, rows.data_ptr())))
        ms_support.append(timed(lambda: d.split_support_dev(rows.data_ptr(), k, rows.data_ptr() + k * w * 8, reps * k, w, counts.data_ptr())))
    pack_bytes = n * row_bytes
    bound_ms = 2 * pack_bytes / (COPY_CEILING_TB_S * 1e12) * 1e3
    out = {"phase_replicates": reps, "per_replicate_ms": {name: _spread(v) for name, v in ms.items()},
           "bipartitions_ms_for_%d_trees" % (reps + 1): _spread(ms_splits[1:]), "support_ms_for_%d_trees" % reps: _spread(ms_support[1:]),
           "pack_GB": pack_bytes / 1e9, "resample_bound_ms": bound_ms, "resample_over_bound": statistics.median(ms["resample"]) / bound_ms,
           "launches_of_the_nj_rounds_per_replicate": 3 * k, "support_histogram": dict(collections.Counter(int(x) for x in counts.cpu().numpy()))}
    per = {name: statistics.median(v) for name, v in ms.items()}
    total = sum(per.values())
    out["share_of_a_replicate"] = {name: v / total for name, v in per.items()}
    out["resample_plus_distance_ms"] = per["resample"] + per["k_distance"]
    d.close()
    return out


def step_call(a, sym):
    from snp_pipeline_amd import device as dev
    d = dev.Device(0)
    secs = []
    for run in range(a.runs + 1):
        t0 = time.perf_counter()
        got = d.nj_bootstrap(sym, a.replicates, a.seed)
        secs.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    d.nj(sym)
    plain = time.perf_counter() - t0
    d.close()
    return {"whole_call_s": _spread(secs[1:]), "first_call_s": secs[0], "device_nj_alone_s": plain, "support_histogram": dict(collections.Counter(int(x) for x in got[6]))}


def step_old(a, sym):
    from snp_pipeline_amd import device as dev
    from tests import nj_bootstrap_cases as bc
    n, reps = a.samples, min(a.replicates, a.old_replicates)
    d = dev.Device(0)
    main = d.nj(sym)                                                 # (also the warm-up)
    main_sets = bc.splits(n, list(zip(main[0].tolist(), main[1].tolist())))
    parts = collections.defaultdict(list)
    have = collections.Counter()
    for b in range(reps):
        t0 = time.perf_counter()
        gathered = np.ascontiguousarray(sym[:, bc.columns(a.seed, b, a.sites)])
        t1 = time.perf_counter()
        tree = d.nj(gathered)
        t2 = time.perf_counter()
        have.update(bc.splits(n, list(zip(tree[0].tolist(), tree[1].tolist()))))
        t3 = time.perf_counter()
        for name, v in (("host_gather_s", t1 - t0), ("device_nj_s", t2 - t1), ("python_bipartitions_s", t3 - t2), ("replicate_s", t3 - t0)):
            parts[name].append(v)
    counts = [have[x] for x in main_sets]
    d.close()
    per = statistics.median(parts["replicate_s"])
    return {"old_replicates_timed": reps, "old_per_replicate": {name: _spread(v) for name, v in parts.items()}, "old_way_s_scaled_to_B": per * a.replicates,
            "old_support_histogram": dict(collections.Counter(counts))}


STEPS = {"check": step_check, "phases": step_phases, "call": step_call, "old": step_old}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--sites", type=int, default=200000)
    ap.add_argument("--groups", type=int, default=400)
    ap.add_argument("--replicates", type=int, default=100)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--check-samples", type=int, default=200)
    ap.add_argument("--phase-replicates", type=int, default=5)
    ap.add_argument("--old-replicates", type=int, default=2)
    ap.add_argument("--steps", nargs="*", default=list(STEPS))
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)      # a child: one step on the symbols of --symbols
    ap.add_argument("--symbols", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    if a.step:
        import torch  # noqa: F401  (before the library: one HIP runtime in the process)
        sym = np.load(a.symbols)
        print(json.dumps(STEPS[a.step](a, sym)))
        return 0
    tmp = tempfile.mkdtemp(prefix="snpboot_")
    result = {"samples": a.samples, "sites": a.sites, "groups": a.groups, "replicates": a.replicates, "seed": a.seed, "runs": a.runs}
    try:
        path = os.path.join(tmp, "symbols.npy")
        np.save(path, planted(a.samples, a.sites, a.groups))
        print("planted %d x %d" % (a.samples, a.sites), file=sys.stderr, flush=True)
        for step in a.steps:
            cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--symbols", path] + [x for name in (
                "samples", "sites", "groups", "replicates", "seed", "runs", "check_samples", "phase_replicates", "old_replicates")
                for x in ("--" + name.replace("_", "-"), str(getattr(a, name)))]
            t0 = time.perf_counter()
            try:
                r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=STEP_LIMIT_S[step])
            except subprocess.TimeoutExpired:
                result["stopped_at"] = "%s: no end after %d s" % (step, STEP_LIMIT_S[step])
                break
            if r.returncode != 0:
                result["stopped_at"] = "%s: exit status %d" % (step, r.returncode)
                break
            result.update(json.loads(r.stdout.strip().splitlines()[-1]))
            print("%s: %.1f s" % (step, time.perf_counter() - t0), file=sys.stderr, flush=True)
        if "whole_call_s" in result and "old_way_s_scaled_to_B" in result:
            result["old_way_over_whole_call"] = result["old_way_s_scaled_to_B"] / result["whole_call_s"]["median"]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    text = json.dumps(result, indent=1, sort_keys=True)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 1 if "stopped_at" in result else 0


if __name__ == "__main__":
    sys.exit(main())
