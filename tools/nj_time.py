#!/usr/bin/env python3
"""What the neighbour-joining tree of the distance step costs on one GPU (profiles/r26/nj.md):

  0. outside every timed region, at --check-samples samples: the device tree is the tree of the statement (tests/nj_cases.py,
     nj_numpy), and the host forms on the symbols and on the matrix give the same records;
  1. the call snpgpu_nj_dev alone on a planted-groups matrix (events around the call, its two waits for the stream included; a
     first call warms the caches and is not counted), beside k_distance in the same run;
  2. the two bounds the design implies.  The bytes the rounds must read: k_nj_rows reads, of every live row, the columns behind it
     up to the stored extent — the sum of those extents over the rounds, found by replaying the merges the call returned through
     the compaction schedule of csrc/nj.hip, times 8 bytes, against the 6.3 TB/s the copy kernel reaches on this part.  And the
     launches: the same number of launches of an empty kernel with the same grids and workgroup sizes, timed in the same run;
  3. with --cpu-samples: the NumPy statement on this host's CPU at those sizes (one core), next to the device call at the same sizes.

    python tools/nj_time.py [--samples 10000] [--sites 200000] [--group 25] [--runs 3] [--cpu-samples 1000 2000] [--out result.json]

--compact NUM DEN names the compaction schedule the library in use was built with (-DNJ_COMPACT_NUM / -DNJ_COMPACT_DEN; 0 1 for
never), so that the replay counts what that library reads; --label goes into the result as it is.  The planted groups are those of
tools/clusters_time.py."""
import argparse
import ctypes
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
ROW_GRID_CAP, ROW_THREADS, PICK_THREADS = 2048, 256, 1024          # csrc/nj.hip


def _spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": xs}


def replay(n, a, b, num, den):
    """The schedule of csrc/nj.hip over the merges the call returned: per round the stored extent m and how many entries
    k_nj_rows reads (of every live position p the columns p + 1 ... m - 1; a pair of columns that straddles either end is not counted).  Returns (entries read, [(grid, threads)] of every
    launch in order, compactions)."""
    slots = np.arange(n, dtype=np.int64)
    live = np.ones(n, dtype=bool)
    entries, launches, compactions = 0, [(min(n, ROW_GRID_CAP), ROW_THREADS)], 0
    m = r = n
    for e in range(max(n - 3, 0)):
        if r * den <= m * num:
            slots = slots[live]
            live = np.ones(r, dtype=bool)
            scan_blocks = (m + 8191) // 8192
            launches += [(scan_blocks, 1024), (1, 1024), (scan_blocks, 1024), (min(m, ROW_GRID_CAP), ROW_THREADS)]       # the scan, k_nj_compact
            m = r
            compactions += 1
        at = np.flatnonzero(live)
        entries += int((m - 1 - at).sum())
        launches += [(min(m, ROW_GRID_CAP), ROW_THREADS), (1, PICK_THREADS), ((m + ROW_THREADS - 1) // ROW_THREADS, ROW_THREADS)]     # rows, pick, update
        live[np.searchsorted(slots, b[e])] = False
        r -= 1
    launches.append((1, 64))
    return entries, launches, compactions


class EmptyKernel:
    """An empty kernel compiled for this device and launched through the HIP module interface on a given stream."""
    def __init__(self, tmp):
        src, obj = os.path.join(tmp, "empty.hip"), os.path.join(tmp, "empty.hsaco")
        with open(src, "w") as f:
            f.write('#include <hip/hip_runtime.h>\nextern "C" __global__ void k_empty() {}\n')
        hipcc = os.environ.get("HIPCC") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc")
        subprocess.run([hipcc, "--offload-arch=gfx950", "--genco", "-O3", src, "-o", obj], check=True)
        # the HIP runtime this process already has (torch's and the library's): a second copy would not know their streams
        with open("/proc/self/maps") as f:
            loaded = sorted(set(line.split()[-1] for line in f if "libamdhip64" in line))
        self.runtime = loaded[0] if loaded else "libamdhip64.so"
        self.hip = ctypes.CDLL(self.runtime)
        self.module, self.fn = ctypes.c_void_p(), ctypes.c_void_p()
        assert self.hip.hipModuleLoad(ctypes.byref(self.module), obj.encode()) == 0
        assert self.hip.hipModuleGetFunction(ctypes.byref(self.fn), self.module, b"k_empty") == 0
        self.hip.hipModuleLaunchKernel.argtypes = [ctypes.c_void_p] + [ctypes.c_uint] * 7 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]

    def launch(self, shapes, stream):
        launch, fn, st = self.hip.hipModuleLaunchKernel, self.fn, ctypes.c_void_p(stream)
        for grid, threads in shapes:
            rc = launch(fn, grid, 1, 1, threads, 1, 1, 0, st, None, None)
            if rc != 0:
                raise RuntimeError("hipModuleLaunchKernel failed (%d)" % rc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--sites", type=int, default=200000)
    ap.add_argument("--group", type=int, default=25)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--check-samples", type=int, default=600, help="0: no check")
    ap.add_argument("--cpu-samples", type=int, nargs="*", default=[])
    ap.add_argument("--compact", type=int, nargs=2, default=[7, 8], metavar=("NUM", "DEN"))
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    import torch
    from clusters_time import planted
    from snp_pipeline_amd import device as dev
    from tests import nj_cases as nc
    n, s = a.samples, a.sites
    num, den = a.compact
    sym = planted(n, s, a.group)
    print("planted %d x %d" % (n, s), file=sys.stderr, flush=True)
    result = {"samples": n, "sites": s, "group": a.group, "groups": (n + a.group - 1) // a.group, "runs": a.runs, "label": a.label, "compact_when_r_le_m_times": [num, den],
              "library": os.environ.get("SNPGPU_LIB", "")}
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
        m = max(k - 3, 1)
        return [torch.zeros(m, dtype=torch.int32, device="cuda") for _ in range(2)] + [torch.zeros(m, dtype=torch.int64, device="cuda") for _ in range(2)]

    def tree_of(mat, k, out):
        return d.nj_dev(mat.data_ptr(), k, k, *(o.data_ptr() for o in out))

    # ---- the check, outside every timed region ------------------------------------------------------------------------------
    k = min(a.check_samples, n)
    if k:
        rows = np.ascontiguousarray(sym[:: max(n // k, 1)][:k])
        got = d.nj(rows, want_matrix=True)
        want = nc.nj_numpy(got[6])
        assert nc.tree_of_arrays(*got[:6]) == want
        assert nc.tree_of_arrays(*d.nj_of_matrix(got[6])) == want
        result.update(check_samples=k, check_negative_lengths=nc.negative_lengths(want))
        print("checks passed at %d samples" % k, file=sys.stderr, flush=True)

    # ---- the call alone -------------------------------------------------------------------------------------------------------
    sym_t = torch.from_numpy(np.ascontiguousarray(sym)).cuda()
    packed = torch.zeros((n, d.packed_row_bytes(s)), dtype=torch.uint8, device="cuda")
    d.pack_matrix_dev(sym_t.data_ptr(), n, s, s, packed.data_ptr())
    del sym_t
    mat = torch.zeros((n, n), dtype=torch.int32, device="cuda")
    out = room(n)
    ms_dist, ms_tree = [], []
    for rep in range(a.runs + 1):
        ms_dist.append(timed(lambda: d.distance_packed_dev(packed.data_ptr(), n, s, mat.data_ptr()))[0])
        ms, (n_merges, star, star_len) = timed(lambda: tree_of(mat, n, out))
        assert n_merges == max(n - 3, 0)
        ms_tree.append(ms)
    result.update(distance_kernel_ms=_spread(ms_dist[1:]), nj_call_ms=_spread(ms_tree[1:]), rounds=n_merges,
                  working_matrix_GB=n * ((n + 1) // 2 * 2) * 8 / 1e9)
    print("call timed", file=sys.stderr, flush=True)

    # ---- the bounds -----------------------------------------------------------------------------------------------------------
    merges_a, merges_b = out[0][:n_merges].cpu().numpy().view(np.uint32), out[1][:n_merges].cpu().numpy().view(np.uint32)
    entries, launches, compactions = replay(n, merges_a, merges_b, num, den)
    triangle = sum(r * (r - 1) // 2 for r in range(4, n + 1))
    result.update(row_kernel_entries_read=entries, row_kernel_GB_read=entries * 8 / 1e9, live_upper_triangle_entries=triangle,
                  entries_over_live_triangle=entries / max(triangle, 1), bound_ms_bytes_at_copy_ceiling=entries * 8 / (COPY_CEILING_TB_S * 1e12) * 1e3,
                  launches=len(launches), compactions=compactions)
    tmp = tempfile.mkdtemp(prefix="snpnj_")
    try:
        empty = EmptyKernel(tmp)
        stream = torch.cuda.current_stream().cuda_stream
        ms_empty = [timed(lambda: empty.launch(launches, stream))[0] for rep in range(a.runs + 1)]
        result.update(bound_ms_same_launches_of_an_empty_kernel=_spread(ms_empty[1:]), hip_runtime=empty.runtime)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    del mat, packed, out
    print("bounds timed", file=sys.stderr, flush=True)

    # ---- the statement on the CPU, the call at the same sizes -----------------------------------------------------------------
    for k in a.cpu_samples:
        rows = np.ascontiguousarray(sym[:: max(n // k, 1)][:k])
        small = torch.from_numpy(d.distance(rows)).cuda()
        small_out = room(k)
        ms = [timed(lambda: tree_of(small, k, small_out))[0] for rep in range(a.runs + 1)]
        t0 = time.perf_counter()
        want = nc.nj_numpy(small.cpu().numpy())
        cpu_s = time.perf_counter() - t0
        got = nc.tree_of_arrays(small_out[0][:k - 3].cpu().numpy().view(np.uint32), small_out[1][:k - 3].cpu().numpy().view(np.uint32),
                                small_out[2][:k - 3].cpu().numpy(), small_out[3][:k - 3].cpu().numpy(), *tree_of(small, k, small_out)[1:])
        assert got == want
        result["numpy_statement_s_at_%d" % k] = cpu_s
        result["nj_call_ms_at_%d" % k] = _spread(ms[1:])
        print("cpu comparison at %d: %.1f s" % (k, cpu_s), file=sys.stderr, flush=True)
    d.close()
    text = json.dumps(result, indent=1, sort_keys=True)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
