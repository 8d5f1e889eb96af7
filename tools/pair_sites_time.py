#!/usr/bin/env python3
"""What the differing sites of the distance step cost on one GPU (profiles/r19/pair_sites.md):

  0. outside every timed region: every pair of both lists has as many entries as the matrix says, and a sample of the pairs has
     the entries of a NumPy walk over the two rows;
  1. the call snpgpu_pair_sites_dev (events around the call, its wait for the stream included) on a planted-groups matrix, for the
     n - 1 edges of the minimum spanning tree and for the pairs i < j within --threshold: the count alone (capacity 0) and the
     whole call with room for the sum of the distances — beside k_distance in the same run, and as a fraction of what reading
     2 passes x m pairs x 2 rows takes at the measured copy ceiling.

    python tools/pair_sites_time.py [--samples 10000] [--sites 200000] [--group 25] [--threshold 50] [--runs 3] [--out result.json]

The planted groups are those of tools/clusters_time.py."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
COPY_CEILING_TB_S = 6.3


def _spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": xs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--sites", type=int, default=200000)
    ap.add_argument("--group", type=int, default=25)
    ap.add_argument("--threshold", type=int, default=50)
    ap.add_argument("--runs", type=int, default=3)
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
    d = dev.Device(0)
    d.use_torch_stream()
    row_bytes = d.packed_row_bytes(s)
    result = {"samples": n, "sites": s, "group": a.group, "threshold": a.threshold, "runs": a.runs, "packed_row_bytes": row_bytes,
              "copy_ceiling_TB_s": COPY_CEILING_TB_S}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    sym_t = torch.from_numpy(sym).cuda()
    packed = torch.zeros((n, row_bytes), dtype=torch.uint8, device="cuda")
    d.pack_matrix_dev(sym_t.data_ptr(), n, s, s, packed.data_ptr())
    torch.cuda.synchronize()
    del sym_t
    mat = torch.zeros((n, n), dtype=torch.int32, device="cuda")
    ms_dist = [timed(lambda: d.distance_packed_dev(packed.data_ptr(), n, s, mat.data_ptr()))[0] for _ in range(a.runs + 1)]
    result["distance_kernel_ms"] = _spread(ms_dist[1:])

    # the two pair lists, from the matrix where it lies
    out = [torch.zeros(max(n - 1, 1), dtype=torch.int32, device="cuda") for _ in range(3)]
    n_edges, _ = d.mst_dev(mat.data_ptr(), n, n, 0, n, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr())
    tree = tuple(o[:n_edges].cpu().numpy() for o in out)
    total = d.close_pairs_dev(mat.data_ptr(), n, n, 0, n, a.threshold)
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    col = torch.zeros(max(total, 1), dtype=torch.int32, device="cuda")
    dist = torch.zeros(max(total, 1), dtype=torch.int32, device="cuda")
    d.close_pairs_dev(mat.data_ptr(), n, n, 0, n, a.threshold, max(total, 1), off.data_ptr(), col.data_ptr(), dist.data_ptr())
    close = dmod.pairs_of_csr(off.cpu().numpy(), col[:total].cpu().numpy().view(np.uint32), dist[:total].cpu().numpy(), a.threshold)
    del out, off, col, dist, mat
    lists = {"tree": (tree[0].view(np.uint32), tree[1].view(np.uint32), tree[2]), "close": close}

    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    for name, (pa, pb, pd) in lists.items():
        m = len(pa)
        want = int(np.asarray(pd).sum(dtype=np.int64))
        d_a = torch.from_numpy(np.ascontiguousarray(pa).view(np.int32)).cuda()
        d_b = torch.from_numpy(np.ascontiguousarray(pb).view(np.int32)).cuda()
        pair_off = torch.zeros(m + 1, dtype=torch.int64, device="cuda")
        site = torch.zeros(max(want, 1), dtype=torch.int32, device="cuda")
        bases = torch.zeros(max(want, 1), dtype=torch.uint8, device="cuda")
        args = (packed.data_ptr(), n, s, d_a.data_ptr(), d_b.data_ptr(), m)
        ms_count, ms_call = [], []
        for rep in range(a.runs + 1):
            ms, got = timed(lambda: d.pair_sites_dev(*args))
            ms_count.append(ms)
            assert got == want
            ms, got = timed(lambda: d.pair_sites_dev(*args, max(want, 1), pair_off.data_ptr(), site.data_ptr(), bases.data_ptr()))
            ms_call.append(ms)
            assert got == want
        # ---- the check, outside every timed region
        h_off, h_site, h_bases = pair_off.cpu().numpy(), site[:want].cpu().numpy().view(np.uint32), bases[:want].cpu().numpy()
        assert np.array_equal(np.diff(h_off), np.asarray(pd, dtype=np.int64))
        for p in np.random.default_rng(7).choice(m, size=min(m, 200), replace=False):
            x, y = sym[pa[p]], sym[pb[p]]
            at = np.flatnonzero(x != y)                                   # (the planted matrix holds ACGT only)
            lo, hi = int(h_off[p]), int(h_off[p + 1])
            assert np.array_equal(h_site[lo:hi], at.astype(np.uint32))
            assert np.array_equal(acgt[h_bases[lo:hi] & 3], x[at]) and np.array_equal(acgt[(h_bases[lo:hi] >> 4) & 3], y[at]) and not (h_bases[lo:hi] & 0x44).any()
        read_bytes = 2 * m * 2 * row_bytes
        bound_ms = read_bytes / (COPY_CEILING_TB_S * 1e12) * 1e3
        result[name] = {"pairs": m, "entries": want, "count_ms": _spread(ms_count[1:]), "call_ms": _spread(ms_call[1:]),
                        "two_pass_read_GB": read_bytes / 1e9, "written_MB": 5 * want / 1e6, "bound_ms_at_copy_ceiling": bound_ms,
                        "fraction_of_bound": bound_ms / statistics.median(ms_call[1:]),
                        "call_over_distance_kernel": statistics.median(ms_call[1:]) / statistics.median(ms_dist[1:])}
        print("%s: %d pairs, %d entries timed and checked" % (name, m, want), file=sys.stderr, flush=True)
        del d_a, d_b, pair_off, site, bases
    d.close()
    text = json.dumps(result, indent=1, sort_keys=True)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
