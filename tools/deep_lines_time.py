#!/usr/bin/env python3
"""Deep-coverage pileups through scan + call: resident synthetic batches (csrc/synth.hip) at several mean depths, the scan (K1) and
the call kernels (K2) timed with HIP events around their launches (Device.kernel_timing), and which call kernel took the lines
(Device.call_pass_counts).  Per depth one row: K1 GB/s and its fraction of the 8 TB/s HBM peak, call-kernel ms per launch, ns per
matched byte (the bytes of the lines the call step reads: matched lines x mean line length) and the pass counts.
    python tools/deep_lines_time.py [depths, default 30,100,250] [reps, default 5]
The synthetic samples stop at 250 reads per position, as samtools mpileup does by default: a mean depth of 250 gives lines of
~540 bytes, all past the 512-byte window; deeper means give the same lines.
DEEP_GENOME (default 400000) positions per sample, one position in 20 listed; the samples of a batch shrink with the depth so that
every batch holds about the same bytes (DEEP_BYTES, default 1.5e9).  The same tool runs on a library without
snpgpu_call_pass_counts (SNPGPU_LIB): the counts are then left out."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from snp_pipeline_amd import _lib as L
    if not os.environ.get("SNPGPU_LIB") is None:                      # an older library: bind what it has
        import ctypes
        have = ctypes.CDLL(os.environ["SNPGPU_LIB"])
        for name in [n for n in L.SIGNATURES if not hasattr(have, n)]:
            del L.SIGNATURES[name]
    from snp_pipeline_amd import device as dev
    depths = [float(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "30,100,250").split(",")]
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    G = int(os.environ.get("DEEP_GENOME", "400000"))
    budget = float(os.environ.get("DEEP_BYTES", "1.5e9"))
    S = G // 20
    contig = b"synth_chr1"
    d = dev.Device(0)
    d.use_torch_stream()
    ref = torch.empty(G + 1, dtype=torch.uint8, device="cuda")
    d.synth_reference_dev(1, G, ref.data_ptr())
    pos = np.sort(np.random.default_rng(2).choice(np.arange(501, G - 499), size=S, replace=False))
    alt_h = np.zeros(G + 1, dtype=np.uint8)
    alt_h[pos] = ord("A")
    alt = torch.from_numpy(alt_h).cuda()
    ss = d.siteset([(contig, int(p)) for p in pos], [1] * S)
    prm = dev.make_params(0, 0.6, 3, 0, 0.0)
    has_counts = "snpgpu_call_pass_counts" in L.SIGNATURES
    print("depth  samples  bytes        lines/sample  mean line  K1 GB/s  of peak  call ms (min..max of %d)   ns/matched byte  passes" % reps)
    for depth in depths:
        n0 = d.synth_pileup_dev(3, 0, G, ref.data_ptr(), alt.data_ptr(), 0, 0, mean_depth=depth, contig=contig)
        B = int(max(1, min(64, budget // max(n0, 1))))
        bufs, sizes = [], []
        for i in range(B):
            n = d.synth_pileup_dev(3, i, G, ref.data_ptr(), alt.data_ptr(), 0, 0, mean_depth=depth, contig=contig)
            t = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
            d.synth_pileup_dev(3, i, G, ref.data_ptr(), alt.data_ptr(), t.data_ptr(), n + 64, mean_depth=depth, contig=contig)
            bufs.append(t)
            sizes.append(n)
        bases = torch.empty((B, S), dtype=torch.uint8, device="cuda")
        filt = torch.empty((B, S), dtype=torch.uint8, device="cuda")
        status = torch.empty((B, 4), dtype=torch.int64, device="cuda")
        ptrs = [t.data_ptr() for t in bufs]
        base = min(ptrs)
        offs = np.array([p - base for p in ptrs], dtype=np.uint64)

        def run():
            d.call_consensus_batch_dev(ss, base, offs, prm, bases.data_ptr(), filt.data_ptr(), status.data_ptr(), sizes=sizes)

        run()
        torch.cuda.synchronize()
        st = status.cpu().numpy()
        lines, matched = int(st[:, 1].sum()), int(st[:, 2].sum())
        mean_line = sum(sizes) / max(lines, 1)
        d.kernel_timing(True)
        d.kernel_time_ms(0), d.kernel_time_ms(1)
        scan_ms, call_ms = [], []
        for _ in range(reps):
            run()
            torch.cuda.synchronize()
            sm, sn = d.kernel_time_ms(0)
            cm, cn = d.kernel_time_ms(1)
            scan_ms.append(sm)
            call_ms.append(cm)
        d.kernel_timing(False)
        gbs = sum(sizes) / (min(scan_ms) * 1e-3) / 1e9
        cmin = min(call_ms)
        passes = d.call_pass_counts() if has_counts else None
        chk = int(bases.to(torch.int64).sum().item())
        print("%-6g %-8d %-12d %-13d %-10.1f %-8.0f %-8.3f %.3f (%.3f..%.3f)   %-16.4f %s  [checksum %d]"
              % (depth, B, sum(sizes), lines // B, mean_line, gbs, gbs / 8000.0, cmin, cmin, max(call_ms), cmin * 1e6 / max(matched * mean_line, 1),
                 " ".join("%s=%d" % (k, passes[k]) for k in dev.Device.CALL_PASS_NAMES) if passes else "(this library does not report them)", chk), flush=True)
        del bufs, bases, filt, status


if __name__ == "__main__":
    main()
