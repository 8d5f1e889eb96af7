#!/usr/bin/env python3
"""What BGZF-compressed pileups cost and save on one GPU (profiles/r14/bgzf.md):

  1. the compression ratio of the bench's synthetic pileup (5 Mbp x 30x) under tools/make_bgzf.py at level 6;
  2. plain bytes per second of the inflate kernel alone (events around its launches), beside the same run's pinned
     host -> device copy rate;
  3. wall time of `call_consensus_batch` (a fresh process per run, files in the page cache) over the same N samples, first
     plain, then BGZF: medians of --runs runs after a warm-up, with the spread.

    python tools/bgzf_time.py [--samples 8] [--genome 5000000] [--runs 5] [--out result.json]
    python tools/bgzf_time.py --plain-only --tree PATH      # the plain runs alone with the package of another checkout (the parent commit)
"""
import argparse
import json
import multiprocessing
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


def _compress(job):
    src, dst = job
    sys.path.insert(0, HERE)
    import make_bgzf
    make_bgzf.main([src, dst, "--level", "6"])
    return os.path.getsize(dst)


def _spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": xs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package and console script are measured")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, a.tree)
    import torch
    from snp_pipeline_amd import device as dev
    G, N = a.genome, a.samples
    d = dev.Device(0)
    d.use_torch_stream()
    ref = torch.empty(G + 1, dtype=torch.uint8, device="cuda")
    d.synth_reference_dev(1, G, ref.data_ptr())
    pos = np.sort(np.random.default_rng(2).choice(np.arange(501, G - 499), size=G // 100, replace=False))
    alt_h = np.zeros(G + 1, dtype=np.uint8)
    alt_h[pos] = ord("A")
    alt = torch.from_numpy(alt_h).cuda()
    tmp = tempfile.mkdtemp(prefix="snpbgzf_")
    result = {"genome_len": G, "samples": N, "runs": a.runs}
    try:
        dirs, plain_bytes = [], []
        for s in range(N):
            n = d.synth_pileup_dev(3, s, G, ref.data_ptr(), alt.data_ptr(), 0, 0)
            t = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
            d.synth_pileup_dev(3, s, G, ref.data_ptr(), alt.data_ptr(), t.data_ptr(), n + 64)
            sdir = os.path.join(tmp, "sample%02d" % s)
            os.makedirs(sdir)
            with open(os.path.join(sdir, "reads.all.pileup"), "wb") as f:
                f.write(t[:n].cpu().numpy().tobytes())
            dirs.append(sdir)
            plain_bytes.append(int(n))
            del t
        with open(os.path.join(tmp, "snplist.txt"), "w") as f:
            for p in pos:
                f.write("synth_chr1\t%d\t1\tsample00\n" % p)
        with open(os.path.join(tmp, "dirs.txt"), "w") as f:
            f.write("\n".join(dirs) + "\n")
        result["plain_bytes_per_sample"] = plain_bytes[0]
        if not a.plain_only:
            t0 = time.perf_counter()
            with multiprocessing.Pool(min(N, 16)) as pool:
                sizes = pool.map(_compress, [(os.path.join(s, "reads.all.pileup"), os.path.join(s, "reads.all.pileup.gz")) for s in dirs])
            result["compress_seconds_host_zlib"] = time.perf_counter() - t0
            result["bgzf_bytes_per_sample"] = sizes[0]
            result["compression_ratio"] = sum(plain_bytes) / float(sum(sizes))
            # ---- the kernel alone -----------------------------------------------------------------------------------------
            with open(os.path.join(dirs[0], "reads.all.pileup.gz"), "rb") as f:
                data = f.read()
            rc, blocks, info = dev.Device.bgzf_index(data)
            assert rc == 0
            comp = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
            out = torch.empty(int(info.plain_bytes) + 4096, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            d.kernel_timing(True)
            ms = []
            for rep in range(a.runs + 1):
                status, _ = d.bgzf_inflate_dev(comp.data_ptr(), len(data), blocks, out.data_ptr(), int(info.plain_bytes))
                assert not status.any()
                ms.append(d.kernel_time_ms(6)[0])
            d.kernel_timing(False)
            with open(os.path.join(dirs[0], "reads.all.pileup"), "rb") as f:
                assert out[:int(info.plain_bytes)].cpu().numpy().tobytes() == f.read()
            result["inflate_kernel_ms"] = _spread(ms[1:])
            result["inflate_plain_GB_per_s"] = info.plain_bytes / (statistics.median(ms[1:]) * 1e-3) / 1e9
            result["inflate_compressed_GB_per_s"] = len(data) / (statistics.median(ms[1:]) * 1e-3) / 1e9
            result["blocks"] = len(blocks)
            del comp, out
        # ---- the pinned host -> device probe of this run ----------------------------------------------------------------------
        nb = 1 << 30
        h = torch.empty(nb, dtype=torch.uint8).pin_memory()
        g = torch.empty(nb, dtype=torch.uint8, device="cuda")
        rates = []
        for rep in range(a.runs + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.copy_(h, non_blocking=True)
            e1.record()
            e1.synchronize()
            rates.append(nb / (e0.elapsed_time(e1) * 1e-3) / 1e9)
        result["pinned_h2d_GB_per_s"] = _spread(rates[1:])
        del h, g
        d.close()
        # ---- the command ----------------------------------------------------------------------------------------------------
        exe = os.path.join(a.tree, "bin", "cfsan_snp_pipeline")
        for label, name in (("plain", "reads.all.pileup"),) + (() if a.plain_only else (("bgzf", "reads.all.pileup.gz"),)):
            cmd = [sys.executable, exe, "call_consensus_batch", "-v", "0", "-f", "-l", os.path.join(tmp, "snplist.txt"), "-o", "consensus.fasta",
                   "--minConsDpth", "3", "--pileupName", name, os.path.join(tmp, "dirs.txt")]
            wall = []
            for rep in range(a.runs + 1):
                t0 = time.perf_counter()
                r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, SNPGPU_DEVICE="0"))
                wall.append(time.perf_counter() - t0)
                assert r.returncode == 0, r.stderr[-2000:]
                if rep == 0:
                    with open(os.path.join(dirs[-1], "consensus.fasta")) as f:
                        fasta = f.read()
                    if "fasta" in result:
                        assert fasta == result["fasta"], "the BGZF run wrote another consensus than the plain run"
                    result["fasta"] = fasta
            result["batch_wall_s_" + label] = _spread(wall[1:])
            result["batch_samples_per_s_" + label] = N / statistics.median(wall[1:])
        result.pop("fasta", None)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    text = json.dumps(result, indent=1, sort_keys=True)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
