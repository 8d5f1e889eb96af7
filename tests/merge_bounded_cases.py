"""Cases for tests/test_gpu_merge_bounded.py: seeded trees of per-sample VCF files (the rows and headers of test_gpu_merge_vcfs) with
chosen lines in front of and behind a column's rows, the budget that gives a wanted plan, and the raw library call."""
import ctypes as C
import os
import random

import test_gpu_merge_vcfs as base

FORMAT = base.FORMAT
CONTIGS = (b"ctg1", "contigé".encode("utf-8"), b"z|3")


def tree(tmp_path, seed, n_columns, n_positions=13, density=0.7, contigs=CONTIGS, before=None, after=None, header_only=(), pad=None):
    """n_columns files over n_positions positions per contig (POS = 3, 6, ...).  before / after: {column: [lines]} in front of and behind
    the column's own rows; pad: {column: bytes of a header line added so that the data starts where the case wants it}.  Column 0
    meets the contigs rotated and only two of them, as in test_gpu_merge_vcfs._tree.  Returns (paths in column order, texts)."""
    rng = random.Random(seed)
    paths, texts = [], []
    for c in range(n_columns):
        head = base._header(b"smp%03d" % c)
        if pad and c in pad:
            head = head.replace(b"##source=test\n", b"##source=test\n" + pad[c] + b"\n")
        parts = [head] + [line + b"\n" for line in (before or {}).get(c, [])]
        mine = list(contigs) if c % 3 else list(contigs[1:]) + list(contigs[:1])
        if c not in header_only:
            for chrom in (mine if c % 5 else mine[:2]):
                for pos in range(1, n_positions + 1):
                    if rng.random() < density:
                        parts.append(base._row(rng, chrom, pos * 3, 8, c) + b"\n")
        parts += [line + b"\n" for line in (after or {}).get(c, [])]
        d = tmp_path / ("d%03d" % c)
        d.mkdir(parents=True)
        p = d / "consensus.vcf"
        text = b"".join(parts)
        p.write_bytes(text)
        paths.append(str(p))
        texts.append(text)
    return paths, texts


def plain_row(chrom, pos, ref=b"A", alt=b"G", cell=b"1:4:0:4:0:0:2:2:PASS", ns=b"NS=1"):
    return b"\t".join([chrom, b"%d" % pos, b".", ref, alt, b".", cell.rsplit(b":", 1)[1], ns, FORMAT, cell])


def rows_of(text):
    return [l for l in text.split(b"\n") if l and not l.startswith(b"#")]


def budget_for(paths, n_sites, want, out_buffer_log2=0):
    """The smallest device_bytes whose plan holds `want` sites a round, and that plan.  sites_per_round grows by single sites with the
    budget while the merge is bounded, so below n_sites the plan found holds exactly `want`; from n_sites on it is the single pass,
    whose one round holds every site (its footprint is the record bound's, a step above the largest bounded plan)."""
    from snp_pipeline_amd.device import Device, SnpGpuError
    total = sum(os.path.getsize(p) for p in paths)

    def plan(budget):
        try:
            return Device.merge_plan(len(paths), n_sites, total, budget, out_buffer_log2)
        except SnpGpuError:
            return None

    lo, hi = 1, 1 << 44
    while lo < hi:
        mid = (lo + hi) // 2
        got = plan(mid)
        if got is not None and got["sites_per_round"] >= want:
            hi = mid
        else:
            lo = mid + 1
    got = plan(lo)
    assert got is not None and got["sites_per_round"] >= want
    if want < n_sites:
        assert got["sites_per_round"] == want and got["input_passes"] == 1 + -(-n_sites // want), (want, got)
    return lo, got


def raw_merge(dev, paths, out_path, device_bytes=0, own_lines=b""):
    """snpgpu_merge_vcf_files_opts itself: (return code, message, stats as a dict with the passes merged in)."""
    from snp_pipeline_amd import _lib as L
    n = len(paths)
    arr = (C.c_char_p * n)(*[os.fsencode(p) for p in paths])
    stats, passes = L.MergeStats(), L.MergePasses()
    opts = L.MergeOpts(out_buffer_log2=0, device_bytes=int(device_bytes))
    rc = dev.lib.snpgpu_merge_vcf_files_opts(dev.ctx, arr, n, os.fsencode(out_path), own_lines, len(own_lines), C.byref(opts), C.byref(stats), C.byref(passes))
    message = dev.lib.snpgpu_last_error(dev.ctx).decode("utf-8", "replace") if rc else ""
    out = {name: getattr(stats, name) for name, _ in L.MergeStats._fields_}
    out.update({name: getattr(passes, name) for name, _ in L.MergePasses._fields_})
    return rc, message, out
