"""Deep-coverage lines without a device: the new entry point is declared, bound and exported; hot_path_batch documents its key; and
the inputs of tests/test_gpu_deep_lines.py are deterministic and the oracle alone takes every one of them — so a failure on the
device can only be the kernels'."""
import os
import re

import pytest

from oracle import pileup_oracle as po
from tests import deep_lines_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pass_counts_entry_in_header_binding_and_library():
    from snp_pipeline_amd import _lib, build, device
    header = open(os.path.join(ROOT, "include", "snpgpu.h")).read()
    assert re.search(r"int\s+snpgpu_call_pass_counts\s*\(\s*snpgpu_ctx\s*\*ctx,\s*uint64_t\s+out\[SNPGPU_CALL_PASSES\]\)", header)
    assert int(re.search(r"#define\s+SNPGPU_CALL_PASSES\s+(\d+)", header).group(1)) == _lib.CALL_PASSES == len(device.Device.CALL_PASS_NAMES)
    assert "snpgpu_call_pass_counts" in _lib.SIGNATURES
    build.build(verbose=False)
    assert hasattr(_lib.load(), "snpgpu_call_pass_counts")
    assert device.Device.CALL_PASS_NAMES == ("lanes128", "lanes256", "lanes512", "wave")


def test_hot_path_batch_documents_call_passes():
    from snp_pipeline_amd import hot_path
    doc = hot_path.hot_path_batch.__doc__
    assert "last_stats" in doc and "call_passes" in doc
    for name in ("lanes128", "lanes512", "wave", "groups_not_counted"):
        assert name in doc
    import inspect
    assert '"call_passes"' in inspect.getsource(hot_path._job_stats)


BUILDERS = [("window_lf", lambda: cases.window_edges(b"\n")), ("window_crlf", lambda: cases.window_edges(b"\r\n")),
            ("window_lf_reversed", lambda: cases.window_edges(b"\n", reverse=True)), ("bases", cases.bases_field_edges),
            ("markers", cases.marker_edges), ("quality", cases.quality_edges), ("routing", cases.routing_batch),
            ("markers_at_window_ends", cases.window_marker_edges), ("all_lines", cases.all_lines_file)] + \
           [("fuzz%d" % k, lambda k=k: cases.fuzz_slice(100 + k)) for k in range(5)]           # (the seeds the GPU test uses)


@pytest.mark.parametrize("name,build", BUILDERS, ids=[b[0] for b in BUILDERS])
def test_inputs_are_deterministic_and_the_oracle_takes_them(name, build):
    data, keys = build()
    assert (data, keys) == build()
    assert max(data) < 0x80
    want, detail = po.call_consensus_sites(data, keys, set(), po.CallerParams(13, 0.6, 3, 0, 0.0))
    assert len(want) == len(keys) and set(detail) == set(keys)


def test_window_edge_lines_have_the_lengths_and_placements_asked_for():
    for term in (b"\n", b"\r\n"):
        data, keys = cases.window_edges(term)
        lines = data.split(term)[:-1]
        start, found, starts = 0, [], []
        for ln in lines:
            if ln.startswith(cases.CHROM + b"\t"):
                found.append(len(ln) + len(term))
                starts.append(start)
            start += len(ln) + len(term)
        n = len(cases.LENGTHS)
        assert found == list(cases.LENGTHS) * 4 and len(keys) == 4 * n
        assert lines[0].startswith(cases.CHROM) and lines[-1].startswith(cases.CHROM)
        assert all(s % 16 == 15 for s in starts[n + 1:2 * n]) and all(s % 4096 == 4088 for s in starts[2 * n:3 * n]) and all(s % 4096 == 0 for s in starts[3 * n:])


def test_bases_fields_hold_single_counts_past_255_and_511():
    data, keys = cases.bases_field_edges()
    _, detail = po.call_consensus_sites(data, keys, set(), po.CallerParams(0, 0.6, 3, 0, 0.0))
    top = [max(rec.forward_base_good_depth.values() or [0]) for rec, _, _ in detail.values()]
    assert max(top) == 513 and sum(1 for t in top if t >= 512) >= 4 and sum(1 for t in top if 256 <= t < 511) >= 4


def test_fuzz_slice_covers_400_to_2300_bytes_and_crosses_2_kib():
    for k in range(5):
        data, keys = cases.fuzz_slice(100 + k)
        sizes = [len(ln) + 1 for ln in data.split(b"\n")[:-1]]
        assert len(sizes) == 300 and 400 <= min(sizes) < 450 and 2250 < max(sizes) <= 2310
        assert sum(1 for n in sizes if n > 2048) >= 20 and sum(1 for n in sizes if 1024 < n <= 2048) >= 100


def test_markers_sit_on_the_last_byte_of_every_window():
    data, keys = cases.window_marker_edges()
    start, seen = 0, set()
    for ln in data.split(b"\n")[:-1]:
        if ln.startswith(cases.CHROM + b"\t"):
            assert start % 16 == 0
            for win in (128, 256, 512, 1024, 2048):
                for m in cases.MARKERS + (b"-105",):
                    full = 109 if m == b"-105" else len(m)          # (the deletion marker with its 105 bases)
                    for at in (win - full, win - 1, win, win - 2):
                        if ln[at:at + len(m)] == m:
                            seen.add((win, m, at - win if at != win - full else -len(m)))
        start += len(ln) + 1
    for win in (128, 256, 512, 1024, 2048):
        for m in cases.MARKERS + (b"-105",):
            assert {(win, m, -len(m)), (win, m, -1), (win, m, 0)} <= seen, (win, m)
        assert (win, b"-105", -2) in seen                        # '-1' inside the window, '05' behind it


def test_routing_batch_has_a_malformed_long_unlisted_line():
    data, keys = cases.routing_batch()
    bad = [ln for ln in data.split(b"\n")[:-1] if len(ln.split(b"\t")) == 5]
    assert len(bad) == 1 and len(bad[0]) > 690 and (bad[0].split(b"\t")[0], 999) not in set(keys)
