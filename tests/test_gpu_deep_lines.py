"""Pileup lines of deep-coverage samples — over 512 bytes, to and past 2 KiB — through the call step (csrc/consensus.hip: the three
one-lane-per-site passes hand them on, the wave-per-site kernel calls them) against oracle/pileup_oracle.py through the C ABI:
bases, filter masks, count records (with and without per-site counts: gpu_util.check_against_oracle runs both chains), and which
pass took which line (Device.call_pass_counts against deep_lines_cases.expected_passes, line by line).  The inputs are those of tests/deep_lines_cases.py, which the oracle is run over on the CPU too."""
import os

import numpy as np
import pytest

from oracle import pileup_oracle as po
from snp_pipeline_amd import _lib as L
from snp_pipeline_amd import device as dev
from tests import deep_lines_cases as cases
from tests.gpu_util import check_against_oracle, get_device, gpu_consensus

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def d():
    return get_device()


def _line_offsets_match(d, data, keys, ss):
    """1 + offset of every listed line, as the scan left it."""
    off = d.line_offsets(ss)
    want = {}
    start = 0
    for ln in data.splitlines(keepends=True):
        f = ln.split(b"\t")
        want[(f[0], int(f[1]))] = start + 1
        start += len(ln)
    for slot, key in enumerate(ss.key_tuples()):
        assert int(off[slot]) == want.get(key, 0), key


@pytest.mark.parametrize("term,reverse", [(b"\n", False), (b"\r\n", False), (b"\n", True), (b"\r\n", True)])
def test_window_edges(d, term, reverse):
    data, keys = cases.window_edges(term, reverse)
    for p in (po.CallerParams(0, 0.6, 3, 0, 0.0), po.CallerParams(20, 0.6, 3, 2, 0.1)):
        check_against_oracle(d, data, keys, [keys[3]], p)
    _, _, ss = gpu_consensus(d, data, keys, [], po.CallerParams())
    _line_offsets_match(d, data, keys, ss)
    assert d.call_pass_counts() == cases.expected_passes(data, set(keys), term)


def test_bases_field_edges(d):
    data, keys = cases.bases_field_edges()
    for p in (po.CallerParams(0, 0.6, 3, 0, 0.0), po.CallerParams(10, 0.9, 300, 200, 0.4)):
        res = check_against_oracle(d, data, keys, [], p)
    assert int(res.counts["total"][:, 0].max()) == 513             # a single count past 512 came through the record
    assert d.call_pass_counts() == cases.expected_passes(data, set(keys)) == {"lanes128": 0, "lanes256": 0, "lanes512": 0, "wave": len(keys)}


def test_markers_at_mask_word_edges(d):
    data, keys = cases.marker_edges()
    for p in (po.CallerParams(0, 0.6, 3, 0, 0.0), po.CallerParams(13, 0.5, 1, 1, 0.0)):
        check_against_oracle(d, data, keys, [], p)
    assert d.call_pass_counts() == cases.expected_passes(data, set(keys))


def test_markers_at_window_ends(d):
    """A marker cut by the end of a window: the pass of that window hands the line on, the next that holds it whole calls it."""
    data, keys = cases.window_marker_edges()
    for p in (po.CallerParams(0, 0.6, 3, 0, 0.0), po.CallerParams(13, 0.5, 1, 1, 0.0)):
        check_against_oracle(d, data, keys, [], p)
    took = d.call_pass_counts()
    assert took == cases.expected_passes(data, set(keys)) and took["lanes256"] and took["lanes512"] and took["wave"]


def test_quality_threshold_at_the_field_edges(d):
    data, keys = cases.quality_edges()
    check_against_oracle(d, data, keys, [], po.CallerParams(13, 0.6, 3, 0, 0.0))
    check_against_oracle(d, data, keys, [], po.CallerParams(14, 0.6, 3, 0, 0.0))


def test_routing_is_reported_per_pass(d):
    """Fails where the library has no snpgpu_call_pass_counts."""
    data, keys = cases.routing_batch()
    assert len(keys) == 64
    for want_counts in (True, False):
        got, res, ss = gpu_consensus(d, data, keys, [], po.CallerParams(0, 0.6, 3, 0, 0.0), want_counts=want_counts)
        assert got == po.call_consensus_sites(data, keys, set(), po.CallerParams(0, 0.6, 3, 0, 0.0))[0]
        took = d.call_pass_counts()
        # 57 short lines and the 100-byte one; nothing for the 256-byte window; 300; then 600, 1100, 1500, 2100 and the line of R's
        assert took == {"lanes128": 58, "lanes256": 0, "lanes512": 1, "wave": 5} == cases.expected_passes(data, set(keys))
        assert sum(took.values()) == int((d.line_offsets(ss) != 0).sum()) == 64


def test_all_lines_chain(d, tmp_path):
    """call_consensus --vcfAllPos: the same chain over every line of a file; rows by oracle/vcf_oracle.py."""
    from oracle import vcf_oracle
    data, keys = cases.all_lines_file()
    path = os.path.join(str(tmp_path), "reads.all.pileup")
    with open(path, "wb") as f:
        f.write(data)
    p = po.CallerParams(13, 0.6, 3, 0, 0.0)
    ss = d.siteset(keys[::3], [L.SITE_IN_SNPLIST] * len(keys[::3]))
    off, flags, counts = d.call_all_lines(ss, path, dev.make_params(13, 0.6, 3, 0, 0.0))
    took = d.call_pass_counts()
    assert len(off) == len(keys) == sum(took.values())
    # every line by the window it fits, counted from the 16-byte boundary below its first byte
    assert took == cases.expected_passes(data) and took["wave"] >= 20
    _, detail = po.call_consensus_sites(data, keys, set(), p)
    names = po.filter_names(p)
    for i, key in enumerate(keys):
        rec, base, mask = detail[key]
        c = counts[i]
        got = po.Record(key[0], key[1], bytes([int(c["ref_base"])]), int(c["raw_depth"]))
        n = int(c["n_symbols"]) & 0xFF
        got.most_common_good_bases = [int(s) for s in c["sym"][:n]] if n else None
        got.base_good_depth = {int(c["sym"][r]): int(c["total"][r]) for r in range(n)}
        got.forward_base_good_depth = {int(c["sym"][r]): int(c["fwd"][r]) for r in range(n)}
        got.reverse_base_good_depth = {int(c["sym"][r]): int(c["rev"][r]) for r in range(n)}
        failed = lambda m: [nm for b, nm in enumerate(names) if m >> b & 1] or None      # noqa: E731
        assert vcf_oracle.vcf_row(got, failed(int(c["filters"]))) == vcf_oracle.vcf_row(rec, failed(mask)), key
        assert int(c["cons_base"]) == base and int(c["good_depth"]) == rec.good_depth


@pytest.mark.parametrize("k", range(5))
def test_seeded_fuzz_slice(d, k):
    data, keys = cases.fuzz_slice(100 + k)
    check_against_oracle(d, data, keys, keys[5::40], po.CallerParams(*cases.FUZZ_PARAMS[k]))
    took = d.call_pass_counts()
    # (a line of odd symbols or adversarial strings may leave its window for reasons the length does not show: the lane passes
    # take at most what expected_passes gives them)
    want = cases.expected_passes(data, set(keys))
    assert sum(took.values()) == len(keys) and took["wave"] >= want["wave"] > 250
    assert all(took[k] <= want[k] for k in ("lanes128", "lanes256", "lanes512"))
