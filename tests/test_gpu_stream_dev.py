"""The streamed call that leaves its rows on the device (snpgpu_call_consensus_files_dev, csrc/stream.hip).

It is the host form ``call_consensus_files`` with another destination: the kernels of file f write row f of the caller's
[n_files][n_sites] device arrays, only status words and return codes come back through pinned memory.  So every case runs both
forms on the same files and the same site set and compares them byte for byte — bases, filters, count records, line offsets,
status words, return codes, and the spill arena as read after each call — with the minimum chunk size and two slots, so that a
250 KB file spans four chunks and slots are reused.  Around the device arrays stands a guard pattern (a row of padding behind
the last row included): nothing outside [n_files][n_sites] may change.  One case goes to the oracle, so that two forms that are
wrong alike cannot pass.
"""
import random

import numpy as np
import pytest

from oracle import fuzz
from oracle import pileup_oracle as po

pytestmark = pytest.mark.gpu

CHUNK = 65536
GUARD = 0xA5
MANY = b"ACGTNRYKMSWBacgtnrykmswb"           # 24 distinct symbols: 16 of them go to the position's spill record


@pytest.fixture(scope="module")
def d():
    from tests.gpu_util import get_device
    dev = get_device()
    dev.use_torch_stream()
    return dev


def _rewrite_line(data, pos, change):
    """`data` with the fields of the line of synth_chr1:`pos` changed by `change(fields)`."""
    lines = data.split(b"\n")
    k = next(i for i, ln in enumerate(lines) if ln.startswith(b"synth_chr1\t%d\t" % pos))
    f = lines[k].split(b"\t")
    change(f)
    lines[k] = b"\t".join(f)
    return b"\n".join(lines)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """The pileups of every case, written once: name -> (path, bytes).  skip_frac=0: every position of a full-size file has a line."""
    tmp = tmp_path_factory.mktemp("stream_dev")
    datas = {}
    for k in range(5):
        datas["f%d" % k] = fuzz.synth_pileup(300 + k, genome_len=3000, n_sites=10, skip_frac=0.0)[0]
        assert 3 * CHUNK < len(datas["f%d" % k]) < 5 * CHUNK          # several chunks each
    big = datas["f0"]
    datas["short"] = big[:big.rindex(b"\n", 0, 20000) + 1]           # shorter than one chunk
    keep = big.rindex(b"\n", 0, CHUNK - 40) + 1
    tail = b"synth_chr1\t2999999\tA\t0\t*\t"
    datas["one_chunk"] = big[:keep] + tail + b"x" * (CHUNK - keep - len(tail))
    assert len(datas["one_chunk"]) == CHUNK
    datas["empty"] = b""

    def bad_pos(f):
        f[1] = b"12x"
    datas["malformed"] = _rewrite_line(datas["f1"], 1500, bad_pos)

    def many(f):
        f[3], f[4], f[5] = b"24", MANY, b"I" * 24

    def long_ref(f):
        f[2] = b"AC"
    datas["many0"] = _rewrite_line(_rewrite_line(datas["f2"], 700, many), 2100, long_ref)
    datas["many1"] = _rewrite_line(datas["f3"], 2900, many)
    out = {}
    for name, data in datas.items():
        p = tmp / (name + ".pileup")
        p.write_bytes(data)
        out[name] = (str(p), data)
    out["missing"] = (str(tmp / "absent.pileup"), None)
    return out


def _keys(n, seed=5, must=()):
    rng = random.Random(seed)
    pos = set(must)
    pool = [p for p in range(1, 3001) if p not in pos]
    pos.update(rng.sample(pool, n - len(pos)))
    return [(b"synth_chr1", p) for p in sorted(pos)]


def _siteset(d, keys, excluded_every=0):
    from snp_pipeline_amd import _lib as L
    return d.siteset(keys, [L.SITE_IN_SNPLIST | (L.SITE_EXCLUDED if excluded_every and i % excluded_every == 0 else 0) for i in range(len(keys))])


def _both_forms(d, ss, paths, prm, counts=True, lines=True, depth=False, exclude=None, n_slots=2):
    """The host form and the device form over the same files.  Returns (host results, host rcs, device form as a dict of host
    copies: base, filt, counts, line, status, rcs, spill) after checking the guard cells of the device arrays."""
    import torch
    from snp_pipeline_amd import device as devmod
    n_files, n = len(paths), len(ss)
    kw = dict(chunk_bytes=CHUNK, n_slots=n_slots, n_readers=2)
    results, rcs, st_host = d.call_consensus_files(ss, paths, prm, want_counts=counts, want_line_offsets=lines, want_depth_sum=depth, exclude=exclude, **kw)
    # a guard row in front of the arrays and one behind them; the rows themselves start at any byte alignment (row f at f * n)
    shape = (n_files + 2, max(n, 1))
    t_base = torch.full(shape, GUARD, dtype=torch.uint8, device="cuda")
    t_filt = torch.full(shape, GUARD, dtype=torch.uint8, device="cuda")
    t_cnt = torch.full(shape + (128,), GUARD, dtype=torch.uint8, device="cuda") if counts else None
    t_line = torch.full(shape, 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda") if lines else None
    torch.cuda.synchronize()
    first = max(n, 1)                                          # elements of the guard row in front
    status, rcs_dev, st_dev = d.call_consensus_files_dev(
        ss, paths, prm, t_base.data_ptr() + first, t_filt.data_ptr() + first, d_counts=t_cnt.data_ptr() + 128 * first if counts else 0,
        d_line_off=t_line.data_ptr() + 8 * first if lines else 0, want_depth_sum=depth, exclude=exclude, **kw)
    spill = d.read_symbol_spill() if counts else None
    torch.cuda.synchronize()
    assert st_dev.bytes == st_host.bytes and st_dev.n_chunks == st_host.n_chunks
    got = {"status": status, "rcs": rcs_dev, "spill": spill}
    for name, t in (("base", t_base), ("filt", t_filt), ("counts", t_cnt), ("line", t_line)):
        if t is None:
            got[name] = None
            continue
        h = t.cpu().numpy()
        pattern = 0x5A5A5A5A5A5A5A5A if name == "line" else GUARD
        assert (h[0] == pattern).all() and (h[n_files + 1] == pattern).all(), "%s: a guard row changed" % name
        if n == 0:
            assert (h == pattern).all(), "%s: written with an empty site set" % name
        body = h[1:n_files + 1, :n]
        if name == "counts":
            body = np.ascontiguousarray(body).view(devmod.COUNTS_DTYPE).reshape(n_files, n)
        elif name == "line":
            body = body.view(np.uint64)
        got[name] = body
    return results, rcs, got


def _assert_equal_records(c_dev, spill_dev, c_host, spill_host, f):
    """The count records of one file, byte for byte.  A record's spill index (n_symbols >> 8) is its place in the call's arena,
    and the call kernels take those places with an atomic counter in whatever order the waves get there: so the indices are
    compared through what they point at — the spill records themselves, byte for byte."""
    a, b = c_dev.copy(), c_host.copy()
    ia, ib = a["n_symbols"] >> 8, b["n_symbols"] >> 8
    assert ((ia != 0) == (ib != 0)).all(), f
    a["n_symbols"] &= 0xFF
    b["n_symbols"] &= 0xFF
    assert a.tobytes() == b.tobytes(), f
    for slot in np.flatnonzero(ia):
        assert spill_dev[int(ia[slot]) - 1].tobytes() == spill_host[int(ib[slot]) - 1].tobytes(), (f, slot)


def _assert_equal_forms(results, rcs, got, counts=True, lines=True, void=()):
    """Byte for byte; `void`: the files whose host rows are void (E_IO) — theirs are '-' / 0 / 0 on the device."""
    assert list(got["rcs"]) == list(rcs)
    for f, r in enumerate(results):
        assert got["status"][f].tolist() == r.status.tolist(), f
        if f in void:
            assert (got["base"][f] == 0x2D).all() and (got["filt"][f] == 0).all(), f
            if lines:
                assert (got["line"][f] == 0).all(), f
            if counts:
                assert not got["counts"][f].view(np.uint8).any(), f
            continue
        assert bytes(got["base"][f]) == bytes(r.bases), f
        assert bytes(got["filt"][f]) == bytes(r.filters), f
        if lines:
            assert got["line"][f].tolist() == r.line_offsets.tolist(), f
        if counts:
            _assert_equal_records(got["counts"][f], got["spill"], r.counts, r.spill, f)
    if counts and results:
        host_spill = results[0].spill
        assert (0 if host_spill is None else len(host_spill)) == len(got["spill"])


def _params():
    from snp_pipeline_amd import device as devmod
    return devmod.make_params(15, 0.9, 5, 2, 0.1)


@pytest.mark.parametrize("names", [
    ("f0",), ("f0", "f1"), ("f0", "f1", "f2"), ("f0", "f1", "f2", "f3", "f4"),          # slot reuse; harvest before and after the last file
    ("f0", "short", "one_chunk", "f1"), ("f0", "empty", "f1"), ("empty",), ("f0", "f1", "empty"),
])
def test_device_rows_equal_the_host_form(d, files, names):
    ss = _siteset(d, _keys(257), excluded_every=9)
    paths = [files[n][0] for n in names]
    results, rcs, got = _both_forms(d, ss, paths, _params())
    assert list(rcs) == [0] * len(names)
    _assert_equal_forms(results, rcs, got)
    assert any(r.counts["status"].any() for r in results) or names == ("empty",)       # (the case is not vacuous)


@pytest.mark.parametrize("n_sites", [0, 1, 255, 257, 1001])
@pytest.mark.parametrize("counts, lines", [(True, True), (False, True), (True, False), (False, False)])
def test_any_row_alignment_with_and_without_counts_and_line_offsets(d, files, n_sites, counts, lines):
    """Odd site counts: row f starts at byte f * n_sites of the base and filter arrays, at any alignment."""
    ss = _siteset(d, _keys(n_sites)) if n_sites else d.siteset([], [])
    paths = [files[n][0] for n in ("f1", "short", "f2")]
    results, rcs, got = _both_forms(d, ss, paths, _params(), counts=counts, lines=lines)
    assert list(rcs) == [0, 0, 0]
    _assert_equal_forms(results, rcs, got, counts=counts, lines=lines)


def test_a_missing_file_and_a_malformed_one_between_good_files(d, files):
    from snp_pipeline_amd import _lib as L
    ss = _siteset(d, _keys(255, must=(1500,)))
    names = ("f0", "missing", "f2", "malformed", "f4")
    results, rcs, got = _both_forms(d, ss, [files[n][0] for n in names], _params())
    assert list(got["rcs"]) == [0, L.E_IO, 0, L.E_PILEUP, 0]
    _assert_equal_forms(results, rcs, got, void=(1,))                 # (status words included: where the malformed line is)
    assert got["status"][3][0] != 0xFFFFFFFFFFFFFFFF and (int(got["status"][3][0]) & 0xFF) == 2
    # the neighbours are untouched by the void file: they are what each gives alone
    for f in (0, 2, 4):
        alone, _, _ = d.call_consensus_files(ss, [files[names[f]][0]], _params(), want_counts=True, want_line_offsets=True, chunk_bytes=CHUNK)
        assert bytes(got["base"][f]) == bytes(alone[0].bases)
        _assert_equal_records(got["counts"][f], got["spill"], alone[0].counts, alone[0].spill, f)


def test_per_file_exclude_lists_and_the_depth_sum(d, files):
    from snp_pipeline_amd import _lib as L
    keys = _keys(255)
    ss = _siteset(d, keys)
    names = ("f0", "f1", "f2")
    exclude = [np.arange(0, 255, 3), np.zeros(0, np.int64), np.asarray([254, 1, -1, 77])]
    results, rcs, got = _both_forms(d, ss, [files[n][0] for n in names], _params(), depth=True, exclude=exclude)
    _assert_equal_forms(results, rcs, got)
    assert (got["filt"][0][0::3] & L.F_REGION).all() and not (got["filt"][1] & L.F_REGION).any()
    assert sorted(np.flatnonzero(got["filt"][2] & L.F_REGION)) == [1, 77, 254]
    for f, n in enumerate(names):
        want = sum(int(fl[3]) for _, ln in po.iter_lines(files[n][1]) for fl in [ln.split()] if len(fl) > 3)
        assert int(got["status"][f][3]) == want == results[f].depth_sum


def test_spill_records_of_several_files_are_one_arena(d, files):
    """Two files with a line of 24 distinct symbols each, one of them also with a reference field of two bytes: the spill indices
    of the records point into the one arena of the call, and the VCF rows made from both forms are the same text."""
    from snp_pipeline_amd import _lib as L
    from snp_pipeline_amd import vcf_writer
    keys = _keys(257, must=(700, 2100, 2900))
    ss = _siteset(d, keys)
    names = ("many0", "f0", "many1")
    results, rcs, got = _both_forms(d, ss, [files[n][0] for n in names], _params())
    assert list(rcs) == [0, 0, 0]
    _assert_equal_forms(results, rcs, got)
    assert len(got["spill"]) == 3
    pointed = [int(v) >> 8 for f in range(3) for v in got["counts"][f]["n_symbols"] if int(v) >> 8]
    assert sorted(pointed) == [1, 2, 3]                               # every record of the arena is some row's, across the files
    filter_names = ["RawDpth", "VarFreq", "Depth", "StrDpth", "StrBias", "Region"]
    n_rows = 0
    for f in range(3):
        order = np.flatnonzero(got["counts"][f]["status"] == L.ST_OK)
        order = order[np.argsort(got["line"][f][order], kind="stable")]
        rows_dev = vcf_writer.format_rows(got["counts"][f], order, ss._names, ss._offs, ss.keys, filter_names, False, ".", spill=got["spill"])
        rows_host = vcf_writer.format_rows(results[f].counts, order, ss._names, ss._offs, ss.keys, filter_names, False, ".", spill=results[f].spill)
        assert rows_dev == rows_host and rows_dev
        n_rows += rows_dev.count(b"\n")
        if f != 1:
            row = next(ln for ln in rows_dev.split(b"\n") if ln.startswith(b"synth_chr1\t%d\t" % (700 if f == 0 else 2900)))
            assert row.split(b"\t")[4].count(b",") >= 9               # ten or more ALT alleles: ranks 8.. came from the arena
    assert n_rows > 700


def test_device_rows_against_the_oracle(d, files):
    from snp_pipeline_amd import _lib as L
    keys = _keys(255)
    ss = _siteset(d, keys, excluded_every=7)
    names = ("f3", "short", "f4")
    _, _, got = _both_forms(d, ss, [files[n][0] for n in names], _params())
    excl = {k for k, fl in zip(ss.key_tuples(), ss.flags) if fl & L.SITE_EXCLUDED}
    p = po.CallerParams(15, 0.9, 5, 2, 0.1)
    for f, n in enumerate(names):
        want, detail = po.call_consensus_sites(files[n][1], ss.key_tuples(), excl, p)
        assert bytes(got["base"][f]) == want
        for slot, key in enumerate(ss.key_tuples()):
            c = got["counts"][f][slot]
            if key not in detail:
                assert c["status"] == L.ST_NO_LINE and got["line"][f][slot] == 0
                continue
            rec, base, mask = detail[key]
            assert (c["raw_depth"], c["good_depth"], c["cons_base"], c["filters"]) == (rec.raw_depth, rec.good_depth, base, mask), (n, key)
            off = int(got["line"][f][slot]) - 1
            assert files[n][1][off:].startswith(b"%s\t%d\t" % key)
