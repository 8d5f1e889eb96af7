"""The in-order staging ring of csrc/stream.hip (Ring) driven through its wrap by each consumer that takes its reader and
staging counts from the CPU budget: vcf_stream (count and merge), pass B of varscan_stream behind a resident prefix, and load_raw.
With one CPU core the budget gives one reader and min(1 + 4, jobs) staging buffers, so every test here has more jobs than buffers:
a wrong place in the ring, a wrong base or a buffer handed back too early shows as text from the wrong piece.  (run_stream's ring
takes its counts from options: tests/test_gpu_stream.py wraps that one.)  Expected results come from the oracles on a small block
of text, replicated with shifted offsets."""
import contextlib

import numpy as np
import pytest

from oracle import fuzz
from oracle import threshold_cases as tc
from oracle import varscan_oracle as vo
from snp_pipeline_amd import _lib as L
from snp_pipeline_amd import device as dev

pytestmark = pytest.mark.gpu

MIB = 1 << 20
VARSCAN_EXTRA = "--min-var-freq 0.2 --min-reads2 2"
FIELDS = ("line_off", "sdp", "dp", "total", "rdf", "rdr", "ref_qual_sum", "adf", "adr", "alt_qual_sum", "ref_base", "alt_base")


@pytest.fixture(scope="module")
def d():
    from gpu_util import get_device
    return get_device()


@contextlib.contextmanager
def _one_reader_five_buffers():
    """One CPU core: snpgpu_reader_threads() == 1, so the ring is min(1 + 4, jobs) buffers.  The setting is process-wide."""
    dev.set_max_cpu_cores(1)
    try:
        assert dev.cpu_budget()["readers"] == 1
        yield
    finally:
        dev.set_max_cpu_cores(0)


def _params():
    from snp_pipeline_amd import varscan
    return varscan.Options(VARSCAN_EXTRA).device_params(), vo.Params(min_var_freq=0.2, min_reads2=2)


def _block(seed, n_lines, at_most):
    """Whole lines of a fuzzed pileup, at most `at_most` bytes of them."""
    data = fuzz.varscan_pileup(seed, n_lines)
    block = data[:data.rfind(b"\n", 0, at_most) + 1]
    assert at_most * 3 // 4 < len(block) <= at_most and len(block) & (len(block) - 1)        # (no power of two: piece edges fall inside lines)
    return block


def _table(recs):
    return np.stack([recs[f].astype(np.int64) for f in FIELDS], axis=1).reshape(-1, len(FIELDS))


def _want_table(block, reps, limit, prm):
    """The oracle's records of `block`, once per repetition with line_off shifted, as far as the lines start before `limit`."""
    e = np.array(tc.varscan_records(block, prm), dtype=np.int64).reshape(-1, len(FIELDS))
    assert len(e) > 5
    t = np.tile(e, (reps, 1))
    t[:, 0] += np.repeat(np.arange(reps, dtype=np.int64) * len(block), len(e))
    return t[t[:, 0] < limit]


# ---- vcf_stream ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vcf_tree(tmp_path_factory):
    """Nine small VCF files (one of them a header alone), a file of no bytes and a path that does not exist: eleven one-piece jobs."""
    from test_gpu_merge_vcfs import _tree
    root = tmp_path_factory.mktemp("ring_vcf")
    paths, texts = _tree(root, 918, 9, 150, empty=(4,))
    assert all(150 < t.count(b"\n") < 600 for i, t in enumerate(texts) if i != 4)
    (root / "nothing.vcf").write_bytes(b"")
    return root, paths, texts


def test_vcf_count_stream_wraps_the_ring(d, vcf_tree):
    from snp_pipeline_amd import collect_metrics as cm
    root, paths, texts = vcf_tree
    nothing, missing = str(root / "nothing.vcf"), str(root / "missing.vcf")
    order = paths[:3] + [nothing] + paths[3:7] + [missing] + paths[7:]
    text_of = dict(zip(paths, texts))
    text_of[nothing] = b""
    with _one_reader_five_buffers():
        got = d.vcf_count_snps_files(order)
    assert len(got) == 11
    for path, res in zip(order, got):
        if path == missing:
            assert isinstance(res, IOError), res               # SNPGPU_E_IO of that file alone
            continue
        data = text_of[path]
        snps, n_data, n_unusual, usual_snps = cm.count_snps_text(data)
        assert res[:3] == (usual_snps, n_data, n_unusual), path
        if n_unusual <= 64 and not res[4]:
            assert res[3] == [off for off, line, raw in cm.data_lines(data) if cm.is_unusual_line(line, raw)], path
    assert got[3][:3] == (0, 0, 0) and sum(r[1] for r in got if not isinstance(r, IOError)) > 2000


def test_vcf_merge_stream_wraps_the_ring(d, vcf_tree, tmp_path):
    from test_gpu_merge_vcfs import _merge_and_compare
    root, paths, texts = vcf_tree
    with _one_reader_five_buffers():
        stats, want = _merge_and_compare(d, tmp_path, paths, texts)
    assert stats["columns"] == 9 and stats["sites"] == sum(1 for l in want.split(b"\n") if l and not l.startswith(b"#")) > 300


# ---- varscan_stream, pass B behind a resident prefix -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nine_pileups(tmp_path_factory):
    """Nine pileups of about 100 KB, each a block of its own four times over, with the oracle's records of each."""
    root = tmp_path_factory.mktemp("ring_pileups")
    _, prm = _params()
    paths, sizes, want, lines = [], [], [], []
    for i in range(9):
        block = _block(40 + i, 500, 25000 + 700 * i)
        data = block * 4
        path = str(root / ("p%d.pileup" % i))
        with open(path, "wb") as f:
            f.write(data)
        paths.append(path)
        sizes.append(len(data))
        want.append(_want_table(block, 4, len(data), prm))
        lines.append(data.count(b"\n"))
    return root, paths, sizes, want, lines


@pytest.mark.parametrize("unreadable", [None, 3])
def test_ingest_past_the_budget_wraps_the_ring_of_pass_b(d, nine_pileups, unreadable):
    """A store whose budget holds the first two files: they are copied in any order (pass A, jobs [0, 2)); the other seven are
    in-order jobs [2, 9) on a ring of five.  With file 3 unreadable its job is an empty one, and its neighbours' are as before."""
    root, paths, sizes, want, lines = nine_pileups
    prm, _ = _params()
    paths = list(paths)
    if unreadable is not None:
        paths[unreadable] = str(root / "missing.pileup")
    # room for files 0 and 1 with their padding (two tail pads of a scan tile + 512 bytes, two roundings to 256), not for file 2 as well
    budget = sizes[0] + sizes[1] + 40 * 1024
    assert 40 * 1024 < sizes[2]
    store = d.pileups(budget)
    try:
        with _one_reader_five_buffers():
            sites, counts, status, rcs = store.ingest(paths, prm, capacity=4096)
        st = store.stats()
        assert (st.n_files, st.n_resident, st.n_readers) == (9, 2, 1)
        assert st.h2d_bytes == st.file_bytes == sum(s for f, s in enumerate(sizes) if f != unreadable)
        for f in range(9):
            ptr, nbytes = store.get(f)
            if f == unreadable:
                assert rcs[f] == L.E_IO and counts[f] == 0 and (ptr, nbytes) == (0, 0)
                continue
            assert rcs[f] == 0 and int(status[f, 0]) == 2 ** 64 - 1 and int(status[f, 1]) == lines[f], f
            assert np.array_equal(_table(sites[f, :counts[f]]), want[f]), f
            assert nbytes == sizes[f] and (ptr != 0) == (f < 2), f
    finally:
        store.close()


# ---- load_raw --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sixty_kib_block():
    return _block(77, 1200, 61000)


@pytest.mark.parametrize("size,pieces", [(32 * MIB, 6), (32 * MIB + 40000, 7)])
def test_load_raw_wraps_the_ring(d, tmp_path, sixty_kib_block, size, pieces):
    """One file of 1 + 1 + 2 + 4 + 8 + 16 MiB pieces (+ a short tail) on a ring of five: the ring wraps by exactly one, and by two."""
    block = sixty_kib_block
    prm, oracle_prm = _params()
    reps = size // len(block) + 1
    text = (block * reps)[:size]
    cut = text.rfind(b"\n", 0, size - 14) + 1                  # whole lines of the repeated block up to here, then one filler line of depth 0
    data = text[:cut] + b"pad" + b"x" * (size - cut - 14) + b"\t1\tA\t0\t*\t*\n"
    assert len(data) == size and sum(1 for c in range(8) if sum([1, 1, 2, 4, 8, 16, 16, 16][:c]) * MIB < size) == pieces
    path = str(tmp_path / "big.pileup")
    with open(path, "wb") as f:
        f.write(data)
    want = _want_table(block, reps, cut, oracle_prm)
    assert 1000 < len(want) < 60000
    with _one_reader_five_buffers():
        recs, n_lines = d.varscan_file(path, prm, capacity=65536)
    assert n_lines == data.count(b"\n")
    got = _table(recs)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:5]
