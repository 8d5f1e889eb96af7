"""The glue kernels of the one-job pipeline in csrc/flows.hip, called directly: snpgpu_region_flow_dev (k_flow_gather, k_flow_exclude)
against the oracle's preserved call and the NumPy statement of its rule (tests/flows_cases.py, pinned to the oracle by
tests/test_flows_cpu.py), snpgpu_rows_copy_dev (k_rows_copy) against NumPy index assignment — at the alignments where it switches
between 16-byte and byte copies, and past the caps of the grids (the loops' second turns)."""
import numpy as np
import pytest

from snp_pipeline_amd import _lib as L
from snp_pipeline_amd import device as dev
from tests import flows_cases as fc

pytestmark = pytest.mark.gpu

GUARD = 64                       # guard bytes in front of and behind every output
FILL = 0xAB


@pytest.fixture(scope="module")
def d():
    from tests.gpu_util import get_device
    device = get_device()
    device.use_torch_stream()
    return device


@pytest.fixture(scope="module")
def n_cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _cuda(a, as_type):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(as_type)).cuda()


def _guarded(nbytes):
    """(whole buffer, data_ptr of its payload): nbytes of payload between two guards, every byte FILL."""
    import torch
    buf = torch.full((nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
    return buf, buf.data_ptr() + GUARD


def _payload_equals(buf, want):
    """The guards are intact and the payload equals `want` (a NumPy uint8 array of any shape): compared on the device."""
    import torch
    n = buf.numel() - 2 * GUARD
    assert want.size == n
    guards_ok = bool((buf[:GUARD] == FILL).all().item()) and bool((buf[GUARD + n:] == FILL).all().item())
    same = n == 0 or torch.equal(buf[GUARD:GUARD + n], torch.from_numpy(np.ascontiguousarray(want).reshape(-1)).cuda())
    return guards_ok, same


def _region_flow(d, c, null_slots=False, expect_err=0):
    """snpgpu_region_flow_dev on the arrays of a case (tests/flows_cases.small_case and the like) against fc.flow_rule: outputs,
    guards, the error word, and the inputs left as they were."""
    import torch
    n, S, n_cols = c["n_samples"], c["n_sites"], len(c["cols"])
    want_base, want_filters, want_err = fc.flow_rule(c["base"], c["filters"], c["line_off"], c["cols"], c["col_of"], c["excl_off"],
                                                     None if null_slots else c["excl_slots"])
    assert want_err == expect_err
    d_base, d_filters, d_line = _cuda(c["base"], np.uint8), _cuda(c["filters"], np.uint8), _cuda(c["line_off"], np.int64)
    d_cols = _cuda(c["cols"], np.int32) if n_cols else None
    d_col_of, d_eoff, d_es = _cuda(c["col_of"], np.int32), _cuda(c["excl_off"], np.int32), _cuda(c["excl_slots"], np.int32)
    inputs = [(t, t.clone()) for t in (d_base, d_filters, d_line, d_col_of, d_eoff, d_es) + ((d_cols,) if n_cols else ())]
    ob, p_ob = _guarded(n * n_cols)
    of, p_of = _guarded(n * S)
    err = torch.tensor([0x5A5A5A5A, 0, 0x5A5A5A5A], dtype=torch.int32, device="cuda")
    d.region_flow_dev(d_base.data_ptr(), d_filters.data_ptr(), d_line.data_ptr(), n, S, d_cols.data_ptr() if n_cols else 0, d_col_of.data_ptr(), n_cols,
                      d_eoff.data_ptr(), 0 if null_slots else d_es.data_ptr(), p_ob if n_cols else 0, p_of, err.data_ptr() + 4)
    torch.cuda.synchronize()
    assert _payload_equals(of, want_filters) == (True, True)
    assert _payload_equals(ob, want_base) == (True, True)
    assert err.cpu().tolist() == [0x5A5A5A5A, want_err, 0x5A5A5A5A]
    for t, before in inputs:
        assert torch.equal(t, before)
    return want_base, want_filters


# ---- region_flow_dev ------------------------------------------------------------------------------------------------------------
def test_region_flow_against_the_oracles_preserved_call(d):
    """Three samples called at the full list on the device, the preserved flow derived there, against the oracle's preserved call."""
    import torch
    from oracle import pileup_oracle as po
    samples, full, preserved = fc.oracle_samples(fc.ORACLE_SEEDS[:3])
    n, S = len(samples), len(full)
    ss = d.siteset(full, [L.SITE_IN_SNPLIST] * S)
    assert ss.key_tuples() == full                                         # slot i is full[i]
    pile = [torch.cat([torch.frombuffer(bytearray(data), dtype=torch.uint8), torch.full((64,), 0x0A, dtype=torch.uint8)]).cuda() for data, _ in samples]
    cols, col_of, excl_off, excl_slots = fc.flow_inputs(full, preserved, [e for _, e in samples])
    d_cols, d_col_of, d_eoff, d_es = _cuda(cols, np.int32), _cuda(col_of, np.int32), _cuda(excl_off, np.int32), _cuda(excl_slots, np.int32)
    for p in (po.CallerParams(0, 0.6, 1, 0, 0.0), po.CallerParams(13, 0.6, 3, 2, 0.1)):
        prm = dev.make_params(p.min_base_quality, p.min_cons_freq, p.min_cons_depth, p.min_cons_strand_depth, p.min_cons_strand_bias)
        base = torch.zeros((n, S), dtype=torch.uint8, device="cuda")
        filt = torch.zeros((n, S), dtype=torch.uint8, device="cuda")
        line = torch.zeros((n, S), dtype=torch.int64, device="cuda")
        status = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
        d.call_consensus_many_dev(ss, [t.data_ptr() for t in pile], [len(data) for data, _ in samples], prm, base.data_ptr(), filt.data_ptr(),
                                  status.data_ptr(), d_line_off=line.data_ptr())
        out_base = torch.full((n, len(cols)), FILL, dtype=torch.uint8, device="cuda")
        out_filt = torch.full((n, S), FILL, dtype=torch.uint8, device="cuda")
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        d.region_flow_dev(base.data_ptr(), filt.data_ptr(), line.data_ptr(), n, S, d_cols.data_ptr(), d_col_of.data_ptr(), len(cols), d_eoff.data_ptr(),
                          d_es.data_ptr(), out_base.data_ptr(), out_filt.data_ptr(), err.data_ptr())
        torch.cuda.synchronize()
        assert int(err[0]) == 0
        ob, of = out_base.cpu().numpy(), out_filt.cpu().numpy()
        compared = 0
        for s, (data, excluded) in enumerate(samples):
            compared += fc.check_against_oracle_preserved(data, full, preserved, excluded, p, ob[s], of[s])
        assert compared > n * len(preserved) // 2 and ((of & fc.F_REGION) != 0).any()


@pytest.mark.parametrize("excl_shape", ["mixed", "long", "none"])
@pytest.mark.parametrize("cols_shape", ["empty", "identity", "subset"])
def test_region_flow_small_cases_and_buffer_integrity(d, cols_shape, excl_shape):
    """The 3 x 37 case with every kind of exclude slot (tests/flows_cases.small_case), lists of 257 and 513 entries (the 256-thread
    stride) and no lists at all (null d_excl_slots): outputs equal the statement, guards and inputs are untouched."""
    c = fc.small_case(cols_shape, excl_shape)
    want_base, want_filters = _region_flow(d, c, null_slots=excl_shape == "none")
    if excl_shape == "none":
        assert np.array_equal(want_filters, c["filters"])
        _region_flow(d, dict(c, excl_off=np.zeros(4, dtype=np.int32)), null_slots=False)          # empty lists with a list pointer
    else:
        assert (want_filters != c["filters"]).any()
        if cols_shape != "empty":
            assert (want_base != c["base"][:, c["cols"]]).any()


@pytest.mark.parametrize("cols_shape", ["empty", "subset"])
def test_region_flow_error_word(d, cols_shape):
    """A slot equal to n_sites and one of 0xFFFFFFFF set bit 0 of the error word (the kernel's own guard) and change nothing else."""
    c = fc.small_case(cols_shape, "mixed", bad_slots=True)
    assert fc.SMALL_SITES in c["excl_slots"] and 0xFFFFFFFF in c["excl_slots"]
    _region_flow(d, c, expect_err=1)


def test_region_flow_second_turn_of_the_exclude_grid(d, n_cu):
    """More samples than k_flow_exclude has workgroups (flows.hip: grid = min(n_samples, 8 * n_cu)): the loop over samples turns twice."""
    cap = 8 * n_cu
    n, S = cap + 3, 7
    assert n > cap
    rng = np.random.default_rng(21)
    base = rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), size=(n, S)).astype(np.uint8)
    filters = rng.integers(0, 32, size=(n, S), dtype=np.uint8) * (rng.random((n, S)) < 0.3)
    filters[rng.random((n, S)) < 0.05] |= fc.F_MALFORMED
    line_off = rng.integers(1, 1 << 33, size=(n, S)).astype(np.uint64) * (rng.random((n, S)) < 0.8)
    cols = np.array([5, 0, 3, 6], dtype=np.uint32)
    lists = [sorted(rng.choice(S, size=int(rng.integers(0, 4)), replace=False)) for _ in range(n)]
    lists[cap - 1], lists[cap], lists[n - 1] = [0, 1], [3, 4], [5, 6]      # the last sample of the first turn, the first and last of the second
    excl_off, excl_slots = fc.csr(lists)
    c = dict(base=base, filters=filters.astype(np.uint8), line_off=line_off.astype(np.uint64), cols=cols, col_of=fc.col_of_cols(cols, S),
             excl_off=excl_off, excl_slots=excl_slots, n_samples=n, n_sites=S)
    _, want_filters = _region_flow(d, c)
    assert (want_filters[cap:] != filters[cap:]).any()


def test_region_flow_second_turn_of_the_gather_grid(d, n_cu):
    """More columns than k_flow_gather's grid covers in one turn (flows.hip: grid = min(ceil(n_samples * n_cols / 256), 16 * n_cu)
    workgroups of 256 threads)."""
    cap_threads = 16 * n_cu * 256
    n, S = 2, 8 * n_cu * 256 + 5
    assert n * S > cap_threads
    rng = np.random.default_rng(22)
    base = rng.choice(np.frombuffer(b"ACGTacgtN", dtype=np.uint8), size=(n, S)).astype(np.uint8)
    filters = np.zeros((n, S), dtype=np.uint8)
    line_off = np.ones((n, S), dtype=np.uint64)
    cols = rng.permutation(S).astype(np.uint32)
    lists = [[0, S - 1, int(cols[0]), int(cols[-1])], [S // 2, int(cols[S // 2])]]
    excl_off, excl_slots = fc.csr(lists)
    c = dict(base=base, filters=filters, line_off=line_off, cols=cols, col_of=fc.col_of_cols(cols, S), excl_off=excl_off, excl_slots=excl_slots,
             n_samples=n, n_sites=S)
    want_base, _ = _region_flow(d, c)
    assert int((want_base != base[:, cols]).sum()) >= 4


def test_region_flow_refusals_and_no_ops(d):
    import torch
    c = fc.small_case("subset", "mixed")
    n, S, n_cols = c["n_samples"], c["n_sites"], len(c["cols"])
    t = dict(base=_cuda(c["base"], np.uint8), filters=_cuda(c["filters"], np.uint8), line=_cuda(c["line_off"], np.int64), cols=_cuda(c["cols"], np.int32),
             col_of=_cuda(c["col_of"], np.int32), eoff=_cuda(c["excl_off"], np.int32), es=_cuda(c["excl_slots"], np.int32))
    ob, p_ob = _guarded(n * n_cols)
    of, p_of = _guarded(n * S)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")

    def call(n_samples=n, n_sites=S, **null):
        p = {k: (0 if k in null else v.data_ptr()) for k, v in t.items()}
        d.region_flow_dev(p["base"], p["filters"], p["line"], n_samples, n_sites, p["cols"], p["col_of"], n_cols, p["eoff"], p["es"], p_ob, p_of,
                          0 if "err" in null else err.data_ptr())

    def untouched():
        torch.cuda.synchronize()
        return bool((ob == FILL).all().item()) and bool((of == FILL).all().item()) and int(err[0]) == 0

    call(n_samples=0)                                                      # no samples: OK, nothing written
    assert untouched()
    for null in ("eoff", "err", "col_of"):
        with pytest.raises(dev.SnpGpuError) as ei:
            call(**{null: True})
        assert ei.value.code == L.E_ARG, null
        assert untouched(), null
    call()                                                                 # ... and the context still works
    torch.cuda.synchronize()
    want_base, want_filters, _ = fc.flow_rule(c["base"], c["filters"], c["line_off"], c["cols"], c["col_of"], c["excl_off"], c["excl_slots"])
    assert _payload_equals(ob, want_base) == (True, True) and _payload_equals(of, want_filters) == (True, True)


# ---- rows_copy_dev --------------------------------------------------------------------------------------------------------------
def _rows_copy(d, rng, n_src_rows, n_dst_rows, n_rows, row_bytes, src_stride, dst_stride, src_off=0, dst_off=0, src_index=None, dst_index=None):
    """snpgpu_rows_copy_dev against dst[dst_index[r], :row_bytes] = src[src_index[r], :row_bytes] on byte buffers: every byte of the
    destination outside the copied ranges (gaps between rows, rows not named, the guards, the bytes before dst_off) stays FILL."""
    import torch
    src_len = src_off + (n_src_rows - 1) * src_stride + row_bytes
    dst_len = dst_off + (n_dst_rows - 1) * dst_stride + row_bytes
    src = rng.integers(0, 256, size=src_len, dtype=np.uint8)
    src[src == FILL] = 0x11                                                # (a copied byte is never mistaken for an untouched one)
    want = np.full(dst_len, FILL, dtype=np.uint8)
    si = np.arange(n_rows) if src_index is None else np.asarray(src_index, dtype=np.int64)
    di = np.arange(n_rows) if dst_index is None else np.asarray(dst_index, dtype=np.int64)
    assert len(si) == len(di) == n_rows and si.max() < n_src_rows and di.max() < n_dst_rows and len(set(di.tolist())) == n_rows
    for r in range(n_rows):
        a, b = src_off + int(si[r]) * src_stride, dst_off + int(di[r]) * dst_stride
        want[b:b + row_bytes] = src[a:a + row_bytes]
    d_src = torch.from_numpy(src).cuda()
    before = d_src.clone()
    buf, p_dst = _guarded(dst_len)
    assert d_src.data_ptr() % 16 == 0 and p_dst % 16 == 0                  # the offsets alone decide the alignment of the rows
    d_si = _cuda(np.asarray(si, dtype=np.uint32), np.int32) if src_index is not None else None
    d_di = _cuda(np.asarray(di, dtype=np.uint32), np.int32) if dst_index is not None else None
    d.rows_copy_dev(d_src.data_ptr() + src_off, src_stride, p_dst + dst_off, dst_stride, n_rows, row_bytes,
                    d_src_index=d_si.data_ptr() if d_si is not None else 0, d_dst_index=d_di.data_ptr() if d_di is not None else 0)
    torch.cuda.synchronize()
    assert _payload_equals(buf, want) == (True, True), (row_bytes, src_stride, dst_stride, src_off, dst_off)
    assert torch.equal(d_src, before)


ROW_BYTES = [1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 4096, 4097, 8191, 8207]


def _strides(row_bytes):
    """row_bytes, row_bytes + 1, the next multiple of 16, and row_bytes rounded up to 8 plus 8 — with a 16-aligned base the last
    makes every other row 16-aligned (an odd multiple of 8): the 16-byte and the byte branch of k_rows_copy run in one launch."""
    return [row_bytes, row_bytes + 1, (row_bytes + 15) // 16 * 16, (row_bytes + 7) // 8 * 8 + 8]


@pytest.mark.parametrize("row_bytes", ROW_BYTES)
def test_rows_copy_alignments_and_strides(d, row_bytes):
    """Every row length around the 16-byte lane and the 256-thread x 16-byte turn of the inner loops (4096 bytes), at source offsets
    0 / 1 / 8, destination offsets 0 / 3 / 16, four strides, and the four forms of the index lists."""
    rng = np.random.default_rng(row_bytes)
    n_rows, n_src_rows, n_dst_rows = 5, 7, 8
    alternating = _strides(row_bytes)[3]
    if alternating % 16 == 0:                                              # (17, 33, 257, ...: eight more bytes make it an odd multiple of 8)
        alternating += 8
    assert alternating % 16 == 8 and alternating >= row_bytes
    forms = [(None, None), ([6, 0, 6, 3, 3], None), (None, [7, 2, 0, 5, 1]), ([1, 1, 5, 0, 6], [4, 7, 0, 2, 6])]
    k = 0
    for src_off in (0, 1, 8):
        for dst_off in (0, 3, 16):
            for stride in _strides(row_bytes):
                for si, di in forms:
                    k += 1
                    other = _strides(row_bytes)[(k // 5) % 4]              # the source's stride: every one of the four with every destination's
                    _rows_copy(d, rng, n_src_rows, n_dst_rows, n_rows, row_bytes, other, stride, src_off, dst_off, si, di)
    # both branches in one launch, for every form of the lists: 16-aligned bases and a stride that is 8 mod 16
    for si, di in forms:
        _rows_copy(d, rng, n_src_rows, n_dst_rows, n_rows, row_bytes, alternating, alternating, 0, 0, si, di)
        _rows_copy(d, rng, n_src_rows, n_dst_rows, n_rows, row_bytes, alternating, (row_bytes + 15) // 16 * 16, 0, 16, si, di)


def test_rows_copy_alternating_stride_takes_both_branches():
    """The stride 'row_bytes rounded up to 8 plus 8' is 8 mod 16 for half of the row lengths of the list: then rows alternate between
    16-aligned and not.  (For the others it is a multiple of 16, and the offsets 1 / 3 / 8 give the byte branch.)  No device work."""
    odd8 = [rb for rb in ROW_BYTES if _strides(rb)[3] % 16 == 8]
    assert odd8 and any(rb > 4096 for rb in odd8) and any(rb < 16 for rb in odd8) and any(16 < rb < 4096 for rb in odd8)


@pytest.mark.parametrize("row_bytes", [17, 33])
def test_rows_copy_second_turn_of_the_grid(d, n_cu, row_bytes):
    """More rows than k_rows_copy has workgroups (flows.hip: grid = min(n_rows, 16 * n_cu)): the loop over rows turns twice."""
    cap = 16 * n_cu
    n_rows = cap + 3
    assert n_rows > cap
    rng = np.random.default_rng(30 + row_bytes)
    stride = (row_bytes + 7) // 8 * 8 + 8
    _rows_copy(d, rng, n_rows, n_rows + 2, n_rows, row_bytes, row_bytes, stride, 0, 0, None, rng.permutation(n_rows + 2)[:n_rows])
    _rows_copy(d, rng, n_rows, n_rows, n_rows, row_bytes, stride, (row_bytes + 15) // 16 * 16, 8, 16, rng.integers(0, n_rows, size=n_rows), rng.permutation(n_rows))


@pytest.mark.parametrize("item", [1, 8, 128])
def test_rows_copy_as_the_job_calls_it(d, item):
    """hot_path._call_scattered: the rows of the resident samples of a group to their places, S = 1237 elements of 1, 8 and 128 bytes
    per row (bases and filters, line offsets, count records) and the four status words."""
    rng = np.random.default_rng(40 + item)
    S, m, g = 1237, 4, 9
    res_idx = [1, 4, 5, 8]
    _rows_copy(d, rng, m, g, m, S * item, S * item, S * item, 0, 0, None, res_idx)
    if item == 8:
        _rows_copy(d, rng, m, g, m, 4 * 8, 4 * 8, 4 * 8, 0, 0, None, res_idx)


def test_rows_copy_refusals_and_no_ops(d):
    import torch
    src = torch.arange(256, dtype=torch.uint8, device="cuda")
    buf, p_dst = _guarded(256)

    def untouched():
        torch.cuda.synchronize()
        return bool((buf == FILL).all().item())

    for kw in (dict(src_stride=31, dst_stride=32), dict(src_stride=32, dst_stride=31), dict(d_src=0), dict(d_dst=0)):
        a = dict(d_src=src.data_ptr(), src_stride=32, d_dst=p_dst, dst_stride=32)
        a.update(kw)
        with pytest.raises(dev.SnpGpuError) as ei:
            d.rows_copy_dev(a["d_src"], a["src_stride"], a["d_dst"], a["dst_stride"], 4, 32)
        assert ei.value.code == L.E_ARG, kw
        assert untouched(), kw
    d.rows_copy_dev(src.data_ptr(), 32, p_dst, 32, 0, 32)                   # no rows, no bytes: OK, nothing written
    d.rows_copy_dev(src.data_ptr(), 32, p_dst, 32, 4, 0)
    assert untouched()
    d.rows_copy_dev(src.data_ptr(), 32, p_dst, 32, 4, 32)                   # ... and the context still works
    torch.cuda.synchronize()
    assert _payload_equals(buf, np.concatenate([np.arange(128, dtype=np.uint8), np.full(128, FILL, dtype=np.uint8)])) == (True, True)
