"""BGZF-compressed pileups on the device: the inflate kernel against Python's zlib byte for byte (every block type, tree shape and
match case of tests/bgzf_cases.py, unaligned placements, plain offsets past 4 GiB), malformed blocks as statuses with nothing
written outside a block's own range, and call_consensus / call_consensus_batch on BGZF files against the same commands on the
plain files."""
import os
import shutil

import numpy as np
import pytest

from oracle import fuzz
from snp_pipeline_amd import _lib as L
from snp_pipeline_amd import device as devmod
from tests import bgzf_cases as bc
from tests.gpu_util import get_device

pytestmark = pytest.mark.gpu

GUARD = 37                                    # bytes of 0xAB in front of, between and behind the texts: odd, so every destination is unaligned
WELL_FORMED = ["stored_full", "stored_empty", "fixed", "dynamic", "memlevel1", "huffman_only", "rle", "far_matches", "hand_dynamic", "incompressible",
               "placement", "long_line", "no_eof", "eof_in_the_middle", "only_eof", "extra_subfield"]


@pytest.fixture(scope="module")
def well_formed():
    files = bc.well_formed()
    assert sorted(files) == sorted(WELL_FORMED)
    return {name: (data, bc.zlib_plain(data)) for name, data in files.items()}


def _inflate_with_guards(d, data, gaps=False):
    """Inflate a file's blocks into a buffer of 0xAB with GUARD bytes in front and behind (gaps: also between the blocks).
    Returns (status, info, host copy of the buffer, [(offset in the buffer, isize)] per block)."""
    import torch
    rc, blocks, _ = devmod.Device.bgzf_index(data)
    assert rc == 0
    at, where = GUARD, []
    for b in blocks:
        b.poff = at
        where.append((at, b.isize))
        at += b.isize + (GUARD if gaps else 0)
    total = at + GUARD
    comp = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    out = torch.full((total,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    status, info = d.bgzf_inflate_dev(comp.data_ptr(), len(data), blocks, out.data_ptr(), total)
    return status, info, out.cpu().numpy().tobytes(), where


@pytest.mark.parametrize("name", WELL_FORMED)
def test_inflate_matches_zlib(well_formed, name):
    d = get_device()
    data, plain = well_formed[name]
    status, info, buf, where = _inflate_with_guards(d, data)
    assert list(status) == [bc.ST_OK] * len(where), (name, list(status))
    assert info.n_bad == 0 and info.plain_bytes == len(plain)
    assert buf[GUARD:GUARD + len(plain)] == plain
    assert buf[:GUARD] == b"\xab" * GUARD and buf[GUARD + len(plain):] == b"\xab" * GUARD


def test_every_destination_alignment(well_formed):
    """The store of the text takes bytes up to a 16-byte boundary, 16-byte vectors, then bytes: every alignment of the first byte,
    with blocks shorter than one vector among them."""
    d = get_device()
    text = well_formed["dynamic"][1]
    sizes = [1, 2, 3, 5, 15, 16, 17, 31, 33, 47, 64, 100, 255, 1000, 4097, 3, 18, 29, 36, 51]
    parts, at = [], 0
    for n in sizes:
        parts.append(bc.make_bgzf.block(text[at:at + n]))
        at += n
    data = b"".join(parts)
    status, _, buf, where = _inflate_with_guards(d, data, gaps=True)      # GUARD = 37 is odd: the offsets walk through the residues mod 16
    assert set(status) == {bc.ST_OK}
    assert len({off % 16 for off, _ in where}) >= 12
    want = bytearray(b"\xab" * len(buf))
    at = 0
    for (off, n) in where:
        want[off:off + n] = text[at:at + n]
        at += n
    assert buf == bytes(want)


@pytest.mark.parametrize("name", sorted(bc.bad_blocks()))
def test_a_bad_block_is_a_status(name):
    """One bad block between good ones: its status names the cause, the others' text is intact, and no byte outside any block's
    own [plain offset, plain offset + ISIZE) is written (guard bytes around the buffer and between the blocks)."""
    d = get_device()
    bad, want = bc.bad_blocks()[name]
    data, texts = bc.bad_file(bad)
    status, info, buf, where = _inflate_with_guards(d, data, gaps=True)
    assert list(status) == [bc.ST_OK, want, bc.ST_OK, bc.ST_OK], (name, list(status))
    assert info.n_bad == 1 and info.bad_block == 1 and info.bad_status == want and info.bad_offset == bc.members(data)[1][0]
    expect = bytearray(b"\xab" * len(buf))
    for i in (0, 2):
        expect[where[i][0]:where[i][0] + where[i][1]] = texts[i]
    lo, n = where[1]
    # inside the bad block's own range anything may stand; everywhere else the buffer is the guards and the good text
    assert buf[:lo] == bytes(expect[:lo]) and buf[lo + n:] == bytes(expect[lo + n:])


def test_table_is_checked_before_any_launch(well_formed):
    import torch
    d = get_device()
    data, plain = well_formed["dynamic"]
    rc, blocks, _ = devmod.Device.bgzf_index(data)
    comp = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    out = torch.full((len(plain),), 0xAB, dtype=torch.uint8, device="cuda")
    with pytest.raises(L.SnpGpuError) as ei:
        d.bgzf_inflate_dev(comp.data_ptr(), len(data), blocks, out.data_ptr(), len(plain) - 1)
    assert ei.value.code == L.E_ARG and "pass the output buffer" in str(ei.value)
    with pytest.raises(L.SnpGpuError) as ei:
        d.bgzf_inflate_dev(comp.data_ptr(), len(data) - 1, blocks, out.data_ptr(), len(plain))
    assert ei.value.code == L.E_ARG and "leaves the compressed data" in str(ei.value)
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all())                                # nothing ran


def test_plain_offsets_past_4_gib():
    """70 000 copies of one compressed 65 280-byte block: a few MB of input, 4.57 GB of text.  Every row of the text must equal
    row 0, and row 0 zlib's output."""
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < 12 << 30:
        pytest.skip("needs 12 GiB of free device memory")
    d = get_device()
    line = b"chr1\t%d\tA\t30\t" + b".,.,..,,.$.,^F.,.,.,..,.,.,.,,." + b"\t" + b"IIIIIHHHHGGGFFFIIIIIHHHHGGGFFF" + b"\n"
    pattern = b"".join(line % (1000 + i) for i in range(2000))[:65280]
    block = bc.make_bgzf.block(pattern)
    n = 70000
    data = block * n
    assert bc.zlib_plain(block) == pattern
    rc, blocks, info = devmod.Device.bgzf_index(data)
    assert rc == 0 and len(blocks) == n and info.plain_bytes == n * 65280 > 1 << 32
    assert blocks[n - 1].poff == (n - 1) * 65280
    comp = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    out = torch.zeros((n, 65280), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    status, info = d.bgzf_inflate_dev(comp.data_ptr(), len(data), blocks, out.data_ptr(), n * 65280)
    assert not status.any() and info.n_bad == 0
    assert out[0].cpu().numpy().tobytes() == pattern
    assert bool((out == out[0]).all())


# ---- through the call: Device.call_consensus_files ------------------------------------------------------------------------------
_SAMPLES = {}


def _sample(seed, **kw):
    """(pileup text, its sites) of a synthetic sample, lambda-sized (48.5 kbp) unless told otherwise; generated once per session."""
    key = (seed, tuple(sorted(kw.items())))
    if key not in _SAMPLES:
        data, _, sites = fuzz.synth_pileup(seed, **dict(dict(genome_len=48502, n_sites=150), **kw))
        _SAMPLES[key] = (data, sites)
    return _SAMPLES[key]


def _odd_bgzf(data, seed):
    """BGZF with block payloads of mixed sizes, so that plain offsets are unaligned and lines straddle block and scan-tile ends."""
    sizes, parts, at, i = [1, 63, 64, 65, 4095, 4096, 4097, 65280], [], 0, seed
    while at < len(data):
        n = sizes[i % len(sizes)]
        parts.append(bc.make_bgzf.block(data[at:at + n]))
        at += n
        i += 1
    return b"".join(parts) + bc.EOF_MARKER


def _same_result(a, b):
    assert bytes(a.bases) == bytes(b.bases) and bytes(a.filters) == bytes(b.filters)
    assert a.counts.tobytes() == b.counts.tobytes()
    assert (a.line_offsets == b.line_offsets).all() and (a.status == b.status).all()


def test_mixed_list_of_plain_and_bgzf_files(tmp_path):
    """The caller's order is kept, the line offsets are those of the plain text, per-file exclude lists travel with their file, and a
    file with a bad block is E_PILEUP while the other files of the call get their results."""
    d = get_device()
    samples = [_sample(60 + i) for i in range(4)]
    sites = sorted({k for _, s in samples for k in s})
    ss = d.siteset(sites, [L.SITE_IN_SNPLIST] * len(sites))
    prm = devmod.make_params(0, 0.6, 3, 0, 0.0)
    plain_paths, mixed_paths = [], []
    for i, (data, _) in enumerate(samples):
        p = tmp_path / ("s%d.pileup" % i)
        p.write_bytes(data)
        plain_paths.append(str(p))
        if i in (1, 3):
            p = tmp_path / ("s%d.pileup.gz" % i)
            p.write_bytes(_odd_bgzf(data, i))
        mixed_paths.append(str(p))
    exclude = [np.arange(i, len(ss), 7, dtype=np.int64) if i in (0, 3) else np.zeros(0, np.int64) for i in range(4)]
    want, want_rc, _ = d.call_consensus_files(ss, plain_paths, prm, want_counts=True, want_line_offsets=True, want_depth_sum=True, exclude=exclude)
    got, got_rc, _ = d.call_consensus_files(ss, mixed_paths, prm, want_counts=True, want_line_offsets=True, want_depth_sum=True, exclude=exclude, bgzf=True)
    assert list(want_rc) == [0, 0, 0, 0] == list(got_rc)
    for a, b in zip(want, got):
        _same_result(a, b)
    assert got[1].bgzf_info["has_eof_marker"] == 1 and got[1].bgzf_info["plain_bytes"] == len(samples[1][0]) and got[0].bgzf_info is None
    # a bad block in the middle of one of three BGZF files
    z = bytearray(_odd_bgzf(samples[1][0], 1))
    m = bc.members(bytes(z))
    off, size = m[len(m) // 2][0], m[len(m) // 2][1]
    z[off + size - 8] ^= 0x40                                       # a CRC byte
    (tmp_path / "bad.gz").write_bytes(bytes(z))
    (tmp_path / "s0.gz").write_bytes(bc.make_bgzf.compress(samples[0][0]))
    got, got_rc, _ = d.call_consensus_files(ss, [str(tmp_path / "s0.gz"), str(tmp_path / "bad.gz"), mixed_paths[3]], prm, want_counts=True,
                                            want_line_offsets=True, want_depth_sum=True, exclude=[exclude[0], exclude[1], exclude[3]], bgzf=True)
    assert list(got_rc) == [0, L.E_PILEUP, 0]
    _same_result(want[0], got[0])
    _same_result(want[3], got[2])
    assert got[1].bgzf_info["bad_block"] == len(m) // 2 and got[1].bgzf_info["bad_status"] == bc.ST_CRC and got[1].bgzf_info["n_bad"] == 1
    assert "CRC32 mismatch" in got[1].bgzf_error and "block %d " % (len(m) // 2) in got[1].bgzf_error
    with pytest.raises(devmod.PileupFormatError):
        d.raise_file_status(str(tmp_path / "bad.gz"), int(got_rc[1]), got[1])
    ss.close()


@pytest.mark.parametrize("name", sorted(bc.bad_blocks()))
def test_the_call_reports_a_file_with_a_bad_block(tmp_path, name):
    """Each kind of bad block, in the middle file of three: snpgpu_call_consensus_bgzf_files gives that file E_PILEUP with the block and
    the cause, and the other files of the call the results of the same text read as a plain file."""
    d = get_device()
    bad, want = bc.bad_blocks()[name]
    text = bc.pileup_text(12000, seed=15)
    text = text[:text.rindex(b"\n") + 1]
    keys = sorted({(ln.split(b"\t")[0], int(ln.split(b"\t")[1])) for ln in text.split(b"\n")[:-1]})[::3]
    ss = d.siteset(keys, [L.SITE_IN_SNPLIST] * len(keys))
    prm = devmod.make_params(0, 0.6, 1, 0, 0.0)
    half = text.index(b"\n", len(text) // 2) + 1
    (tmp_path / "a.txt").write_bytes(text)
    (tmp_path / "b.txt").write_bytes(text[half:])
    (tmp_path / "a.gz").write_bytes(bc.make_bgzf.compress(text, payload=1777))
    (tmp_path / "bad.gz").write_bytes(bc.bad_file(bad)[0])
    (tmp_path / "b.gz").write_bytes(bc.make_bgzf.compress(text[half:], payload=4099, eof=False))
    call = lambda names, **kw: d.call_consensus_files(ss, [str(tmp_path / n) for n in names], prm, want_counts=True, want_line_offsets=True, **kw)     # noqa: E731
    plain, plain_rc, _ = call(["a.txt", "b.txt"])
    got, got_rc, _ = call(["a.gz", "bad.gz", "b.gz"], bgzf=True)
    assert list(plain_rc) == [0, 0] and list(got_rc) == [0, L.E_PILEUP, 0]
    assert int(np.count_nonzero(plain[0].line_offsets)) == len(keys)
    _same_result(plain[0], got[0])
    _same_result(plain[1], got[2])
    info = got[1].bgzf_info
    assert (info["bad_block"], info["bad_status"], info["n_bad"], info["index_rc"]) == (1, want, 1, 0)
    assert "block 1 " in got[1].bgzf_error and not np.count_nonzero(got[1].line_offsets) and bytes(got[1].bases) == b"-" * len(keys)
    assert got[2].bgzf_info["has_eof_marker"] == 0
    ss.close()


# ---- the commands ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def _argv(monkeypatch):
    monkeypatch.setattr("sys.argv", ["cfsan_snp_pipeline", "test"])


def _run(line):
    from snp_pipeline_amd import cfsan_snp_pipeline as cli
    args = cli.parse_command_line(line)
    args.verbose = 0
    return cli.run_command_from_args(args)


def _tree(root, samples, compressed, pileup_name):
    """Sample directories with a pileup each (BGZF for the indices in `compressed`), a snplist, an exclude VCF per sample, a reference."""
    root.mkdir()
    dirs = []
    for i, (data, sites) in enumerate(samples):
        sdir = root / ("sample%d" % i)
        sdir.mkdir()
        (sdir / pileup_name).write_bytes(_odd_bgzf(data, i) if i in compressed else data)
        with open(str(sdir / "var.flt_removed.vcf"), "w") as f:
            f.write("##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS\n")
            for c, p in sites[i::5]:
                f.write("%s\t%d\t.\tA\tC\t.\tPASS\t.\tGT\t1/1\n" % (c.decode(), p))
        (sdir / "metrics").write_text('sample="sample%d"\n' % i)
        dirs.append(str(sdir))
    (root / "dirs.txt").write_text("\n".join(dirs) + "\n")
    with open(str(root / "snplist.txt"), "w") as f:
        for c, p in sorted({k for _, s in samples for k in s}):
            f.write("%s\t%d\t1\tsampleX\n" % (c.decode(), p))
    (root / "ref.fasta").write_text(">synth_chr1\n" + "A" * 48502 + "\n")
    return dirs


def _outputs(sdir):
    out = {}
    for name in ("consensus.fasta", "consensus.vcf", "metrics"):
        with open(os.path.join(sdir, name)) as f:
            out[name] = [ln for ln in f.read().split("\n") if not ln.startswith("##fileDate")]
    return out


def test_commands_on_bgzf_samples(tmp_path):
    """Four lambda-sized samples, two of them BGZF, an exclude file each: call_consensus_batch writes what it writes for the plain
    files; so does the per-sample command on a BGZF file."""
    samples = [_sample(60 + i) for i in range(4)]
    flags = "-f -l %s/snplist.txt -o consensus.fasta -e var.flt_removed.vcf --vcfFileName consensus.vcf --minConsDpth 3 --amdMetricsRefFasta %s/ref.fasta"
    plain = _tree(tmp_path / "plain", samples, (), "reads.all.pileup.gz")
    mixed = _tree(tmp_path / "mixed", samples, (1, 2), "reads.all.pileup.gz")          # (detection is by content: the plain ones carry the same name)
    for root in ("plain", "mixed"):
        assert _run("call_consensus_batch %s --pileupName reads.all.pileup.gz %s/dirs.txt" % (flags % (tmp_path / root, tmp_path / root), tmp_path / root)) == 0
    want = [_outputs(s) for s in plain]
    assert [_outputs(s) for s in mixed] == want
    assert all(len(w["consensus.vcf"]) > 50 and "avePileupDepth" in "".join(w["metrics"]) for w in want)
    # the per-sample command on one BGZF file
    one = "-f -l %s/snplist.txt -o %s/consensus.fasta -e %s/var.flt_removed.vcf --vcfFileName consensus.vcf --minConsDpth 3 --amdMetricsRefFasta %s/ref.fasta"
    for root, sdir in (("plain", plain[1]), ("mixed", mixed[1])):
        for name in ("consensus.fasta", "consensus.vcf"):
            os.unlink(os.path.join(sdir, name))
        with open(os.path.join(sdir, "metrics"), "w") as f:
            f.write('sample="sample1"\n')
        assert _run("call_consensus %s %s/reads.all.pileup.gz" % (one % (tmp_path / root, sdir, sdir, tmp_path / root), sdir)) == 0
    assert _outputs(mixed[1]) == _outputs(plain[1]) and len(_outputs(mixed[1])["consensus.vcf"]) > 50


def _error_of(tmp_path, monkeypatch, name, data, compressed, snplist, extra=""):
    """Exit code or exception, and the error log, of the per-sample command on one pileup."""
    root = tmp_path / name
    sdir = root / "sampleE"
    sdir.mkdir(parents=True)
    (sdir / "reads.all.pileup").write_bytes(bc.make_bgzf.compress(data, payload=777) if compressed else data)
    (root / "snplist.txt").write_text(snplist)
    log = root / "error.log"
    monkeypatch.setenv("errorOutputFile", str(log))
    try:
        rc = _run("call_consensus -f -l %s/snplist.txt -o %s/consensus.fasta --vcfFileName consensus.vcf%s %s/reads.all.pileup" % (root, sdir, extra, sdir))
        what = ("returned", rc)
    except SystemExit as e:
        what = ("exit", e.code)
    except Exception as e:                    # noqa: B902  (the class and the words are what is compared)
        what = (type(e).__name__, str(e))
    produced = sorted(n for n in os.listdir(str(sdir)) if n != "reads.all.pileup")
    return what, (log.read_text().replace(str(root), "ROOT") if log.exists() else ""), produced, sdir


def test_errors_of_a_bgzf_sample_are_those_of_the_plain_file(tmp_path, monkeypatch):
    lines = [b"c1\t5\tA\t3\tGGG\tIII", b"c1\t6\tC\t3\t...\tIII", b"c1\t5\tA\t4\tTTTt\tIIII", b"c1\t7\tG\t2\t..\tII", b"c1\t9\tG\t3\taaa\tIII", b"c1\t9\tG\t1\t.\tI"]
    repeated = b"\n".join(lines) + b"\n" + b"".join(b"c1\t%d\tA\t2\t..\tII\n" % p for p in range(20, 400))
    snplist = "c1\t5\t1\tx\nc1\t7\t1\tx\nc1\t9\t1\tx\nc1\t300\t1\tx\n"
    # a pileup that repeats listed positions: a row for every matching line
    a = _error_of(tmp_path, monkeypatch, "rep_plain", repeated, False, snplist)
    b = _error_of(tmp_path, monkeypatch, "rep_bgzf", repeated, True, snplist)
    assert a[:3] == b[:3] and a[0] == ("returned", 0)
    rows = lambda s: [ln for ln in (s / "consensus.vcf").read_text().split("\n") if not ln.startswith("##fileDate")]      # noqa: E731
    assert rows(a[3]) == rows(b[3]) and len([r for r in rows(a[3]) if r and not r.startswith("#")]) == 6
    assert (a[3] / "consensus.fasta").read_text() == (b[3] / "consensus.fasta").read_text()
    # ... one of whose repeated lines is malformed, and a malformed line at a listed position of a pileup without repeats
    for tag, exc, data in (("rep_bad", "ValueError", repeated.replace(b"c1\t5\tA\t4\tTTTt\tIIII", b"c1\t5\tA\tfour\tTTTt\tIIII")),
                           ("bad", "IndexError", repeated.replace(b"c1\t300\tA\t2\t..\tII", b"c1\t300\tA").replace(b"c1\t5\tA\t4\tTTTt\tIIII\n", b"").replace(b"c1\t9\tG\t1\t.\tI\n", b""))):
        a = _error_of(tmp_path, monkeypatch, tag + "_plain", data, False, snplist)
        b = _error_of(tmp_path, monkeypatch, tag + "_bgzf", data, True, snplist)
        assert a[:3] == b[:3], tag
        assert a[0][0] == exc, a[0]                  # (what the reference raises for the line: oracle.pileup_oracle on the same text)
    # --vcfAllPos with a BGZF pileup: a global error before any output is touched
    what, log, produced, _ = _error_of(tmp_path, monkeypatch, "allpos", repeated, True, snplist, extra=" --vcfAllPos")
    assert what == ("exit", 100) and "--vcfAllPos cannot be used with a BGZF-compressed pileup" in log and produced == []


def test_a_truncated_bgzf_sample_is_a_sample_error(tmp_path, monkeypatch):
    samples = [_sample(80 + i, genome_len=6000, n_sites=40) for i in range(3)]
    dirs = _tree(tmp_path / "t", samples, (0, 1, 2), "reads.all.pileup")
    whole = open(os.path.join(dirs[1], "reads.all.pileup"), "rb").read()
    with open(os.path.join(dirs[1], "reads.all.pileup"), "wb") as f:
        f.write(whole[:len(whole) * 2 // 3])
    log = tmp_path / "error.log"
    monkeypatch.setenv("errorOutputFile", str(log))
    monkeypatch.setenv("StopOnSampleError", "false")
    root = tmp_path / "t"
    assert _run("call_consensus_batch -f -l %s/snplist.txt -o consensus.fasta --vcfFileName consensus.vcf --minConsDpth 3 %s/dirs.txt" % (root, root)) == 0
    text = log.read_text()
    assert "call_consensus failed for sample sample1" in text and "truncated" in text and "sample0" not in text and "sample2" not in text
    assert not os.path.exists(os.path.join(dirs[1], "consensus.fasta"))
    plain = _tree(tmp_path / "p", samples, (), "reads.all.pileup")
    proot = tmp_path / "p"
    assert _run("call_consensus_batch -f -l %s/snplist.txt -o consensus.fasta --vcfFileName consensus.vcf --minConsDpth 3 %s/dirs.txt" % (proot, proot)) == 0
    for i in (0, 2):
        for name in ("consensus.fasta", "consensus.vcf"):
            a = [ln for ln in open(os.path.join(dirs[i], name)).read().split("\n") if not ln.startswith("##fileDate")]
            assert a == [ln for ln in open(os.path.join(plain[i], name)).read().split("\n") if not ln.startswith("##fileDate")]
    # --vcfAllPos in a batch with a BGZF sample: the global error, and nothing new in any sample directory
    shutil.rmtree(str(tmp_path / "p"))
    before = {d: sorted(os.listdir(d)) for d in dirs}
    with pytest.raises(SystemExit) as ei:
        _run("call_consensus_batch -f -l %s/snplist.txt -o consensus2.fasta --vcfFileName consensus2.vcf --vcfAllPos %s/dirs.txt" % (root, root))
    assert ei.value.code == 100 and {d: sorted(os.listdir(d)) for d in dirs} == before
