"""The host side of the BGZF reader — probe, block index, the serial inflater that shares its decode statements with the inflate
kernel, the plain bytes at an offset — against Python's zlib, without a GPU; and the same cases through a stand-alone program
built with AddressSanitizer and UndefinedBehaviorSanitizer (tools/probe/bgzf_host_check.hip), which is where an index out of
bounds in the shared decode code has to show before the same bytes are given to the kernel."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from snp_pipeline_amd import _lib as L
from snp_pipeline_amd import build as B
from tests import bgzf_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return L.load()


@pytest.fixture(scope="module")
def well_formed():
    files = bc.well_formed()
    return {name: (data, bc.zlib_plain(data)) for name, data in files.items()}


def _index(lib, data):
    a = np.frombuffer(data, dtype=np.uint8) if data else np.zeros(0, np.uint8)
    n, info = C.c_uint64(), L.BgzfInfo()
    rc = lib.snpgpu_bgzf_index(a.ctypes.data_as(C.c_void_p), len(a), None, 0, C.byref(n), C.byref(info))
    blocks = (L.BgzfBlock * max(int(n.value), 1))()
    rc2 = lib.snpgpu_bgzf_index(a.ctypes.data_as(C.c_void_p), len(a), blocks, n.value, C.byref(n), C.byref(info))
    assert rc2 == rc
    return rc, list(blocks)[:n.value], info


def _inflate_host(lib, data, blocks):
    a = np.frombuffer(data, dtype=np.uint8)
    out, sts = [], []
    for b in blocks:
        buf = C.create_string_buffer(max(b.isize, 1))
        sts.append(lib.snpgpu_bgzf_inflate_block_host(a.ctypes.data + b.coff, C.byref(b), buf))
        out.append(buf.raw[:b.isize])
    return out, sts


def test_index_and_host_inflater_match_zlib(lib, well_formed):
    for name, (data, plain) in well_formed.items():
        rc, blocks, info = _index(lib, data)
        want = bc.members(data)
        assert rc == 0 and len(blocks) == len(want), name
        assert [(b.coff, b.csize, b.crc, b.isize) for b in blocks] == [(m[0], m[1], m[3], m[4]) for m in want], name
        assert info.plain_bytes == len(plain) and info.compressed_bytes == len(data) and info.bad_block == 0xFFFFFFFFFFFFFFFF
        assert info.has_eof_marker == (0 if name == "no_eof" else 1), name
        texts, sts = _inflate_host(lib, data, blocks)
        assert set(sts) == {bc.ST_OK}, (name, sts)
        assert b"".join(texts) == plain, name
        poff = 0
        for b in blocks:
            assert b.poff == poff
            poff += b.isize


def test_the_cases_show_what_they_are_meant_to(well_formed):
    """The generators against zlib alone: the far matches sit where they should, the incompressible blocks are larger than their text."""
    far = bc.members(well_formed["far_matches"][0])
    assert far[0][4] == 32768 + 3 + 3 and far[1][4] == 65536
    plain = well_formed["far_matches"][1]
    assert plain[32768:32771] == plain[0:3]
    second = plain[far[0][4]:]
    assert second[-258:] == second[-258 - 32768:-32768] and len(second) == 65536
    # rle: zlib under Z_RLE matches at distance 1 only, up to 258 bytes at a time; the text holds runs one, two and many bytes longer than
    # that, and what zlib makes of the long runs is far too short to be literals, so matches of the full length into a run are in the stream
    import itertools
    import zlib
    runs = [len(list(g)) for _, g in itertools.groupby(well_formed["rle"][1][:2392])]
    assert runs == [1, 2, 3, 4, 258, 259, 260, 600, 5, 1000]
    for n in (259, 260, 600, 1000):
        assert len(bc.make_bgzf.raw_deflate(b"A" * n, 6, zlib.Z_RLE)) < 16
    assert len(bc.make_bgzf.raw_deflate(well_formed["rle"][1][:2392], 6, zlib.Z_RLE)) < 64
    hand = bc.zlib_plain(well_formed["hand_dynamic"][0][:bc.members(well_formed["hand_dynamic"][0])[0][1]] + bc.EOF_MARKER)
    assert hand == bytes(sorted(b"ACGTNacgtn.,$^")) + b"gnt" + b"AAAAAAAA"


def test_bad_blocks_end_with_their_status_on_the_host(lib):
    for name, (bad, want) in bc.bad_blocks().items():
        data, texts = bc.bad_file(bad)
        rc, blocks, _ = _index(lib, data)
        assert rc == 0 and len(blocks) == 4, name
        got, sts = _inflate_host(lib, data, blocks)
        assert sts == [bc.ST_OK, want, bc.ST_OK, bc.ST_OK], (name, sts)
        assert got[0] == texts[0] and got[2] == texts[2]


def test_index_refuses_what_is_not_bgzf(lib, tmp_path):
    for name, (data, want_rc, want_valid) in bc.index_cases().items():
        rc, blocks, info = _index(lib, data)
        assert (rc, len(blocks)) == (want_rc, want_valid), name
        assert info.index_rc == want_rc
        if want_rc:
            assert info.bad_block == want_valid and info.bad_offset == sum(b.csize for b in blocks), name
    assert b"recompress with bgzip" in lib.snpgpu_bgzf_strerror(bc.E_NOT_BGZF)
    assert len({lib.snpgpu_bgzf_strerror(c) for c in (bc.E_NOT_GZIP, bc.E_NOT_BGZF, bc.E_TRUNCATED, bc.E_ISIZE, bc.E_MAGIC)}) == 5


def test_probe_is_by_content(lib, tmp_path, well_formed):
    cases = bc.index_cases()
    want = {"empty": 0, "plain_text": 0, "plain_gzip": bc.E_NOT_BGZF, "cut_middle": 1, "isize_65537": 1, "cut_header_05": 1}
    for name, expected in want.items():
        p = tmp_path / (name + ".pileup")            # (the name says nothing)
        p.write_bytes(cases[name][0])
        assert lib.snpgpu_bgzf_probe(os.fsencode(str(p))) == expected, name
    p = tmp_path / "reads.txt"
    p.write_bytes(well_formed["extra_subfield"][0])
    assert lib.snpgpu_bgzf_probe(os.fsencode(str(p))) == 1
    p.write_bytes(well_formed["dynamic"][0][:7])      # the first header itself is cut
    assert lib.snpgpu_bgzf_probe(os.fsencode(str(p))) == bc.E_TRUNCATED
    assert lib.snpgpu_bgzf_probe(os.fsencode(str(tmp_path / "absent"))) == L.E_IO


def test_read_range(tmp_path, well_formed):
    from snp_pipeline_amd import pileup_text
    data, plain = well_formed["placement"]
    p = tmp_path / "placement.gz"
    p.write_bytes(data)
    blocks = bc.members(data)
    edges = np.cumsum([m[4] for m in blocks])
    for e in [int(x) for x in edges[:-1]]:
        assert pileup_text.read_range(str(p), e - 3, 7) == plain[e - 3:e + 4]              # across a block boundary
    assert pileup_text.read_range(str(p), len(plain) - 1, 1) == plain[-1:]                 # the last byte
    assert pileup_text.read_range(str(p), len(plain) - 1, 100) == plain[-1:]
    assert pileup_text.read_range(str(p), len(plain), 10) == b""
    assert pileup_text.read_range(str(p), 60000, 80000) == plain[60000:140000]             # over several blocks
    assert pileup_text.plain_size(str(p)) == len(plain) and pileup_text.read_all(str(p)) == plain
    with pileup_text.TextAt(str(p)) as t:
        at = plain.index(b"\n", 70000) + 1
        assert t.line(at) == plain[at:plain.index(b"\n", at)] and t.slice(at, 50) == plain[at:at + 50]
    q = tmp_path / "plain"
    q.write_bytes(plain)
    with pileup_text.TextAt(str(q)) as t:
        assert t.line(at) == plain[at:plain.index(b"\n", at)] and not t.compressed
    bad, _ = bc.bad_file(bc.bad_blocks()["crc_flip"][0])
    p.write_bytes(bad)
    assert pileup_text.read_range(str(p), 0, 100) == bc.zlib_plain(bad[:bc.members(bad)[0][1]])[:100]
    with pytest.raises(ValueError):
        pileup_text.read_range(str(p), 4990, 100)                                          # runs into the bad block


def test_host_decoder_under_sanitizers(tmp_path, well_formed):
    """Every well-formed and malformed case through the index, the host inflater and read_range in a stand-alone program whose
    host code is built with -fsanitize=address,undefined: buffers of exactly the files' and the texts' sizes, so that one byte
    read or written outside them ends the program with a report."""
    d = tmp_path / "cases"
    d.mkdir()
    lines = []
    for name, (data, plain) in well_formed.items():
        (d / (name + ".bgzf")).write_bytes(data)
        (d / (name + ".txt")).write_bytes(plain)
        lines.append("%s.bgzf 0 %d %s.txt %s" % (name, len(bc.members(data)), name, ",".join(["0"] * len(bc.members(data)))))
    for name, (bad, want) in bc.bad_blocks().items():
        data, texts = bc.bad_file(bad)
        (d / (name + ".bgzf")).write_bytes(data)
        # the plain file of a bad case: the good blocks' text at their plain offsets, the bad block's range as a gap
        isizes = [m[4] for m in bc.members(data)]
        (d / (name + ".txt")).write_bytes(texts[0] + b"\0" * isizes[1] + texts[2])
        lines.append("%s.bgzf 0 4 %s.txt 0,%d,0,0" % (name, name, want))
    for name, (data, want_rc, want_valid) in bc.index_cases().items():
        (d / (name + ".bgzf")).write_bytes(data)
        lines.append("%s.bgzf %d %d - -" % (name, want_rc, want_valid))
    (d / "manifest.txt").write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "bgzf_host_check")
    cmd = [B._hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-fno-gpu-sanitize", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tools", "probe", "bgzf_host_check.hip"),
           os.path.join(B.CSRC, "bgzf_host.hip"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(d)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-6000:]
    assert "%d cases, 0 failures" % len(lines) in r.stdout
    sys.stdout.write(r.stdout[-200:])
