"""Generators of BGZF files for the tests of the BGZF reader: what zlib emits under each level / strategy / memLevel, streams
written bit by bit where zlib never emits the case (a 15-bit code, repeat codes that run from the literal/length lengths into
the distance lengths, a single-code distance tree, matches at distance 32 768), and malformed blocks.

The expected text of a well-formed file is never taken from the code under test: ``zlib_plain`` walks the gzip members with
struct and inflates each with Python's zlib.  Everything is seeded."""
import gzip
import importlib.util
import os
import random
import struct
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_bgzf", os.path.join(ROOT, "tools", "make_bgzf.py"))
make_bgzf = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(make_bgzf)

EOF_MARKER = make_bgzf.EOF_MARKER

# statuses of include/snpgpu.h
(ST_OK, ST_BTYPE, ST_STORED_LEN, ST_CODE_SET, ST_SYMBOL, ST_DISTANCE, ST_INPUT_END, ST_OUTPUT_OVER, ST_OUTPUT_SHORT, ST_CRC) = range(10)
E_NOT_GZIP, E_NOT_BGZF, E_TRUNCATED, E_ISIZE, E_MAGIC = -101, -102, -103, -104, -105


def members(data):
    """[(offset, size, deflate bytes, crc, isize)] of a well-formed BGZF file, by struct alone."""
    out, off = [], 0
    while off < len(data):
        assert data[off:off + 4] == b"\x1f\x8b\x08\x04", off
        xlen = struct.unpack_from("<H", data, off + 10)[0]
        extra, bsize, o = data[off + 12:off + 12 + xlen], None, 0
        while o + 4 <= len(extra):
            slen = struct.unpack_from("<H", extra, o + 2)[0]
            if extra[o:o + 2] == b"BC" and slen == 2:
                bsize = struct.unpack_from("<H", extra, o + 4)[0]
            o += 4 + slen
        size = bsize + 1
        crc, isize = struct.unpack_from("<II", data, off + size - 8)
        out.append((off, size, data[off + 12 + xlen:off + size - 8], crc, isize))
        off += size
    return out


def zlib_plain(data):
    """The text of a well-formed BGZF file according to Python's zlib (CRC and ISIZE checked as gzip does)."""
    parts = []
    for _, _, deflate, crc, isize in members(data):
        d = zlib.decompressobj(-15)
        text = d.decompress(deflate) + d.flush()
        assert d.eof and len(text) == isize and zlib.crc32(text) == crc
        parts.append(text)
    return b"".join(parts)


def pileup_text(n_bytes, seed=11):
    """Pileup-shaped text: the synthetic sample of the first run of tests/golden/pileup_vectors.json.gz, repeated with other seeds
    until there is enough of it."""
    from oracle import fuzz
    with gzip.open(os.path.join(ROOT, "tests", "golden", "pileup_vectors.json.gz"), "rb") as f:
        import json
        run = json.loads(f.read().decode())["runs"][0]
    parts, have, k = [], 0, 0
    while have < n_bytes:
        data, _, _ = fuzz.synth_pileup(run["seed"] + 1000 * k + (seed - 11), **run["kw"])
        parts.append(data)
        have += len(data)
        k += 1
    return b"".join(parts)[:n_bytes]


# ---- a bit writer and just enough of an encoder to place every token by hand ---------------------------------------------
class BitWriter(object):
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, value, n):
        """n bits of value, least significant first (header fields, extra bits)."""
        self.acc |= (value & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, n):
        """A Huffman code of n bits, most significant first."""
        for i in range(n - 1, -1, -1):
            self.bits((code >> i) & 1, 1)

    def done(self, pad=0):
        while self.n:
            self.bits(pad, 1)
        return bytes(self.out)


def canonical(lens):
    """{symbol: (code, length)} of the canonical code with these lengths (RFC 1951 3.2.2)."""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
_DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
FIXED_LIT = canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = canonical([5] * 32)


def put_tokens(bw, tokens, lit, dist, end=True):
    """tokens: an int is a literal, a pair is (length, distance)."""
    for t in tokens:
        if isinstance(t, int):
            bw.code(*lit[t])
            continue
        length, distance = t
        k = 28 if length == 258 else max(i for i in range(28) if _LBASE[i] <= length)
        bw.code(*lit[257 + k])
        bw.bits(length - _LBASE[k], _LEXT[k])
        d = max(i for i in range(30) if _DBASE[i] <= distance)
        bw.code(*dist[d])
        bw.bits(distance - _DBASE[d], _DEXT[d])
    if end:
        bw.code(*lit[256])


def fixed_stream(tokens, final=True, end=True, pad=0):
    bw = BitWriter()
    bw.bits(1 if final else 0, 1)
    bw.bits(1, 2)
    put_tokens(bw, tokens, FIXED_LIT, FIXED_DIST, end)
    return bw.done(pad)


def _lengths_header(bw, lit_lens, dist_lens, cl_lens, ops):
    """HLIT / HDIST / HCLEN, the code length code and the sequence `ops` of (code length symbol, extra value) written with it."""
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    bw.bits(len(lit_lens) - 257, 5)
    bw.bits(len(dist_lens) - 1, 5)
    bw.bits(19 - 4, 4)
    for s in order:
        bw.bits(cl_lens[s], 3)
    cl = canonical(cl_lens)
    for sym, extra in ops:
        bw.code(*cl[sym])
        if sym == 16:
            bw.bits(extra - 3, 2)
        elif sym == 17:
            bw.bits(extra - 3, 3)
        elif sym == 18:
            bw.bits(extra - 11, 7)


def _apply_ops(ops):
    seq = []
    for sym, extra in ops:
        if sym < 16:
            seq.append(sym)
        elif sym == 16:
            seq.extend([seq[-1]] * extra)
        else:
            seq.extend([0] * extra)
    return seq


def hand_dynamic_deflate():
    """Two dynamic blocks written by hand.  The first has codes of 1 to 15 bits (end-of-block and the only length symbol take the
    two 15-bit codes), a code-18 run of 13 zeros that covers the last eleven literal/length lengths AND the first two distance
    lengths, and a distance tree of a single code.  In the second a code-16 repeat runs from the last literal/length length
    over all four distance lengths."""
    bw = BitWriter()
    # block 1
    lits = sorted(b"ACGTNacgtn.,$^")
    lit_lens = [0] * 269
    for i, c in enumerate(lits):
        lit_lens[c] = i + 1
    lit_lens[256] = lit_lens[257] = 15
    dist_lens = [0, 0, 1]
    ops, run = [], 0

    def zeros(n):
        while n >= 11:
            k = min(n, 138)
            ops.append((18, k))
            n -= k
        if n >= 3:
            ops.append((17, n))
            n = 0
        ops.extend([(0, 0)] * n)
    for s in range(258):
        if lit_lens[s] == 0:
            run += 1
            continue
        zeros(run)
        run = 0
        ops.append((lit_lens[s], 0))
    assert run == 0
    ops.append((18, 13))                      # literal/length 258 .. 268 and distance 0, 1
    ops.append((1, 0))                        # distance 2
    assert _apply_ops(ops) == lit_lens + dist_lens
    used = sorted({s for s, _ in ops})        # 0?, 1 .. 15, 17?, 18
    cl_lens = [0] * 19
    for i, s in enumerate(used):
        cl_lens[s] = 4 if i < 32 - len(used) else 5       # a complete code: x codes of 4 bits and y of 5 with x + y = n, 2x + y = 32
    assert sum(2.0 ** -l for l in cl_lens if l) == 1.0
    bw.bits(0, 1)
    bw.bits(2, 2)
    _lengths_header(bw, lit_lens, dist_lens, cl_lens, ops)
    put_tokens(bw, list(lits) + [(3, 3)], canonical(lit_lens), canonical(dist_lens))
    # block 2
    lit_lens = [0] * 259
    lit_lens[65] = lit_lens[256] = lit_lens[257] = lit_lens[258] = 2
    dist_lens = [2, 2, 2, 2]
    ops = [(18, 65), (2, 0), (18, 138), (18, 52), (2, 0), (2, 0), (16, 5)]
    assert _apply_ops(ops) == lit_lens + dist_lens
    cl_lens = [0] * 19
    cl_lens[2], cl_lens[16], cl_lens[18] = 1, 2, 2
    bw.bits(1, 1)
    bw.bits(2, 2)
    _lengths_header(bw, lit_lens, dist_lens, cl_lens, ops)
    put_tokens(bw, [65, 65, 65, 65, (4, 2)], canonical(lit_lens), canonical(dist_lens))
    return bw.done()


def block_of_deflate(deflate):
    """A block around a hand-made deflate stream; its text, CRC and ISIZE are what zlib makes of the stream."""
    d = zlib.decompressobj(-15)
    text = d.decompress(deflate) + d.flush()
    assert d.eof
    return make_bgzf.member(deflate, zlib.crc32(text), len(text))


def far_match_blocks():
    """(length 3 at distance 32 768; length 258 at distance 32 768 ending on the last byte of a 65 536-byte block)."""
    rng = random.Random(5)
    first = [rng.randrange(144) for _ in range(32768)]          # (8-bit codes: the block stays below 64 KiB)
    a = fixed_stream(first + [(3, 32768), 1, 2, 3])
    b = fixed_stream(first + [7, 9] + [(258, 32768)] * 127)
    ba, bb = block_of_deflate(a), block_of_deflate(b)
    assert members(bb)[0][4] == 65536
    return ba, bb


# ---- well-formed files ------------------------------------------------------------------------------------------------------
def well_formed():
    """{name: file bytes}"""
    rng = random.Random(1)
    text = pileup_text(3 * 65280)
    one = text[:65280]
    cases = {}
    cases["stored_full"] = make_bgzf.compress(one, level=0)
    cases["stored_empty"] = make_bgzf.member(b"\x00\x00\x00\xff\xff" + b"\x01\x03\x00\xfc\xffabc", zlib.crc32(b"abc"), 3) + \
        make_bgzf.member(b"\x01\x00\x00\xff\xff", 0, 0) + EOF_MARKER
    cases["fixed"] = make_bgzf.compress(text, strategy=zlib.Z_FIXED)
    cases["dynamic"] = make_bgzf.compress(text, level=6)
    cases["memlevel1"] = make_bgzf.compress(one, level=6, mem_level=1)
    cases["huffman_only"] = make_bgzf.compress(one, strategy=zlib.Z_HUFFMAN_ONLY)
    runs = b"".join(bytes([65 + i % 4]) * n for i, n in enumerate([1, 2, 3, 4, 258, 259, 260, 600, 5, 1000]))
    cases["rle"] = make_bgzf.compress(runs + one[:20000] + b"G" * 700, strategy=zlib.Z_RLE)
    far3, far258 = far_match_blocks()
    cases["far_matches"] = far3 + far258 + EOF_MARKER
    cases["hand_dynamic"] = block_of_deflate(hand_dynamic_deflate()) + make_bgzf.block(text[:5000]) + EOF_MARKER
    cases["incompressible"] = make_bgzf.compress(bytes(rng.randrange(256) for _ in range(2 * 65280)), level=9)
    assert all(size > isize for _, size, _, _, isize in members(cases["incompressible"])[:-1])
    sizes, parts, at = [1, 63, 64, 65, 4095, 4096, 4097, 65280], [], 0
    for i in range(20):
        n = sizes[i % len(sizes)]
        parts.append(make_bgzf.block(text[at:at + n]))
        at += n
    cases["placement"] = b"".join(parts) + EOF_MARKER
    long_line = b"chrL\t7\tA\t600\t" + b".," * 300 + b"\t" + b"I" * 600 + b"\n"
    pre, post = text[:text.index(b"\n", 3000) + 1], text[4000:text.index(b"\n", 6000) + 1]
    post = post[post.index(b"\n") + 1:]
    cases["long_line"] = make_bgzf.block(pre + long_line[:100]) + make_bgzf.block(long_line[100:300]) + make_bgzf.block(long_line[300:] + post) + EOF_MARKER
    cases["no_eof"] = make_bgzf.compress(one[:30000], eof=False)
    cases["eof_in_the_middle"] = make_bgzf.block(one[:1000]) + EOF_MARKER + make_bgzf.block(one[1000:2500]) + EOF_MARKER
    cases["only_eof"] = EOF_MARKER
    cases["extra_subfield"] = make_bgzf.block(one[:777], extra_before=b"XY\x03\x00abc") + make_bgzf.block(one[777:999], extra_before=b"ZZ\x00\x00") + EOF_MARKER
    return cases


# ---- malformed blocks: one bad block between two good ones ------------------------------------------------------------------
def _with_footer(block, crc=None, isize=None):
    c, n = struct.unpack_from("<II", block, len(block) - 8)
    return block[:-8] + struct.pack("<II", c if crc is None else crc, n if isize is None else isize)


def bad_blocks():
    """{name: (bad block bytes, the status it must end with)}"""
    text = pileup_text(9000, seed=12)
    good = make_bgzf.block(text[:6000])
    crc, isize = struct.unpack_from("<II", good, len(good) - 8)
    cases = {}
    cases["crc_flip"] = (_with_footer(good, crc=crc ^ 0x00010000), ST_CRC)
    cases["isize_smaller"] = (_with_footer(good, isize=isize - 1), ST_OUTPUT_OVER)
    cases["isize_larger"] = (_with_footer(good, isize=isize + 1), ST_OUTPUT_SHORT)
    cases["distance_before_start"] = (make_bgzf.member(fixed_stream([97, (3, 5), 98]), 0, 5), ST_DISTANCE)
    bw = BitWriter()                          # a dynamic header whose code length code is over-subscribed: four codes of one bit
    bw.bits(1, 1)
    bw.bits(2, 2)
    bw.bits(0, 5)
    bw.bits(0, 5)
    bw.bits(0, 4)
    for _ in range(4):
        bw.bits(1, 3)
    bw.bits(0, 32)
    cases["oversubscribed"] = (make_bgzf.member(bw.done(), 0, 10), ST_CODE_SET)
    cases["reserved_btype"] = (make_bgzf.member(b"\x07" + b"\x00" * 9, 0, 4), ST_BTYPE)
    cases["len_nlen"] = (make_bgzf.member(b"\x01\x05\x00\x00\x00hello", zlib.crc32(b"hello"), 5), ST_STORED_LEN)
    # nine literals and no end-of-block code; the last byte is padded with ones, so no run of zero bits reads as the 7-bit end code
    cases["no_end_of_block"] = (make_bgzf.member(fixed_stream(list(b"ACGTACGTA"), end=False, pad=1), zlib.crc32(b"ACGTACGTA"), 9), ST_INPUT_END)
    return cases


def bad_file(bad):
    """(file bytes, [text of block 0, None, text of block 2, b""]): the bad block between two good ones, then the EOF marker."""
    text = pileup_text(9000, seed=13)
    a, b = text[:5000], text[5000:8123]
    return make_bgzf.block(a) + bad + make_bgzf.block(b) + EOF_MARKER, [a, None, b, b""]


# ---- files the index must refuse --------------------------------------------------------------------------------------------------
def index_cases():
    """{name: (file bytes, expected return code of the index, expected number of valid blocks before the bad one)}"""
    text = pileup_text(5000, seed=14)
    good = make_bgzf.block(text[:3000])
    last = make_bgzf.block(text[3000:])
    cases = {"empty": (b"", 0, 0), "plain_text": (text, E_NOT_GZIP, 0), "plain_gzip": (gzip.compress(text), E_NOT_BGZF, 0)}
    for cut in range(1, 18):                  # every byte position of the last block's header
        cases["cut_header_%02d" % cut] = (good + last[:cut], E_TRUNCATED, 1)
    cases["cut_middle"] = (good + last[:len(last) // 2], E_TRUNCATED, 1)
    cases["cut_footer"] = (good + last[:-3], E_TRUNCATED, 1)
    big = bytearray(last)
    struct.pack_into("<H", big, 16, len(last) + 50 - 1)
    cases["bsize_past_end"] = (good + bytes(big), E_TRUNCATED, 1)
    cases["isize_65537"] = (good + _with_footer(last, isize=65537) + EOF_MARKER, E_ISIZE, 1)
    cases["magic_mid_file"] = (good + b"\x1f\x8c" + last[2:] + EOF_MARKER, E_MAGIC, 1)
    cases["text_mid_file"] = (good + b"chr1\t5\tA\t3\t...\tIII\n", E_MAGIC, 1)
    return cases
