#!/usr/bin/env python3
"""Plain text -> BGZF with Python's zlib, as `bgzip` lays it out: gzip members whose deflate stream is raw (wbits=-15), 65 280
bytes of text per block, the block size in the extra subfield BC, and the 28-byte empty block as the end-of-file marker.

    tools/make_bgzf.py reads.all.pileup reads.all.pileup.gz [--level 6] [--strategy default|filtered|huffman|rle|fixed]
                       [--memLevel 8] [--payload 65280] [--no-eof]

The options beyond --level exist for the tests: they make zlib emit the block types and tree shapes the inflate kernel has to
handle (stored blocks at level 0, fixed Huffman, Huffman-only, run-length matches, hundreds of deflate blocks at memLevel 1).
"""
import argparse
import struct
import sys
import zlib

PAYLOAD = 65280
STRATEGIES = {"default": zlib.Z_DEFAULT_STRATEGY, "filtered": zlib.Z_FILTERED, "huffman": zlib.Z_HUFFMAN_ONLY, "rle": zlib.Z_RLE,
              "fixed": zlib.Z_FIXED}
EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def member(deflate, crc, isize, extra_before=b""):
    """One BGZF block around a raw deflate stream.  extra_before: other subfields in front of BC (the format allows them)."""
    xlen = len(extra_before) + 6
    bsize = 12 + xlen + len(deflate) + 8 - 1
    if bsize > 0xFFFF:
        raise ValueError("block of %d bytes does not fit BSIZE" % (bsize + 1))
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff" + struct.pack("<H", xlen) + extra_before + b"BC" + struct.pack("<HH", 2, bsize)
            + deflate + struct.pack("<II", crc & 0xFFFFFFFF, isize))


def raw_deflate(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    return c.compress(text) + c.flush()


def block(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8, extra_before=b""):
    """The block of one piece of text (at most 65 536 bytes; whatever zlib makes of it has to fit 64 KiB)."""
    if len(text) > 65536:
        raise ValueError("at most 65536 bytes of text per block")
    return member(raw_deflate(text, level, strategy, mem_level), zlib.crc32(text), len(text), extra_before)


def compress(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8, payload=PAYLOAD, eof=True):
    out = [block(data[i:i + payload], level, strategy, mem_level) for i in range(0, len(data), payload)]
    if eof:
        out.append(EOF_MARKER)
    return b"".join(out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("plain")
    ap.add_argument("out")
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--strategy", choices=sorted(STRATEGIES), default="default")
    ap.add_argument("--memLevel", type=int, default=8)
    ap.add_argument("--payload", type=int, default=PAYLOAD)
    ap.add_argument("--no-eof", action="store_true")
    a = ap.parse_args(argv)
    if not 1 <= a.payload <= 65536:
        ap.error("--payload must be between 1 and 65536")
    n_in = n_out = 0
    with open(a.plain, "rb") as src, open(a.out, "wb") as dst:
        while True:
            piece = src.read(a.payload)
            if not piece:
                break
            b = block(piece, a.level, STRATEGIES[a.strategy], a.memLevel)
            dst.write(b)
            n_in += len(piece)
            n_out += len(b)
        if not a.no_eof:
            dst.write(EOF_MARKER)
            n_out += len(EOF_MARKER)
    print("%d -> %d bytes (ratio %.3f)" % (n_in, n_out, n_in / n_out if n_out else 0.0), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
