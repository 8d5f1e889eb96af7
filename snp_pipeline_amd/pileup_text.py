"""The text of a pileup file on the HOST, whether the file holds it plain or BGZF-compressed (``samtools mpileup | bgzip``).

The device reads either kind (csrc/bgzf.hip); the few places where the host looks at the text itself — a line at an offset for a
row of consensus.vcf, the whole text when a byte >= 0x80 has to be judged — go through this module, which for a BGZF file
inflates the one or two blocks that cover the bytes asked for with the host inflater.  ``TextAt`` indexes the file once for any
number of reads; ``read_range`` (snpgpu_bgzf_read_range) is the one-off form, which indexes the file on every call.
Detection is by content, never by name."""
import ctypes as C
import os

from . import _lib as L

# what the probe says of a gzip file that is no usable BGZF: the library reports such a file itself, per file
_BROKEN = (L.BGZF_E_NOT_BGZF, L.BGZF_E_TRUNCATED, L.BGZF_E_MAGIC)


def probe(path):
    """1: BGZF, 0: not gzip (plain text), negative: E_IO or a BGZF_E_* code (gzip that is no BGZF)."""
    return int(L.load().snpgpu_bgzf_probe(os.fsencode(path)))


def is_compressed(path):
    """True for a file the BGZF reader has to take (BGZF, or gzip that it will refuse in its own words)."""
    kind = probe(path)
    return kind == 1 or kind in _BROKEN


def strerror(code):
    return L.load().snpgpu_bgzf_strerror(int(code)).decode("ascii")


def status_name(status):
    return L.load().snpgpu_bgzf_status_name(int(status)).decode("ascii")


def read_range(path, offset, nbytes):
    """The plain bytes [offset, offset + nbytes) of a BGZF file (fewer at the end of the text)."""
    buf = C.create_string_buffer(max(int(nbytes), 1))
    got = C.c_uint64()
    rc = L.load().snpgpu_bgzf_read_range(os.fsencode(path), int(offset), int(nbytes), buf, C.byref(got))
    if rc == L.E_IO:
        raise IOError("cannot open or read the pileup file %s" % path)
    if rc != 0:
        raise ValueError("compressed pileup %s: %s" % (path, "a block cannot be inflated" if rc == L.E_PILEUP else strerror(rc)))
    return buf.raw[:int(got.value)]


class _Index(object):
    """A BGZF file mapped once, with its block table (snpgpu_bgzf_index, one pass over the headers) and the text of the block that
    was inflated last: what serves any number of reads at plain offsets."""

    def __init__(self, path):
        import mmap
        import numpy as np
        self.path = path
        self._f = open(path, "rb")
        self._mm = self._arr = None
        self.blocks, self.n_blocks, self.plain_bytes = (L.BgzfBlock * 0)(), 0, 0
        self._ends = np.zeros(0, np.uint64)
        self._cached, self._text = -1, b""
        if os.fstat(self._f.fileno()).st_size == 0:
            return
        self._mm = mmap.mmap(self._f.fileno(), 0, access=mmap.ACCESS_READ)
        self._arr = np.frombuffer(self._mm, dtype=np.uint8)
        lib, n, info = L.load(), C.c_uint64(), L.BgzfInfo()
        ptr = self._arr.ctypes.data_as(C.c_void_p)
        rc = lib.snpgpu_bgzf_index(ptr, len(self._arr), None, 0, C.byref(n), C.byref(info))
        if rc == 0:
            self.blocks = (L.BgzfBlock * max(int(n.value), 1))()
            rc = lib.snpgpu_bgzf_index(ptr, len(self._arr), self.blocks, n.value, C.byref(n), C.byref(info))
        del ptr                                   # (it keeps the array, and with it the mapping, alive)
        if rc != 0:
            self.close()
            raise ValueError("compressed pileup %s: %s" % (path, strerror(rc)))
        self.n_blocks, self.plain_bytes = int(n.value), int(info.plain_bytes)
        self._ends = np.fromiter((self.blocks[i].poff + self.blocks[i].isize for i in range(self.n_blocks)), dtype=np.uint64, count=self.n_blocks)

    def _block_text(self, i):
        if i != self._cached:
            b = self.blocks[i]
            buf = C.create_string_buffer(max(int(b.isize), 1))
            st = L.load().snpgpu_bgzf_inflate_block_host(self._arr.ctypes.data + b.coff, C.byref(b), buf)
            if st != 0:
                raise ValueError("compressed pileup %s: block %d at byte offset %d cannot be inflated: %s" % (self.path, i, b.coff, status_name(st)))
            self._cached, self._text = i, buf.raw[:b.isize]
        return self._text

    def read(self, offset, nbytes):
        import numpy as np
        out, offset, nbytes = [], int(offset), int(nbytes)
        i = int(np.searchsorted(self._ends, np.uint64(offset), side="right")) if len(self._ends) else 0      # the first block whose text ends behind the offset
        while nbytes > 0 and i < len(self._ends):
            text, b = self._block_text(i), self.blocks[i]
            piece = text[offset - b.poff:offset - b.poff + nbytes]
            out.append(piece)
            offset += len(piece)
            nbytes -= len(piece)
            i += 1
        return b"".join(out)

    def close(self):
        self._arr = None
        if self._mm is not None:
            self._mm.close()
            self._mm = None
        if self._f is not None:
            self._f.close()
            self._f = None


def plain_size(path):
    """Bytes of text in a BGZF file (from its block headers alone)."""
    ix = _Index(path)
    try:
        return ix.plain_bytes
    finally:
        ix.close()


def read_all(path):
    """The whole text of a pileup file of either kind."""
    if probe(path) == 1:
        ix = _Index(path)
        try:
            return ix.read(0, ix.plain_bytes)
        finally:
            ix.close()
    with open(path, "rb") as f:
        return f.read()


class TextAt(object):
    """Lines of a pileup of either kind by their offset in the plain text.  A BGZF file is indexed once, when it is opened."""

    def __init__(self, path):
        self.path = path
        self.compressed = probe(path) == 1
        self._f = self._mm = self._ix = None
        if self.compressed:
            self._ix = _Index(path)
        else:
            import mmap
            self._f = open(path, "rb")
            self._mm = mmap.mmap(self._f.fileno(), 0, access=mmap.ACCESS_READ)

    def slice(self, start, nbytes):
        if self.compressed:
            return self._ix.read(start, nbytes)
        return self._mm[start:start + nbytes]

    def line(self, start):
        """From `start` to the end of its line (the terminator excluded)."""
        if not self.compressed:
            end = self._mm.find(b"\n", start)
            return self._mm[start:end if end >= 0 else len(self._mm)]
        out, step = b"", 4096
        while True:
            piece = self._ix.read(start + len(out), step)
            at = piece.find(b"\n")
            if at >= 0:
                return out + piece[:at]
            out += piece
            if len(piece) < step:
                return out
            step *= 4

    def close(self):
        if self._ix is not None:
            self._ix.close()
            self._ix = None
        if self._mm is not None:
            self._mm.close()
            self._f.close()
            self._mm = self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
