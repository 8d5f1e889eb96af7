"""Cases for the line filter of the site-calling scan (phase B of k_varscan_scan, snp_pipeline_amd/csrc/varscan.hip), and a CPU
statement of that filter.

Three things live here, all plain Python:

  probes and a placer   probe() / tight() build pileup lines, Built.put() puts each at a chosen ALIGNED coordinate (the kernel's tiles
                        are counted from `lo` bytes below the file: lo = (address & 15) + 16) with filler lines of chosen length in
                        front and a control line behind; fillers and controls are plain and cannot call anything.
  dealing()             which wave of the launch reads which tiles: varscan_launch and the head of k_varscan_scan, restated.
  filter_model()        what phase B decides for one line - plain, calls, dropped or candidate - written from the kernel's comments
                        byte by byte: no ring, no SWAR, no modulo.  locate() / effective() add what depends on where the line lies.

The expected records of every test come from oracle/threshold_cases.varscan_records and oracle/varscan_oracle.py (expected()); the
model only proves that a case reaches the branch it is named for and that the filter, as designed, drops nothing the oracle calls."""
import os
import re
from collections import namedtuple

from oracle import threshold_cases as tc
from oracle import varscan_oracle as vo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what the Python statements below are written for; source_constants() reads the same from varscan.hip and the CPU suite compares
VS_TILE, VS_RING, VS_PAD, VS_CAND_LOCAL, WG_WAVES, SHARES, MAX_WAVES = 4096, 8192, 64, 136, 12, (140, 100, 66, 66), 256 * 64


def source_constants():
    src = open(os.path.join(ROOT, "snp_pipeline_amd", "csrc", "varscan.hip")).read()
    one = lambda pat: re.search(pat, src).groups()                                       # noqa: E731
    tile = int(one(r"#define VS_TILE (\d+)u")[0])
    a, b = one(r"VARSCAN_MAX_WAVES = (\d+) \* (\d+);")
    return dict(VS_TILE=tile, VS_RING=int(one(r"#define VS_RING \((\d+)u \* VS_TILE\)")[0]) * tile, VS_PAD=int(one(r"#define VS_PAD (\d+)u")[0]),
                VS_CAND_LOCAL=int(one(r"#define VS_CAND_LOCAL (\d+)u")[0]), WG_WAVES=int(one(r"uint32_t wg_waves = (\d+);")[0]),
                SHARES=tuple(int(x) for x in one(r"uint32_t share\[4\] = \{(\d+), (\d+), (\d+), (\d+)\};")), MAX_WAVES=int(a) * int(b),
                tiles="h_files[i].n_tiles = h_files[i].hi / VS_TILE + 1;" in src, want="if (want > total_tiles / 4) want = total_tiles / 4 ? total_tiles / 4 : 1;" in src,
                share_of="sh[(w >> 2) & 3u]" in src)


# ---- the launch's dealing -----------------------------------------------------------------------------------------------------
def lo_of(address):
    """varscan_file_coords: the aligned coordinates start 16..31 bytes below the file's first byte."""
    return (address & 15) + 16


def dealing(nbytes, lo, n_cu):
    """(n_tiles, [(t_first, t_end)] per wave) of a launch over ONE pileup of nbytes bytes whose first byte has aligned coordinate lo."""
    hi = lo + nbytes
    n_tiles = hi // VS_TILE + 1                                 # (the tile of position hi, the virtual terminator, included)
    want = min(n_cu * WG_WAVES, MAX_WAVES)
    if want > n_tiles // 4:
        want = n_tiles // 4 or 1
    weight = lambda w: SHARES[(w >> 2) & 3]                     # noqa: E731  wave w of a workgroup: the (w / 4)-th oldest of its SIMD
    blk = sum(weight(w) for w in range(WG_WAVES))
    cum = lambda x: (x // WG_WAVES) * blk + sum(weight(w) for w in range(x % WG_WAVES))   # noqa: E731
    span = cum(want)
    return n_tiles, [(n_tiles * cum(g) // span, n_tiles * cum(g + 1) // span) for g in range(want)]


Where = namedtuple("Where", "tile p0 wave index e carried long_")


def locate(off, e_off, lo, runs):
    """Where the scan meets the line whose first byte is file offset `off` and whose terminator (the LF of a CR LF pair) is file
    offset `e_off`: the tile that owns it is the tile of the terminator in FRONT of it; p0 and e count from that tile's start
    (p0 in 1..VS_TILE); carried: it ends in the next tile; long_: it does not end there either (the walk finds its end)."""
    x = off + lo
    k = (x - 1) // VS_TILE
    e = e_off + lo - k * VS_TILE
    wave = [g for g, (a, b) in enumerate(runs) if a <= k < b]
    assert len(wave) == 1, (off, k, runs)
    return Where(k, x - k * VS_TILE, wave[0], k - runs[wave[0]][0], e, e >= VS_TILE, e >= 2 * VS_TILE)


# ---- phase B's decision for one line --------------------------------------------------------------------------------------------
def is_letter(c):
    """The scan's "letter" class: bit 6 set, bits 3 and 7 clear ('@'..'G', 'P'..'W', '`'..'g', 'p'..'w': every ACGTacgt, no N)."""
    return c < 0x80 and (c & 0x48) == 0x40


Verdict = namedtuple("Verdict", "plain calls dropped window r head depth b0 t4 letters tabs")


def filter_model(line, min_coverage, min_reads2):
    """line: the bytes of one line without its terminator.  plain: four TABs where chrom / position / a one-byte reference / 1-4 depth
    digits (value >= 1) put them - looked for in the line's first 32 bytes, in its first 64 when those hold fewer than four and the
    line is longer than 32 -, at least one byte of read bases, a fifth TAB exactly depth + 1 bytes before the end, five TABs in all.
    calls: depth >= min_coverage and at least max(min_reads2, 1) letter-class bytes in the read-base column.  A plain line that does
    not call is dropped; every other non-empty line is a candidate and is walked.
    The window is chosen per line here.  The kernel takes the 64-bit window for a whole wave round as soon as one lane's line asks
    for it, so a line may be judged over 64 bytes where this statement looks at 32: `window` is the least the kernel looks at, and a
    line that is plain here is plain there (its first four TABs are the same in both), not always the other way round - which only
    sends more lines to the walk."""
    span = len(line)
    in32 = [i for i in range(min(span, 32)) if line[i] == 9]
    window = 32 if len(in32) >= 4 or span <= 32 else 64
    r = tuple(i for i in range(min(span, window)) if line[i] == 9)[:4]
    head, depth, b0, t4, letters, plain = False, 0, None, None, 0, False
    if len(r) == 4:
        digits = line[r[2] + 1:r[3]]
        head = r[0] > 0 and r[1] > r[0] + 1 and r[2] == r[1] + 2 and 1 <= len(digits) <= 4 and all(0x30 <= c <= 0x39 for c in digits) and int(digits) >= 1
    if head:
        depth = int(line[r[2] + 1:r[3]])
        b0 = r[3] + 1
        t4 = span - depth - 1
        if b0 + 1 + depth < span:                                                       # (b0 < t4: at least one byte of read bases)
            plain = line[t4] == 9 and line.count(b"\t") == 5
            letters = sum(1 for c in line[b0:t4] if is_letter(c))
    calls = depth >= min_coverage and letters >= max(min_reads2, 1)
    return Verdict(plain, calls, span > 0 and plain and not calls, window, r, head, depth, b0, t4, letters, line.count(b"\t"))


def effective(v, w):
    """What becomes of a line with verdict v at place w: "dropped", "plain" (a candidate whose columns the walk takes from the scan),
    "walk" (a candidate parsed in full) or "long" (end unknown).  A line that is handed to the next tile is vouched for where it
    starts when its four TABs lie in that tile; else the next tile looks again, which it can when the line starts in the 64 bytes
    in front of it."""
    if w.long_:
        return "long"
    shortcut = v.plain and (not w.carried or w.p0 + v.r[3] < VS_TILE or w.p0 + 63 >= VS_TILE)
    return "walk" if not shortcut else ("dropped" if v.dropped else "plain")


# ---- parameter sets -----------------------------------------------------------------------------------------------------------
def cov(depth):
    """min_coverage equal to a probe's depth; two variant reads pass at any depth of up to four digits."""
    return dict(min_coverage=depth, min_reads2=2, min_var_freq=0.0001)


D2 = dict(min_reads2=2, min_var_freq=0.2)                        # as the existing tests use (min_coverage 8)
R1 = dict(min_coverage=8, min_reads2=1, min_var_freq=0.0001)     # min_reads2 1 and 0: the filter still asks for one letter
R0 = dict(min_coverage=8, min_reads2=0, min_var_freq=0.0001)
V1 = dict(min_coverage=1, min_reads2=1, min_var_freq=0.0001)
DEPTH_OF_DIGITS = {1: 8, 2: 12, 3: 100, 4: 1000}


def pkey(kw):
    return tuple(sorted(kw.items()))


def options_text(kw):
    p = vo.Params(**kw)
    return "--min-coverage %d --min-reads2 %d --min-avg-qual %d --min-var-freq %r" % (p.min_coverage, p.min_reads2, p.min_avg_qual, p.min_var_freq)


# ---- lines ----------------------------------------------------------------------------------------------------------------------
LETTER_QUALS = b"@ABCDEFGPQRSTUVW"                               # Q31-38 and Q47-54: every quality is of the letter class
NAME_BYTES = b"CTGAcatgPQEF"                                     # ... and so is every byte of a name


def name_of(n, k=0):
    return bytes(NAME_BYTES[(k + i) % len(NAME_BYTES)] for i in range(n))


def probe(name, pos, ref, depth_text, bases, quals):
    """Raw bytes of a pileup line, no terminator (pos: int or bytes)."""
    return b"\t".join([name, pos if isinstance(pos, bytes) else b"%d" % pos, ref, depth_text, bases, quals])


def tight(name, pos, depth, variant, extra=0, k=0):
    """A probe with exactly as many letter-class bytes in its read bases as the filter asks for, `depth` reads and qualities:
    "ends": G at b0 and g at t4 - 1; "inner": at b0 + 1 and t4 - 2; "first" / "last": one letter (min_reads2 <= 1) at either end.
    The rest is '.', ',' and `extra` '$' (read ends: no read, no quality) spread over the middle."""
    n_let = 2 if variant in ("ends", "inner") else 1
    mid = [b".," [i % 2:i % 2 + 1] for i in range(depth - n_let - (2 if variant == "inner" else 0))]
    if mid:
        for i in range(extra):
            mid[(7 * i + k) % len(mid)] += b"$"
    elif extra:
        raise ValueError("no room for '$' in a probe of depth %d" % depth)
    body = b"".join(mid)
    bases = {"ends": b"G" + body + b"g", "inner": b".G" + body + b"g,", "first": b"G" + body, "last": body + b"g"}[variant]
    return probe(name, pos, b"A", b"%d" % depth, bases, bytes(LETTER_QUALS[(k + i) % 16] for i in range(depth)))


_FILLERS = {}


def filler(n, q=b"E"):
    """A plain line of exactly n >= 11 bytes that cannot call: no letter in its read bases."""
    if (n, q) not in _FILLERS:
        for dig in (1, 2, 3, 4):
            for x in range(4):
                d = n - 8 - dig - x
                if d >= 2 and d % 2 == 0 and len(str(d // 2)) == dig:
                    _FILLERS[(n, q)] = b"f\t5\tA\t%d\t" % (d // 2) + b"." * (d // 2) + b"$" * x + b"\t" + q * (d // 2)
                    break
            if (n, q) in _FILLERS:
                break
        else:
            raise ValueError("no filler of %d bytes" % n)
    return _FILLERS[(n, q)]


CONTROL = b"k\t3\tA\t8\t.,.,.,.,\tEEEEEEEE"                      # behind every probe: plain, cannot call

Probe = namedtuple("Probe", "off line e_off prm expect")         # expect: what the case is named for (checked by check_reach)


class Built(object):
    def __init__(self, name, lo, eol):
        self.name, self.lo, self.eol, self.chunks, self.size, self.probes, self.n_lines, self.fillers = name, lo, eol, [], 0, [], 0, set()
        self.data = None

    def _line(self, line):
        self.chunks.append(line + self.eol)
        self.size += len(line) + len(self.eol)
        self.n_lines += 1

    def fill_to(self, target, step=61):
        """Filler lines up to file offset `target`: lines of `step` bytes, the last of whatever length is missing."""
        gap = target - self.size
        if gap == 0:
            return
        t = len(self.eol)
        if gap < 11 + t:
            raise ValueError("%s: no room for a filler in %d bytes before offset %d" % (self.name, gap, target))
        while gap > step + t + 11 + t:
            self._line(filler(step))
            self.fillers.add(filler(step))
            gap -= step + t
        self._line(filler(gap - t))
        self.fillers.add(filler(gap - t))

    def put(self, line, prm=None, x=None, control=True, step=61, **expect):
        """line at aligned coordinate x (None: right here), then the control line."""
        if x is not None:
            self.fill_to(x - self.lo, step)
        off = self.size
        self._line(line)
        if prm is not None:
            self.probes.append(Probe(off, line, off + len(line) + len(self.eol) - 1, prm, expect))
        if control:
            self._line(CONTROL)
        return off

    def finish(self, nbytes=None):
        if nbytes is not None:
            self.fill_to(nbytes)
        self.data = b"".join(self.chunks)
        assert len(self.data) == self.size
        return self

    def params(self):
        out = {pkey(D2): D2}
        for p in self.probes:
            out[pkey(p.prm)] = p.prm
        return [out[k] for k in sorted(out)]


# ---- the expected result ------------------------------------------------------------------------------------------------------
_VALID = {}


def _valid(line):
    if line not in _VALID:
        try:
            vo.mpileup2snp(line, vo.Params(min_coverage=10 ** 9))
            _VALID[line] = True
        except ValueError:
            _VALID[line] = False
    return _VALID[line]


def expected(data, kw, cache):
    """(records, lines) as threshold_cases.varscan_records states them, or ("error", offset of the first line varscan_oracle
    refuses).  Lines end as for Java's readLine() (LF, CR, CR LF: varscan_oracle.mpileup2snp); cache: per data, shared by its runs."""
    if "lines" not in cache:
        lines, at = [], 0
        for m in re.finditer(b"\r\n|\r|\n", data):
            lines.append((at, data[at:m.start()]))
            at = m.end()
        if at < len(data):
            lines.append((at, data[at:]))
        cache["lines"] = lines
        cache["bad"] = next((off for off, ln in lines if ln and not _valid(ln)), None)
        cache["lf"] = b"\n".join(ln for _, ln in lines) + b"\n"
        cache["off"], at = {}, 0
        for off, ln in lines:
            cache["off"][at] = off
            at += len(ln) + 1
        cache["counts"] = {}
    if cache["bad"] is not None:
        return "error", cache["bad"]
    recs = tc.varscan_records(cache["lf"], vo.Params(**kw), cache["counts"])
    return sorted((cache["off"][r[0]],) + tuple(r[1:]) for r in recs), sum(1 for _, ln in cache["lines"] if ln)


def rec_tuples(recs):
    return sorted((int(r["line_off"]), int(r["sdp"]), int(r["dp"]), int(r["total"]), int(r["rdf"]), int(r["rdr"]), int(r["ref_qual_sum"]),
                   int(r["adf"]), int(r["adr"]), int(r["alt_qual_sum"]), int(r["ref_base"]), int(r["alt_base"])) for r in recs)


# ---- reach: a case is what its name says ----------------------------------------------------------------------------------------
def check_reach(b, p, n_cu=256):
    """Every key of p.expect, asserted with the model and the dealing statement; returns the line's fate (effective())."""
    n_tiles, runs = dealing(len(b.data), b.lo, n_cu)
    content = p.line
    v = filter_model(content, vo.Params(**p.prm).min_coverage, vo.Params(**p.prm).min_reads2)
    w = locate(p.off, p.e_off, b.lo, runs)
    x = p.off + b.lo
    fate = effective(v, w)
    ex = dict(p.expect)
    where = (b.name, p.off, ex)
    variant = ex.pop("variant", None)
    if ex.pop("tight", True):
        assert v.plain and v.calls and v.depth == vo.Params(**p.prm).min_coverage and v.letters == max(vo.Params(**p.prm).min_reads2, 1), (where, v)
        at = [i for i in range(v.b0, v.t4) if is_letter(content[i])]
        assert at == {"ends": [v.b0, v.t4 - 1], "inner": [v.b0 + 1, v.t4 - 2], "first": [v.b0], "last": [v.t4 - 1]}[variant], where
        assert all(is_letter(c) for c in content[v.t4 + 1:]) and all(is_letter(c) for c in content[:v.r[0]]) and is_letter(content[v.r[1] + 1]), where
    edge = (x + VS_TILE // 2) // VS_TILE                         # the tile edge nearest to the line's first byte: the one in front of tile `edge`
    kind = _edge_kinds(n_tiles, runs).get(edge)                  # (no edge in front of tile 0)
    checks = {"r3": lambda: v.r[3], "window": lambda: v.window, "b0m": lambda: (x + v.b0) % 32, "t4m": lambda: (x + v.t4) % 32,
              "tile_off": lambda: x % VS_TILE, "carried": lambda: w.carried, "long_": lambda: w.long_, "fate": lambda: fate,
              "first_of_run": lambda: kind == "first", "index_parity": lambda: {"in_odd": 1, "in_even": 0}[kind],
              "last_tile": lambda: kind == "last", "t4_tile_off": lambda: (x + v.t4) % VS_TILE,
              "e_tile_off": lambda: (p.e_off + b.lo) % VS_TILE, "cr_tile_off": lambda: (p.off + len(p.line) + b.lo) % VS_TILE,
              "b0_t4_words": lambda: (x + v.t4) // 32 - (x + v.b0) // 32, "b0_t4_tiles": lambda: (x + v.t4) // VS_TILE - (x + v.b0) // VS_TILE,
              "length": lambda: len(content), "plain": lambda: v.plain, "head": lambda: v.head, "stale_tile_index": lambda: w.index >= 1}
    for key, want in ex.items():
        got = checks[key]()
        assert got == want, (where, key, got, v, w)
    return fate


# ---- families -------------------------------------------------------------------------------------------------------------------
DEV_LO = lo_of(5)               # the GPU tests put a pileup 5 bytes behind an aligned device address
FILE_LO = lo_of(0)              # ... and a file lands on an aligned one
LF, CRLF, CR = b"\n", b"\r\n", b"\r"


def family_a(lo=DEV_LO):
    """Head geometry: name length 1..60 x position digits 1..10 x depth digits 1..4 (r3 = 7 .. 78), each probe tight under
    min_coverage = its depth; a file of short names with a long one now and then; tight probes of every length 11..64."""
    out, b, n = [], None, 0
    for dd in (1, 2, 3, 4):
        depth = DEPTH_OF_DIGITS[dd]
        for L in range(1, 61):
            for P in range(1, 11):
                if b is None or b.size > 120 * 1024:
                    b = Built("A%d" % len(out), lo, LF)
                    out.append(b)
                r3 = L + P + dd + 4
                n += 1
                variant = ("ends", "inner")[(L + P) % 2]
                b.put(tight(name_of(L, n), 10 ** (P - 1) + n % 9, depth, variant, extra=n % 3, k=n), cov(depth), variant=variant,
                      window=32 if r3 < 32 else 64, fate="plain" if r3 < 64 else "walk", tight=r3 < 64, **({"r3": r3} if r3 < 64 else {"plain": False}))
    m = Built("A_mixed", lo, LF)                                 # one long name per ~45 lines: its round takes the 64-bit window, every other lane's line is short
    for i in range(1800):
        L = 40 if i % 45 == 22 else 1 + i % 3
        variant = ("ends", "inner")[i % 2]
        m.put(tight(name_of(L, i), 1 + i, 8, variant, extra=i % 5, k=i), cov(8), control=i % 4 == 0, r3=L + len(str(1 + i)) + 5, variant=variant,
              window=64 if L == 40 else 32, fate="plain")
    s = Built("A_short", lo, LF)                                 # spans below 32 and below 64 (a line of under 11 bytes has no six columns)
    for rep in range(12):
        for length in range(11, 65):
            # length = name + position digits + 7 + 2 * depth + '$' (a one-digit depth)
            depth = 1 + (rep + length) % min(9, (length - 9) // 2)
            variant = ("first", "last")[rep % 2] if depth == 1 else ("ends", "first", "last", "inner")[(rep + length) % (4 if depth >= 4 else 3)]
            rest = length - 7 - 2 * depth
            extra = min(rest - 2, rep % 3) if depth >= 5 else 0
            L = 1 + (rest - extra - 2) * (rep % 5) // 4
            P = rest - extra - L
            if P > 10:
                L, P = L + P - 10, 10
            prm = cov(depth) if variant in ("ends", "inner") else dict(min_coverage=depth, min_reads2=rep % 2, min_var_freq=0.0001)
            s.put(tight(name_of(L, length), 10 ** (P - 1), depth, variant, extra=extra, k=rep), prm, length=length, variant=variant, fate="plain")
    return [x.finish(max(x.size, 40 * 1024)) for x in out + [m, s]]


SHORT, LONG, R63 = "short", "long", "r63"


def _shape(shape, k):
    """(line, parameter set, variant): a 34-byte probe, one of over 200 bytes, one whose fourth TAB is byte 63."""
    if shape == SHORT:
        return tight(name_of(1, k), 7, 12, "ends", k=k), cov(12), "ends"
    if shape == LONG:
        return tight(name_of(2, k), 77, 100, "inner", extra=k % 4, k=k), cov(100), "inner"
    return tight(name_of(50, k), 1234567, 12, "ends", k=k), cov(12), "ends"


def _edge_kinds(n_tiles, runs):
    """kind of the edge in front of tile e, e = 1 .. n_tiles - 1"""
    kinds = {}
    for e in range(1, n_tiles):
        g = [i for i, (a, z) in enumerate(runs) if a <= e < z][0]
        kinds[e] = "last" if e == n_tiles - 1 else "first" if e == runs[g][0] else ("in_odd" if (e - runs[g][0]) % 2 else "in_even")
    return kinds


def family_b(eol=LF, lo=DEV_LO, n_cu=256):
    """Where the line starts.  Cells (kind of tile edge, offset of the first byte from the edge, shape): every offset 0..127 of a
    tile; -70 .. +6 around an edge inside a wave's run at an odd and at an even tile index, around the first tile of a wave's run
    and around the last tile of the file; r3 = 63 at 4032, 4033, 4034, 4095 and 0; the line whose fourth TAB is the first byte of
    the next tile while the tile before had a TAB there.  One cell per edge; files of 33 tiles (8 waves), and for the edge in
    front of the last tile, of which a file has one, files of 11 tiles (2 waves)."""
    pending = {"any": [("any", d, (SHORT, LONG)[d % 2]) for d in range(7, 128)]}
    for kind in ("in_odd", "in_even", "first", "last"):
        pending[kind] = [(kind, d, LONG) for d in range(-70, 7)] + [(kind, d, SHORT) for d in range(-40, 7)]
    for kind in ("in_odd", "in_even"):
        pending[kind] += [(kind, d, R63) for d in (-64, -63, -62, -1, 0)]
    stale = ["in_odd", "in_even"]
    out = []
    while any(pending.values()):
        big = any(pending[k] for k in ("in_odd", "in_even", "first", "any"))
        n_tiles = 33 if big else 11
        nbytes = n_tiles * VS_TILE - lo - 100
        _, runs = dealing(nbytes, lo, n_cu)
        b = Built("B%d%s" % (len(out), {LF: "", CRLF: "_crlf", CR: "_cr"}[eol]), lo, eol)
        kinds = _edge_kinds(n_tiles, runs)
        reserved, blocked = {}, set()
        while big and stale:                                    # (the first file) tile e, with the tiles on either side of it left alone
            want = stale.pop()
            e = [e for e in sorted(kinds) if kinds[e] == want and 3 <= e < n_tiles - 2 and not {e - 1, e, e + 1} & (blocked | set(reserved))][0]
            reserved[e] = want
            blocked |= {e - 1, e + 1}
        for e, kind in sorted(kinds.items()):
            k = len(out) * 64 + e
            if e in reserved:
                # tile e - 1 starts with a TAB; the probe's depth "12" straddles the edge in front of tile e + 1, its fourth TAB is that
                # tile's second byte: seen from tile e the string of the other slot still says "TAB" for the byte in between
                b.put(filler(40), x=(e - 1) * VS_TILE - 1)
                line = probe(name_of(1, k), 1, b"A", b"12", b"G" * 12, b"E")
                b.put(line, V1, x=(e + 1) * VS_TILE - 7, tight=False, plain=False, head=True, carried=True, fate="walk", stale_tile_index=True,
                      tile_off=VS_TILE - 7)
                continue
            cells = pending[kind] or (pending["any"] if kind != "last" else [])
            if not cells or e in blocked:
                continue
            _, d, shape = cells.pop(0)
            x = e * VS_TILE + d
            expect = dict(tile_off=d % VS_TILE)
            if kind != "any":
                expect.update(last_tile=kind == "last", first_of_run=kind == "first")
                if kind.startswith("in_"):
                    expect["index_parity"] = 1 if kind == "in_odd" else 0
            line, prm, variant = _shape(shape, k)
            carried = d <= 0 and d + len(line) + len(eol) - 1 >= 0
            if shape == R63:
                expect.update(r3=63, window=64, fate="plain")
            b.put(line, prm, x=x, variant=variant, carried=carried, **expect)
        out.append(b.finish(nbytes))
    return out


def family_c(eol=LF, lo=DEV_LO, n_cu=256):
    """The ends of the letter interval [b0, t4): b0 % 32 and t4 % 32 each at 0, 1, 30, 31; both in one string word, in neighbouring
    words, in different tiles (= different ring slots, from either slot); the fifth TAB on the last byte of a tile and on the
    first of the next; the terminator (and, for CR LF, the CR) on the last byte of a tile; read bases of one byte; an empty
    base column (not plain)."""
    n_tiles = 33
    nbytes = n_tiles * VS_TILE - lo - 100
    _, runs = dealing(nbytes, lo, n_cu)
    b = Built("C%s" % {LF: "", CRLF: "_crlf", CR: "_cr"}[eol], lo, eol)
    at = [VS_TILE + 200]                                        # the next free aligned coordinate

    def put(line, prm, x, **expect):
        b.put(line, prm, x=x, **expect)
        at[0] = x + len(line) + 200

    k = 0
    for u in (0, 1, 30, 31):
        for v in (0, 1, 30, 31):
            for variant, depth in (("ends", 12), ("inner", 8), ("first", 8), ("last", 100)):
                k += 1
                extra = (v - u - depth) % 32
                line = tight(name_of(1 + k % 3, k), 5 + k, depth, variant, extra=extra, k=k)
                b0 = filter_model(line, 1, 1).b0
                x = at[0] + (u - (at[0] + b0)) % 32
                prm = cov(depth) if variant in ("ends", "inner") else dict(min_coverage=depth, min_reads2=k % 2, min_var_freq=0.0001)
                put(line, prm, x, variant=variant, b0m=u, t4m=v)
    # one word / neighbouring words
    line = tight(name_of(2), 9, 8, "ends", extra=3)
    put(line, cov(8), at[0] + (4 - (at[0] + filter_model(line, 1, 1).b0)) % 32, variant="ends", b0_t4_words=0)
    put(line, cov(8), at[0] + (27 - (at[0] + filter_model(line, 1, 1).b0)) % 32, variant="ends", b0_t4_words=1)
    # b0 and t4 in different tiles: out of slot 0 into slot 1 and back; the fifth TAB on either side of a tile edge; terminators on it
    kinds = _edge_kinds(n_tiles, runs)
    edges = [e for e in sorted(kinds) if kinds[e] in ("in_odd", "in_even") and e * VS_TILE > at[0] + 400]
    seen = set()
    for j, e in enumerate(edges[:12]):
        variant = ("ends", "inner")[j % 2]
        line = tight(name_of(3, j), 40 + j, 100, variant, extra=j, k=j)
        v = filter_model(line, 1, 1)
        # j % 3 == 0: the edge in the middle of the read bases; 1: the fifth TAB the last byte of the tile; 2: the first of the next
        x = e * VS_TILE - (v.b0 + 50 if j % 3 == 0 else v.t4 + 1 if j % 3 == 1 else v.t4)
        seen.add((j % 3, kinds[e]))
        put(line, cov(100), x, variant=variant, carried=True, index_parity=1 if kinds[e] == "in_odd" else 0,
            **({"b0_t4_tiles": 1} if j % 3 == 0 else {"t4_tile_off": VS_TILE - 1} if j % 3 == 1 else {"t4_tile_off": 0, "b0_t4_tiles": 1}))
    if len(seen) != 6:
        raise ValueError("family C: not every place of the interval at both tile parities: %r" % sorted(seen))
    if len(edges) < 16:
        raise ValueError("family C: too few tile edges")
    for j, e in enumerate(edges[12:16]):
        line, prm, variant = _shape((SHORT, LONG)[j % 2], j)
        if j < 2 or eol != CRLF:                                # the terminator the last byte of a tile
            put(line, prm, e * VS_TILE - len(line) - len(eol), variant=variant, e_tile_off=VS_TILE - 1, carried=False)
        else:                                                   # CR the last byte of a tile, its LF the first of the next
            put(line, prm, e * VS_TILE - len(line) - 1, variant=variant, cr_tile_off=VS_TILE - 1, e_tile_off=0, carried=True)
    # the `fits` edge
    put(probe(name_of(1), 3, b"A", b"1", b"G", b"E"), V1, at[0], variant="first", length=11)
    put(probe(name_of(1), 4, b"A", b"1", b"", b"E"), V1, at[0], tight=False, plain=False, head=True, fate="walk")
    put(probe(name_of(1), 5, b"A", b"3", b"", b"GGG"), V1, at[0], tight=False, plain=False, head=True, fate="walk")
    return [b.finish(nbytes)]


ODD_GOOD = [("quals one short", b"8", b"GGG...gg", b"EEEEEEE", b""), ("quals one long", b"8", b"GGG...gg", b"EEEEEEEEE", b""),
            ("a sixth TAB", b"8", b"GGG...gg", b"EEEEEEEE", b"\tGGGGGGGG"), ("further columns", b"8", b"GGG...gg", b"EEEEEEEE", b"\tx\t\ty"),
            ("depth 0", b"0", b"*", b"*", b""), ("depth 00012", b"00012", b"GGGggg......", b"EEEEEEEEEEEE", b""),
            ("depth 012", b"012", b"GGGggg......", b"EEEEEEEEEEEE", b""), ("depth 12345", b"12345", b"GGG...gg", b"EEEEEEEE", b"")]
ODD_BAD = [("depth +12", probe(b"C", 9, b"A", b"+12", b"GGGggg......", b"EEEEEEEEEEEE")), ("a two-byte reference", probe(b"C", 9, b"AC", b"8", b"GGG...gg", b"EEEEEEEE")),
           ("an empty name", probe(b"", 9, b"A", b"8", b"GGG...gg", b"EEEEEEEE"))]


def family_d(lo=DEV_LO):
    """Lines the shortcut must hand to the walk, each next to a tight probe: one file of those varscan_oracle accepts, and one
    file per line it refuses (the offset of the first refused line is the result)."""
    good = Built("D_good", lo, LF)
    for rep in range(160):                                      # (40 KiB: several waves)
        for i, (what, depth, bases, quals, more) in enumerate(ODD_GOOD):
            good.put(tight(name_of(1 + rep % 5, i), 100 + rep, 8, ("ends", "inner")[rep % 2], extra=rep % 7, k=rep), cov(8), control=False,
                     variant=("ends", "inner")[rep % 2], fate="plain")
            good.put(probe(name_of(2, rep), 200 + rep, b"A", depth, bases, quals) + more, D2, tight=False, plain=what == "depth 012", fate="plain" if what == "depth 012" else "walk")
    out = [good.finish()]
    for j, (what, line) in enumerate(ODD_BAD):
        b = Built("D_bad%d" % j, lo, LF)
        for rep in range(720):
            b.put(tight(name_of(1 + rep % 5, j), 100 + rep, 8, ("ends", "inner")[rep % 2], extra=rep % 7, k=rep), cov(8), variant=("ends", "inner")[rep % 2], fate="plain")
            if rep in (350, 500):
                b.put(line)
        out.append(b.finish())
    return out


def family_f(lo=DEV_LO, n_cu=256):
    """Long carried lines: tight probes of about 4 000 .. 8 200 bytes that start in one tile and end in the next; the terminator on
    the last byte of the second tile (carried) and on the first byte of the third (end unknown: the walk finds it)."""
    n_tiles = 33
    nbytes = n_tiles * VS_TILE - lo - 100
    b = Built("F", lo, LF)
    # (first tile of the probe, offset in it, depth, '$', the terminator's offset from the start of the owning tile or None)
    for j, (tile, off, depth, e) in enumerate([(2, 3000, 1990, None), (5, 100, 2040, None), (8, 2900, 2600, None), (11, 50, 3000, 2 * VS_TILE - 1),
                                               (15, 50, 3000, 2 * VS_TILE), (19, 2000, 3040, 2 * VS_TILE - 1), (23, 3000, 2500, 2 * VS_TILE), (27, 4090, 2000, None)]):
        variant = ("ends", "inner")[j % 2]
        x = tile * VS_TILE + off
        extra = 0 if e is None else tile * VS_TILE + e - x - len(tight(name_of(3, j), 50 + j, depth, variant))
        line = tight(name_of(3, j), 50 + j, depth, variant, extra=extra, k=j)
        expect = dict(carried=True, long_=e == 2 * VS_TILE, fate="long" if e == 2 * VS_TILE else "plain")
        if e is not None:
            expect["e_tile_off"] = e % VS_TILE
        b.put(line, cov(depth), x=x, variant=variant, **expect)
    return [b.finish(nbytes)]


def all_families():
    """{family: [Built]} for the LF families and family E (B and C with CR LF and lone CR ends)."""
    return {"A": family_a(), "B": family_b(), "C": family_c(), "D": family_d(), "E_crlf": family_b(CRLF) + family_c(CRLF),
            "E_cr": family_b(CR) + family_c(CR), "F": family_f()}


G_FILLER = b"CCC\t1\tA\t1\t.\tE\n"                                # 14 bytes, 5 TABs, 5 letters: plain, cannot call


def family_g_plan(n_cu, lo=DEV_LO):
    """The pileup of family G for a device of n_cu CUs: (filler line, bytes, tiles, runs, [(file offset, probe line)], how many probes
    straddle a wrap of the letter count / of the TAB count / of neither).  The file is G_FILLER over and over; a wave's share is at
    least 66 / cum(waves) of the tiles, 48 tiles of fillers hold 70 217 letters and as many TABs, so ceil(48 * cum(waves) / 66) tiles
    let every wave's run pass 65 536 of both before its end.  One probe (its length a multiple of the filler's) in every k-th wave's
    run, so that in front of it the run holds fillers only and the counts are arithmetic: letters before b0 = 65 534 or 65 535
    ([b0, t4) of an "ends" or "inner" probe straddles the wrap), TABs before the line 65 531 .. 65 535 ([p0, le) straddles it), or
    the probe far from either."""
    fl = G_FILLER
    assert filter_model(fl[:-1], 1, 0).dropped and len(fl) == 14 and fl.count(b"\t") == 5 and sum(1 for c in fl if is_letter(c)) == 5
    want = min(n_cu * WG_WAVES, MAX_WAVES)
    weight = lambda w: SHARES[(w >> 2) & 3]                     # noqa: E731
    cum = (want // WG_WAVES) * sum(weight(w) for w in range(WG_WAVES)) + sum(weight(w) for w in range(want % WG_WAVES))
    n_tiles = -(-48 * cum // min(SHARES))
    nbytes = (n_tiles * VS_TILE - lo - 1) // 14 * 14
    got_tiles, runs = dealing(nbytes, lo, n_cu)
    assert got_tiles == n_tiles and len(runs) == want and min(b - a for a, b in runs) >= 47, (got_tiles, n_tiles, len(runs))
    pl = [sum(1 for c in fl[:j] if is_letter(c)) for j in range(15)]
    pt = [fl[:j].count(b"\t") for j in range(15)]
    letters_before = lambda y: 5 * (y // 14) + pl[y % 14]        # noqa: E731  (in a file of fillers only)
    tabs_before = lambda y: 5 * (y // 14) + pt[y % 14]           # noqa: E731
    stride = max(1, want // 192)
    probes, kinds = [], {"letters": 0, "tabs": 0, "neither": 0}
    for j, g in enumerate(range(0, want, stride)):
        s = max(runs[g][0] * VS_TILE - lo, 0)                    # file offset of the run's first byte
        kind = ("letters", "tabs", "neither")[j % 3]
        variant = ("ends", "inner")[(j // 3) % 2]
        found = None
        for L in range(1, 7):
            line = tight(name_of(L, j), 3 + j % 5, 12, variant, k=j)
            line = tight(name_of(L, j), 3 + j % 5, 12, variant, extra=-(len(line) + 1) % 14, k=j)
            v = filter_model(line, 12, 2)
            head = sum(1 for c in line[:v.b0] if is_letter(c))  # the probe's own letters in front of b0: name and reference
            if kind == "letters":                               # the filler line the probe replaces: from the count wanted in front of it
                i = (65535 - head + letters_before(s)) // 5
            elif kind == "tabs":
                i = (65535 + tabs_before(s)) // 5
            else:
                i = s // 14 + 1 + 977 * (j % 11)
            o = 14 * i
            lb0 = letters_before(o) - letters_before(s) + head
            tp0 = tabs_before(o) - tabs_before(s)
            straddles = (lb0 < 65536 <= lb0 + 2, tp0 < 65536 <= tp0 + 5)
            if (kind == "neither" and not any(straddles)) or (kind == "letters" and straddles[0]) or (kind == "tabs" and straddles[1]):
                found = (o, line, straddles)
                break
        if not found:
            raise ValueError("family G: no %s probe for wave %d" % (kind, g))
        o, line, straddles = found
        w = locate(o, o + len(line), lo, runs)
        assert w.wave == g and not w.long_ and o >= s and o + len(line) + 1 <= nbytes and (len(line) + 1) % 14 == 0, (g, w)
        assert v.plain and v.calls and v.letters == 2 and v.depth == 12 and all(is_letter(c) for c in line[v.t4 + 1:])
        kinds["letters"] += straddles[0]
        kinds["tabs"] += straddles[1]
        kinds["neither"] += not any(straddles)
        probes.append((o, line))
    return fl, nbytes, n_tiles, runs, probes, kinds
