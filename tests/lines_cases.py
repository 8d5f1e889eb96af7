"""Plain statements of the two things every all-lines and consensus kernel depends on — where the lines of a pileup start
(k_lines_index) and which site of the set a line's (name, position) is (the four look-ups of csrc/scan.hip) — in NumPy and plain
Python, and builders for pileups whose line terminators land on exact byte offsets.  No device and no library code is used here;
tests/test_lines_cpu.py pins these statements against bytes.splitlines, CPython's universal-newlines reader and the oracle."""
import random

import numpy as np

from oracle import pileup_oracle as po

LF, CRLF, CR = b"\n", b"\r\n", b"\r"


# ---- the statements -----------------------------------------------------------------------------------------------------------------
def line_starts(data):
    """Offsets (int64, ascending) of the lines of `data`: byte 0 starts a line when there is one; a line ends at '\\n', or at a '\\r'
    whose next byte is not '\\n' (the pair ends it then); a start at len(data) is no line.  Nothing else ends a line: not '\\v',
    '\\f', 0x1c-0x1e or 0x85."""
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    n = len(a)
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    nxt = np.empty(n, dtype=np.uint8)
    nxt[:-1] = a[1:]
    nxt[-1] = 0                                              # (no byte follows the last one: a '\r' there ends its line alone)
    ends = (a == 10) | ((a == 13) & (nxt != 10))             # the LAST byte of every terminator
    after = np.nonzero(ends)[0].astype(np.int64) + 1
    return np.concatenate([np.zeros(1, dtype=np.int64), after[after < n]])


def lines_of(data, starts):
    """The bytes of every line with its terminator, by the offsets of `starts`."""
    bounds = list(map(int, starts)) + [len(data)]
    return [bytes(data[bounds[i]:bounds[i + 1]]) for i in range(len(starts))]


def name_and_position(line, blank_ok=False):
    """(name, position) of a line as the oracle takes them: po.parse_record on line.split() gives .chrom and .position — int() of
    the second field, so 007, +7 and 1_0 are positions.  blank_ok: None for a line without fields (a blank line)."""
    fields = line.split()
    if blank_ok and not fields:
        return None
    rec = po.parse_record(fields[:4] if len(fields) >= 4 else fields, 0)
    return rec.chrom, rec.position


def line_flags(data, starts, keys, flags, blank_ok=False):
    """The flag byte (uint8) of every line: that of the key its (name, position) is, or 0."""
    by_key = {}
    for k, f in zip(keys, flags):
        by_key[k] = by_key.get(k, 0) | int(f)                # (a key given twice: the flags OR-ed, as the site set does)
    out = np.zeros(len(starts), dtype=np.uint8)
    for i, ln in enumerate(lines_of(data, starts)):
        key = name_and_position(ln, blank_ok)
        out[i] = by_key.get(key, 0) if key is not None else 0
    return out


def last_line_of(data, starts, keys):
    """({key: 1 + offset of the LAST line at that (name, position), or 0}, number of lines that are at some key): what
    Device.line_offsets(ss) and res.n_matched give after call_consensus."""
    last = {k: 0 for k in keys}
    hits = 0
    for s, ln in zip(starts, lines_of(data, starts)):
        key = name_and_position(ln)
        if key in last:
            last[key] = int(s) + 1
            hits += 1
    return last, hits


# ---- builders -----------------------------------------------------------------------------------------------------------------------
def min_width(name, pos):
    """Bytes of the shortest well-formed line of (name, pos): name pos ref 0 * * with five separators."""
    return len(name) + len(b"%d" % pos) + 9


def pileup_line(name, pos, width=None, sep=b"\t", ref=b"A", seed=0):
    """One well-formed pileup line without its terminator; with `width`, of exactly that many bytes: the length comes from the read
    count (two bytes a read), the last byte or two from leading zeros in the position column — int() takes 007, and so do the
    reference and parse_line_slow.  Depth 0 is the shortest line (name pos ref 0 * *)."""
    rng = random.Random(seed * 1000003 + pos)

    def body(depth, zeros):
        if depth == 0:
            bases, quals = b"*", b"*"
        else:
            bases = bytes(rng.choice(b".,.,.,GgTtc") for _ in range(depth))
            quals = bytes(33 + rng.randrange(20, 41) for _ in range(depth))
        return name + sep + b"0" * zeros + b"%d" % pos + b"\t" + ref + b"\t%d\t" % depth + bases + b"\t" + quals

    if width is None:
        return body(rng.randrange(0, 9), 0)
    base = len(body(0, 0))
    if width < base:
        raise ValueError("a line of %r %d has at least %d bytes, %d asked" % (name, pos, base, width))
    depth = max(0, (width - base) // 2 + 1)
    while depth > 0 and len(body(depth, 0)) > width:          # (the digits of the depth count too)
        depth -= 1
    ln = body(depth, width - len(body(depth, 0)))
    assert len(ln) == width
    return ln


def build_pileup(specs, targets=None, sep=b"\t", seed=0):
    """specs: [(name, position, terminator)]; targets: {index into specs: byte offset at which that line's terminator starts}.
    Lines without a target get a short length of their own.  Returns (data, starts): the text and the offset of every line of
    specs.  Asserts that every terminator is where the case asked, so that a case cannot silently miss its edge."""
    targets = targets or {}
    out, starts, at = [], [], 0
    for i, (name, pos, term) in enumerate(specs):
        starts.append(at)
        ln = pileup_line(name, pos, targets[i] - at if i in targets else None, sep=sep, seed=seed)
        out.append(ln + term)
        at += len(ln) + len(term)
    data = b"".join(out)
    for i, (name, pos, term) in enumerate(specs):
        end = starts[i + 1] if i + 1 < len(specs) else len(data)
        assert data[end - len(term):end] == term, i
        if i in targets:
            assert end - len(term) == targets[i] and data[targets[i]:targets[i] + len(term)] == term, (i, targets[i])
        body = data[starts[i]:end - len(term)]
        assert body and not (set(body) & {10, 13}), i         # no terminator byte inside a line
    return data, np.asarray(starts, dtype=np.int64)


def plan_terminators(placements, name=b"ctg", first_pos=1, filler=(20, 90), end=None, last_term=LF, seed=0):
    """specs and targets for build_pileup such that, for every (offset, terminator) of `placements` (ascending), a line's terminator
    starts exactly at that offset; filler lines ending in '\\n' (lengths drawn from `filler`) fill the space between.  end: the size
    of the file — the last line's terminator `last_term` (b"" for an unterminated line) ends exactly there."""
    rng = random.Random(seed)
    placements = list(placements)
    if end is not None:
        placements.append((end - len(last_term), last_term))
    specs, targets, at, pos = [], {}, 0, first_pos
    for off, term in placements:
        need = min_width(name, 10 * pos + 1000) + 1           # (a line and its '\n', with room for the positions to grow)
        while off - at > filler[1] + 2 * need:               # room for a filler line and still a whole line behind it
            w = rng.randrange(max(filler[0], need), filler[1] + 1)
            specs.append((name, pos, LF))
            targets[len(specs) - 1] = at + w
            at += w + 1
            pos += 1
        if off - at > filler[1] + need:                       # two lines left: split the space
            w = (off - at) // 2
            specs.append((name, pos, LF))
            targets[len(specs) - 1] = at + w
            at += w + 1
            pos += 1
        specs.append((name, pos, term))
        targets[len(specs) - 1] = off
        at = off + len(term)
        pos += 1
    return specs, targets


def random_text(rng, n_tokens):
    """A string over the bytes that are or look like line ends ('\\n' '\\r' '\\r\\n' '\\v' '\\f' 0x1c 0x1d 0x1e 0x85), TAB, blank and
    letters."""
    tokens = [b"\n", b"\r", b"\r\n", b"\v", b"\f", b"\x1c", b"\x1d", b"\x1e", b"\x85", b"\t", b" ", b"a", b"Zq", b"7"]
    return b"".join(rng.choice(tokens) for _ in range(n_tokens))
