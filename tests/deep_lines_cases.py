"""Deterministic deep-coverage pileup lines (over 512 bytes, up to and past 2 KiB: past every window of the one-lane-per-site call
passes, and at the edges of windows twice and four times as wide) shared by tests/test_deep_lines_cpu.py (the
oracle alone takes every one) and tests/test_gpu_deep_lines.py (the device against the oracle).  Every builder returns
(file bytes, [(chrom, pos) of the lines under test])."""
import random
import re

from oracle import fuzz

CHROM = b"deep"
LENGTHS = (511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049)


def line(pos, ref, bases, quals, depth=None, chrom=CHROM):
    n = depth if depth is not None else max(1, len(quals))
    return b"%s\t%d\t%s\t%d\t%s\t%s" % (chrom, pos, ref, n, bases, quals)


def exact_line(pos, total, term, rng):
    """A well-formed line of exactly `total` bytes, terminator included: mixed-strand reads, a '$' when the parity asks for one."""
    over = len(line(pos, b"A", b"", b"", depth=1000)) + len(term)
    rem = total - over
    n = rem // 2
    bases = bytes(rng.choice(b".,ACGTacgt*") for _ in range(n)) + (b"$" if rem & 1 else b"")
    quals = bytes(rng.randint(33, 74) for _ in range(n))
    out = line(pos, b"A", bases, quals, depth=1000)
    assert len(out) + len(term) == total
    return out


def filler(pos, length, term):
    """A short unlisted line of exactly `length` bytes with its terminator (length >= 24)."""
    head = b"fill\t%d\tC\t1\t" % pos
    n = length - len(head) - len(term) - 1
    assert n >= 2, length
    return head + b"." * (n // 2) + b"$" * (n & 1) + b"\t" + b"I" * (n // 2)


def window_edges(term, reverse=False, seed=5):
    """Lines of every LENGTHS entry, each at four placements: wherever it falls, starting at byte 15 of a 16-byte block, starting 8
    bytes before a 4 KiB tile boundary of the scan's fetch, and starting right on one.  A line under test is first and last."""
    rng = random.Random(seed)
    lengths = list(reversed(LENGTHS)) if reverse else list(LENGTHS)
    out, keys, pos = b"", [], 0
    for place in range(4):
        for total in lengths:
            pos += 1
            if place and out:
                want = (15, 4096 - 8, 0)[place - 1]
                mod = 16 if place == 1 else 4096
                pad = (want - len(out)) % mod
                while pad < 24 + len(term):
                    pad += mod
                out += filler(pos, pad, term) + term
            out += exact_line(pos, total, term, rng) + term
            keys.append((CHROM, pos))
    return out, keys


def bases_field_edges():
    """255 .. 513 read bases: one symbol alone on one strand (a single count of 256 / 512 and more), forward, reverse, mixed, and
    '.' / ',' standing for the reference base."""
    out, keys, pos = [], [], 0
    for n in (255, 256, 257, 511, 512, 513):
        for bases in (b"G" * n, b"g" * n, b"Gg" * (n // 2) + b"G" * (n & 1), b"." * n, b"," * n, b".," * (n // 2) + b"T" * (n & 1),
                      b"G" * (n - 1) + b"c", b"*" * n):
            pos += 1
            out.append(line(pos, b"a", bases, b"I" * n))
            keys.append((CHROM, pos))
    return b"\n".join(out) + b"\n", keys


MARKERS = (b"^I", b"^^", b"$", b"+12ACGTACGTACGT", b"-3NNN", b"*")


def marker_edges():
    """Every marker ending at, beginning at and straddling bit 63/64 of every mask word (bases fields of up to 16 words), and at the
    end of the field; an indel whose declared length runs past the field and past the window."""
    out, keys, pos = [], [], 0
    for m in MARKERS:
        for w in range(1, 16):
            for start in (64 * w - len(m), 64 * w, 64 * w - max(1, len(m) // 2)):
                if start < 1:
                    continue
                pos += 1
                bases = b"Ac" * (start // 2) + b"A" * (start & 1) + m + b"gT" * 5
                n_reads = start + 10 + (1 if m == b"*" else 0)
                out.append(line(pos, b"T", bases, b"I" * n_reads))
                keys.append((CHROM, pos))
    for total_reads in (230, 480, 990):                          # ... at the last bytes of the field
        for m in MARKERS:
            pos += 1
            out.append(line(pos, b"T", b"aC" * (total_reads // 2) + m, b"I" * (total_reads + 1)))
            keys.append((CHROM, pos))
    for declared, follow in ((900, 100), (1200, 700), (2000, 300), (65536, 450), (70000, 900)):
        pos += 1
        out.append(line(pos, b"G", b"A" * 40 + b"+%d" % declared + b"ACGT" * (follow // 4) + b"ttt", b"I" * 500))
        keys.append((CHROM, pos))
    return b"\n".join(out) + b"\n", keys


def quality_edges():
    """-q 13: qualities 12 / 13 / 14 at positions 255-257 and 511-513 of the quality field, and quality fields that end there (the
    zip of bases and qualities truncates, pileup.py:248-250)."""
    out, keys, pos = [], [], 0
    for n in (600, 300):
        for at in (255, 256, 257, 511, 512, 513):
            for q in (12, 13, 14):
                if at >= n:
                    continue
                pos += 1
                quals = bytearray(b"I" * n)
                quals[at] = 33 + q
                quals[at - 1] = 33 + 12
                out.append(line(pos, b"C", b"Tt" * (n // 2), bytes(quals)))
                keys.append((CHROM, pos))
    for qlen in (255, 256, 257, 511, 512, 513):
        pos += 1
        out.append(line(pos, b"C", b"tT" * 300, bytes(33 + 12 + (i % 3) for i in range(qlen)), depth=600))
        keys.append((CHROM, pos))
    return b"\n".join(out) + b"\n", keys


ROUTING_TOTALS = (100, 300, 600, 1100, 1500, 2100)


def routing_batch():
    """64 listed sites: 57 short lines, one line each of ROUTING_TOTALS bytes, one 700-byte line of a symbol the lane passes do not
    count (R: well-formed, handed on).  A malformed long line — 700 bytes, five fields, no qualities — stands at an UNLISTED
    position: at a listed one the call raises, as the reference does, and it must disturb neither the scan nor the routing of
    the others.  110 short unlisted lines keep the file's mean line length under 100 bytes (the 128-byte pass runs)."""
    rng = random.Random(11)
    out, keys, pos = [], [], 0
    for i in range(57):
        pos += 1
        out.append(line(pos, b"A", b".,.,G", b"IIIII"))
        keys.append((CHROM, pos))
    for total in ROUTING_TOTALS:
        pos += 1
        out.append(exact_line(pos, total, b"\n", rng))
        keys.append((CHROM, pos))
    pos += 1
    out.append(line(pos, b"A", b"Rr" * 170, b"I" * 340))
    keys.append((CHROM, pos))
    out.append(b"fill\t999\tC\t680\t" + b".," * 340)
    for i in range(110):
        out.append(filler(i + 1, 40, b"\n"))
    return b"\n".join(out) + b"\n", keys


def window_marker_edges():
    """Every marker ending at, beginning at and straddling the last byte of a window (128 .. 2048 bytes; the lines start on a
    16-byte boundary), and indel counts of two and more digits split by the window's end: no pass whose window ends inside the
    marker may call the line, the next one that holds it whole must."""
    out, keys, pos = b"", [], 0
    for win in (128, 256, 512, 1024, 2048):
        for m in MARKERS + (b"+12ACGTACGTACGT", b"-105" + b"n" * 105):
            for at in (win - len(m), win - 1, win, win - 2):     # ends at the last byte; begins at it (a count: sign | digits); begins behind it; one digit each side
                pos += 1
                head = line(pos, b"T", b"", b"", depth=4000)[:-1]                    # ... up to the bases field
                n = at - len(head)
                bases = b"Ac" * (n // 2) + b"A" * (n & 1) + m + b"gT" * 5
                reads = n + 10 + (1 if m == b"*" else 0)
                ln = head + bases + b"\t" + b"I" * reads
                pad = (-len(out)) % 16
                if pad:
                    out += filler(pos, pad + 32, b"\n") + b"\n"
                assert len(out) % 16 == 0 and ln[at:at + len(m)] == m
                out += ln + b"\n"
                keys.append((CHROM, pos))
    return out, keys


def all_lines_file():
    """About 200 lines for the all-lines chain: every LENGTHS entry, the routing lengths, and short lines between them."""
    rng = random.Random(17)
    out, keys = [], []
    for pos in range(1, 201):
        if pos % 8 == 0:
            total = (LENGTHS + ROUTING_TOTALS + (700, 900, 1300))[(pos // 8) % 18]
            out.append(exact_line(pos, total, b"\n", rng))
        else:
            n = rng.randint(3, 60)
            out.append(line(pos, b"G", bytes(rng.choice(b".,ACGTacgt") for _ in range(n)), bytes(rng.randint(33, 74) for _ in range(n))))
        keys.append((CHROM, pos))
    return b"\n".join(out) + b"\n", keys


WINDOWS = (("lanes128", 128, 64), ("lanes256", 256, 128), ("lanes512", 512, 255))


def expected_passes(data, listed=None, term=b"\n"):
    """Which call pass takes each line (each line of a `listed` position, when given) of a file of well-formed lines, by the rule
    the header states: a window of W bytes starts at the 16-byte boundary at or below the line's first byte and holds the line when
    its terminator lies inside it and its bases field is at most 64 / 128 / 255 bytes; a symbol besides *ACGTN (outside '^x' pairs)
    sends the line on; the 128-byte pass does not run when the file's lines average more than 100 bytes; what no window holds is
    the wave-per-site kernel's."""
    lines = data.split(term)[:-1]
    deep = len(data) > 100 * len(lines)
    took = {"lanes128": 0, "lanes256": 0, "lanes512": 0, "wave": 0}
    start = 0
    for ln in lines:
        f = ln.split(b"\t")
        if listed is None or (f[0], int(f[1])) in listed:
            end_at = (start & 15) + len(ln)                      # the terminator's byte in the window
            field = f[4]
            plain = not re.sub(rb"[.,ACGTNacgtn*$+\-0-9]", b"", re.sub(rb"\^.", b"", field))
            name = "wave"
            for cand, win, most in WINDOWS:
                if plain and end_at < win and len(field) <= most and not (deep and win == 128):
                    name = cand
                    break
            took[name] += 1
        start += len(ln) + len(term)
    return took


FUZZ_PARAMS = ((0, 0.6, 3, 0, 0.0), (13, 0.6, 3, 0, 0.0), (15, 0.75, 10, 4, 0.25), (30, 0.9, 2, 1, 0.1), (1, 0.5, 1, 0, 0.5))


def fuzz_slice(seed, n_lines=300):
    """Lines whose byte length, newline included, is drawn uniformly from 400 .. 2300, out of the tokens of oracle/fuzz.py (its bases
    tokens and, on a quarter of the lines, its odd symbols and adversarial strings; all ASCII — the product refuses bytes >= 0x80 by
    design), six fields each, the quality field within a few bytes of one per read."""
    rng = random.Random(seed)
    out, keys = [], []
    for pos in range(1, n_lines + 1):
        total = rng.randint(400, 2300)
        ref = rng.choice(b"ACGTNacgtn").to_bytes(1, "little")
        slack = rng.choice([0, 0, 0, 0, -2, -1, 1, 3])
        toks, size, reads = [], 0, 0
        odd_symbols = rng.random() < 0.25                        # (a line with '#', '<', '>' or an adversarial string is the wave kernel's)
        over = len(line(pos, ref, b"", b"", depth=1000)) + 1
        while over + size + max(0, reads + slack) < total - 1:
            t = fuzz._adversarial(rng) if odd_symbols and rng.random() < 0.02 else fuzz._bases_token(rng)
            if not odd_symbols and t in "#<>":
                t = "*"
            toks.append(t)
            size += len(t)
            reads += 1
        bases = "".join(toks).encode()
        qlen = max(0, reads + slack) + max(0, total - (over + size + max(0, reads + slack)))     # (the last token may overshoot: then no padding)
        out.append(line(pos, ref, bases, bytes(rng.randint(33, 74) for _ in range(qlen)), depth=1000))
        keys.append((CHROM, pos))
    return b"\n".join(out) + b"\n", keys
