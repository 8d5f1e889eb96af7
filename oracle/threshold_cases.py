"""Counts at the rounding edges of the call thresholds, and pileup lines that carry exactly those counts.
TEST INFRASTRUCTURE ONLY (same rules as pileup_oracle.py: tests/, smoke() and bench.py's cpu_baseline may import it).

Every call ends in a threshold test on floating-point numbers that the reference does in IEEE double:

* the consensus caller (pileup.py:564-584, ``pileup_oracle.call_record``): ``n < good * minConsFreq`` and
  ``nf, nr < n * minConsStrdBias`` -- a count against a double PRODUCT;
* VarScan's selection (``varscan_oracle.call_line``): ``reads2 / total < min_var_freq`` -- a double QUOTIENT against the option.

A plausible rewrite (float32, a quotient for a product or the other way round, exact rationals, ``<=``, a fused or extended
product) gives the same verdict almost everywhere and a different one at a few counts.  ``product_cases`` / ``quotient_cases``
find those counts by enumeration, together with the exact ties and the counts one either side of them; ``consensus_line`` and
``varscan_line`` write pileup lines that carry given counts at a given byte length, so that each case can be put in front of
every parser of the HIP library (the line length picks the kernel).
"""
import random
from fractions import Fraction

import numpy as np

MIN_CONS_FREQS = (0.6, 0.55, 0.15, 0.7, 0.75, 0.9, 0.5, 0.0, 1.0)
MIN_CONS_STRAND_BIASES = (0.1, 0.15, 0.25, 0.3, 0.5)
MIN_VAR_FREQS = (0.9, 0.2, 0.55, 0.05)

MIN_BASE_QUAL = 13          # the consensus lines' minBaseQual: '.' (46) is a good read exactly at it, '-' (45) one just below


def _f32(x):
    return np.float32(x)


# "x < y * f": the reference, and the ways it could be written wrongly
PRODUCT_FORMS = {
    "float32": lambda x, y, f: bool(_f32(x) < _f32(y) * _f32(f)),
    "quotient": lambda x, y, f: x / y < f,
    "exact_decimal": lambda x, y, f: Fraction(x) < y * Fraction(repr(f)),
    "less_equal": lambda x, y, f: x <= y * f,
    # fma(y, f, -x) or a long double product: y < 2^11 and f's 53-bit significand fit a 64-bit significand, so both are exact
    "fma_or_long_double": lambda x, y, f: Fraction(x) < y * Fraction(f),
}

# "x / y < f": the reference, and the ways it could be written wrongly.  (Exact rationals are no such way: below 2^26 a double
# quotient equals the option's double only when the decimal quotient equals the decimal option, so their verdicts agree;
# QUOTIENT_EQUIVALENT holds that form, and a test checks that it does agree on every case.)
QUOTIENT_FORMS = {
    "float32": lambda x, y, f: float(_f32(x) / _f32(y)) < f,            # (the option stays a double, as in the kernels' parameters)
    "product": lambda x, y, f: x < y * f,
    "less_equal": lambda x, y, f: x / y <= f,
    "long_double": lambda x, y, f: Fraction(x, y) < Fraction(f),        # (an extended quotient: exact for these sizes' verdicts)
}

QUOTIENT_EQUIVALENT = {"exact_decimal": lambda x, y, f: Fraction(x, y) < Fraction(repr(f))}


def product_ref(x, y, f):
    return x < y * f


def quotient_ref(x, y, f):
    return x / y < f


def _cases(ref, forms, values, depth_max, ties_per_value):
    """(x, y, f) with 1 <= y <= depth_max and 0 <= x <= y: every x where a form other than "<=" disagrees with `ref`, and
    the decimal ties x = y * f with x - 1 and x + 1 at `ties_per_value` depths per value (the first ones, then spread out)."""
    out = set()
    for f in values:
        fd = Fraction(repr(f))
        ties = []
        for y in range(1, depth_max + 1):
            t = y * fd
            lo, hi = max(0, int(t) - 1), min(y, int(t) + 2)
            for x in range(lo, hi + 1):
                r = ref(x, y, f)
                if any(m(x, y, f) != r for k, m in forms.items() if k != "less_equal"):
                    out.add((x, y, f))
            if t.denominator == 1:
                ties.append(y)
        keep = ties[:ties_per_value // 2]
        rest = ties[ties_per_value // 2:]
        if rest:
            step = max(1, len(rest) // (ties_per_value - len(keep)))
            keep += rest[step - 1::step][:ties_per_value - len(keep)]
        for y in keep:
            x0 = int(y * fd)
            for x in (x0 - 1, x0, x0 + 1):
                if 0 <= x <= y:
                    out.add((x, y, f))
    return sorted(out, key=lambda c: (c[2], c[1], c[0]))


def product_cases(values, depth_max=400, ties_per_value=12):
    return _cases(product_ref, PRODUCT_FORMS, values, depth_max, ties_per_value)


def quotient_cases(values, depth_max=400, ties_per_value=12):
    return _cases(quotient_ref, QUOTIENT_FORMS, values, depth_max, ties_per_value)


# ---- consensus cases: counts per symbol ----------------------------------------------------------------------------------
# The lane kernels know the symbols * A C G N T; a position whose minority reads need more symbols than that (a consensus
# frequency under 1/6) takes its other symbols from IUPAC codes, which the wave-per-site kernel ranks like any other byte.
OTHERS = b"CGTN*RYKMSWBDHV"


def _spread(total, n, cons):
    """`total` minority reads over symbols other than `cons`, none with more reads than the consensus (n) — a symbol that
    sorts before `cons` strictly fewer — as {symbol: count}."""
    out = {}
    for s in OTHERS:
        if total == 0:
            break
        if s == cons:
            continue
        k = min(total, n if s > cons else n - 1)
        if k > 0:
            out[s] = k
            total -= k
    if total:
        raise ValueError("cannot spread the minority reads")
    return out


def consensus_counts(n, nf, good, cons=0x41):
    """{symbol: (forward, reverse)} with `good` reads, `n` of them (nf forward) on the consensus symbol `cons`, and the rest
    on other symbols, split between the strands."""
    counts = {cons: (nf, n - nf)}
    for i, (s, k) in enumerate(sorted(_spread(good - n, n, cons).items())):
        f = k if s == 0x2A else (k + i % 2) // 2              # '*' has no reverse-strand spelling
        counts[s] = (f, k - f)
    return counts


def consensus_cases():
    """[(kind, counts, params)]: kind names the test at its edge; params is (min_cons_freq, min_cons_depth,
    min_cons_strand_depth, min_cons_strand_bias) of the run the case was made for (every run calls every case)."""
    out = []
    for x, y, f in product_cases(MIN_CONS_FREQS):
        if y - x > 14 * max(x, 1) or x == 0:
            continue                                          # (no consensus of x reads among y: it needs x >= the others)
        out.append(("VarFreq", consensus_counts(x, (x + 1) // 2, y), (f, 1, 0, 0.0)))
    for x, y, b in product_cases(MIN_CONS_STRAND_BIASES, ties_per_value=10):
        if x * 2 > y:
            continue                                          # nf = x, nr = y - x: the lesser strand is the one at the edge
        out.append(("StrBias", consensus_counts(y, x, y), (0.0, 1, 0, b)))
    for d in (1, 10, 37):                                     # minConsDpth and minConsStrdDpth at D - 1, D, D + 1
        for n in (d - 1, d, d + 1):
            if n >= 1:
                out.append(("Depth", consensus_counts(n, n // 2, n + n // 3), (0.0, d, 0, 0.0)))
            if n >= 0:
                out.append(("StrDpth", consensus_counts(n + d + 1, n, n + d + 1), (0.0, 1, d, 0.0)))
    return out


def _qual(q):
    return bytes([q + 33])


def consensus_line(chrom, pos, ref, counts, low=0, length=None, raw_depth=None, seed=0, min_base_quality=MIN_BASE_QUAL):
    """One pileup line (bytes, no terminator): `counts` {upper symbol byte: (forward, reverse)} reads at or above
    min_base_quality (the reference base spelled '.' / ','), `low` reads below it; padded to `length` bytes with indel
    text, '^X' read starts and '$' read ends, none of which counts.  ValueError when the counts alone are longer."""
    rng = random.Random(seed)
    ref_u = ref.upper()[0]
    reads = []
    for sym, (f, r) in sorted(counts.items()):
        for strand, k in ((0, f), (1, r)):
            for _ in range(k):
                if sym == ref_u:
                    b = b"," if strand else b"."
                else:
                    b = bytes([sym + 32 if strand and 0x41 <= sym <= 0x5A else sym])
                reads.append([b, _qual(rng.choice((min_base_quality, min_base_quality, 40)))])
    for i in range(low):
        reads.append([b"acgtACGT"[i % 8:i % 8 + 1], _qual(max(0, min_base_quality - 1 - (i % 2) * min(9, min_base_quality - 1)))])
    rng.shuffle(reads)
    quals = b"".join(q for _, q in reads)
    depth = len(reads) if raw_depth is None else raw_depth
    head = b"%s\t%d\t%s\t%d\t" % (chrom, pos, ref, depth)
    core = len(head) + sum(len(b) for b, _ in reads) + 1 + len(quals)
    if length is None:
        return head + b"".join(b for b, _ in reads) + b"\t" + quals
    rest = length - core
    if rest < 0:
        raise ValueError("the counts need %d bytes" % core)
    pre, post = [b""] * len(reads), [b""] * (len(reads) + 1)    # text in front of / behind read i (post[-1]: with no reads)
    slots = len(reads) if reads else 1
    while rest >= 8:                                          # indels (+k / -k and k bases): the bulk of the padding
        k = rng.randint(1, min(600, rest - 4))
        text = (b"+" if rng.random() < 0.5 else b"-") + str(k).encode() + bytes(rng.choice(b"ACGTNacgtn") for _ in range(k))
        if len(text) > rest:
            continue
        post[rng.randrange(slots)] += text
        rest -= len(text)
    free = [i for i in range(len(reads))]
    rng.shuffle(free)
    while rest >= 2 and free and rng.random() < 0.7:          # ^X: a read start and its mapping quality
        pre[free.pop()] = b"^" + bytes([rng.choice(b"!5FK]~")])
        rest -= 2
    for _ in range(rest):                                     # $: read ends
        post[rng.randrange(slots)] += b"$"
    bases = b"".join(pre[i] + b + post[i] for i, (b, _) in enumerate(reads)) + (post[0] if not reads else b"")
    line = head + bases + b"\t" + quals
    assert len(line) == length, (len(line), length)
    return line


# ---- VarScan cases ------------------------------------------------------------------------------------------------------
def varscan_cases(min_avg_qual):
    """[(kind, spec, params)]: spec is the keyword set of varscan_line, params the varscan_oracle.Params keywords of the run the
    case was made for (every run calls every case).  The frequency cases split total into reads1, reads2 and indel reads."""
    m = min_avg_qual
    out = []
    for i, (x, y, f) in enumerate(quotient_cases(MIN_VAR_FREQS)):
        if x == 0:
            continue
        indel = (y - x) // 3 if i % 2 else 0
        r1 = y - x - indel
        out.append(("VarFreq", dict(rdf=r1 - r1 // 3, rdr=r1 // 3, adf=x - x // 2, adr=x // 2, indel=indel, n_reads=i % 3),
                    dict(min_coverage=1, min_reads2=1, min_avg_qual=m, min_var_freq=f)))
    cov, r2 = 20, 7
    for d in (cov - 1, cov, cov + 1):                         # --min-coverage on the depth column, then on the quality depth
        out.append(("SDP", dict(rdf=10, rdr=9, adf=4, adr=4, sdp=d), dict(min_coverage=cov, min_reads2=2, min_avg_qual=m, min_var_freq=0.05)))
        out.append(("DP", dict(rdf=d - 9, rdr=3, adf=3, adr=3, sdp=40), dict(min_coverage=cov, min_reads2=2, min_avg_qual=m, min_var_freq=0.05)))
    for d in (r2 - 1, r2, r2 + 1):                            # --min-reads2
        out.append(("Reads2", dict(rdf=12, rdr=11, adf=d - d // 2, adr=d // 2), dict(min_coverage=8, min_reads2=r2, min_avg_qual=m, min_var_freq=0.05)))
    # --min-avg-qual: every variant read exactly at it (quality sum m * reads2), and one of them a point below (that read drops out)
    for k in (5, 6, 9):
        out.append(("AvgQual", dict(rdf=6, rdr=6, adf=k - 2, adr=2, alt_exact=True), dict(min_coverage=8, min_reads2=5, min_avg_qual=m, min_var_freq=0.05)))
        out.append(("AvgQual", dict(rdf=6, rdr=6, adf=k - 2, adr=2, alt_exact=True, alt_one_below=True),
                    dict(min_coverage=8, min_reads2=5, min_avg_qual=m, min_var_freq=0.05)))
    return out


def varscan_line(chrom, pos, ref, rdf=0, rdr=0, adf=0, adr=0, alt=b"G", indel=0, n_reads=0, low=0, sdp=None, alt_exact=False,
                 alt_one_below=False, min_avg_qual=15, length=None, seed=0):
    """One pileup line (bytes, no terminator) that VarScan reads back as: rdf / rdr reference reads and adf / adr `alt` reads at
    or above min_avg_qual, `indel` reads with an insertion or deletion, `n_reads` N reads at or above it (quality depth only),
    `low` reads below it (nothing), depth column `sdp` (default: one per quality); every variant read exactly AT min_avg_qual
    with alt_exact (alt_one_below: one more variant read a point below it).  Padded to `length` bytes with '^X' read starts and
    '$' read ends (indel text would count)."""
    rng = random.Random(seed)
    m = min_avg_qual
    hi = max(m, min(m + 25, 222))
    q = lambda: bytes([33 + rng.randint(m, hi)])              # noqa: E731
    reads = [[b".", q()] for _ in range(rdf)] + [[b",", q()] for _ in range(rdr)]
    a = alt.upper()
    reads += [[a, bytes([33 + m]) if alt_exact else q()] for _ in range(adf)] + [[a.lower(), bytes([33 + m]) if alt_exact else q()] for _ in range(adr)]
    if alt_one_below:
        reads.append([a, bytes([33 + m - 1])])
    reads += [[b"nN*"[i % 3:i % 3 + 1], q()] for i in range(n_reads)]
    reads += [[b"ACGTacgt"[i % 8:i % 8 + 1], bytes([33 + rng.randint(max(0, m - 12), m - 1)])] for i in range(low)] if m > 0 else []
    rng.shuffle(reads)
    ind = []
    for i in range(indel):
        k = 1 + i % 3
        ind.append((rng.randrange(len(reads) + 1), (b"+" if i % 2 else b"-") + str(k).encode() + bytes(rng.choice(b"ACGTacgt") for _ in range(k))))
    quals = b"".join(x for _, x in reads)
    head = b"%s\t%d\t%s\t%d\t" % (chrom, pos, ref, len(reads) if sdp is None else sdp)
    pre, post = [b""] * (len(reads) + 1), [b""] * (len(reads) + 1)
    for slot, text in ind:
        post[slot] += text
    core = len(head) + sum(len(b) for b, _ in reads) + sum(len(t) for _, t in ind) + 1 + len(quals)
    if length is not None:
        rest = length - core
        if rest < 0:
            raise ValueError("the counts need %d bytes" % core)
        free = list(range(len(reads)))
        rng.shuffle(free)
        while rest >= 2 and free and rng.random() < 0.7:
            pre[free.pop()] = b"^" + bytes([rng.choice(b"!5FK]~")])
            rest -= 2
        for _ in range(rest):
            post[rng.randrange(len(reads) + 1)] += b"$"
    bases = b"".join(pre[i] + b + post[i] for i, (b, _) in enumerate(reads)) + post[len(reads)]
    line = head + bases + b"\t" + quals
    assert length is None or len(line) == length, (len(line), length)
    return line


def varscan_records(data, prm, cache=None):
    """What the device pass of phase-1 site calling returns for a pileup (bytes), restated with varscan_oracle's counting: one
    tuple (line offset, sdp, dp, total, rdf, rdr, ref quality sum, adf, adr, alt quality sum, ref, alt) per (line, allele) that
    passes --min-coverage, --min-reads2, --min-avg-qual and --min-var-freq — before Fisher's test and --p-value.  cache: a dict
    that keeps each line's counts for later calls with the same data and min_avg_qual."""
    from oracle import varscan_oracle as vo
    out = []
    off = 0
    for line in data.split(b"\n"):
        start, off = off, off + len(line) + 1
        f = line.split(b"\t")
        if len(f) < 6:
            continue
        depth = int(f[3])
        if depth < prm.min_coverage:
            continue
        key = (start, prm.min_avg_qual)
        if cache is None or key not in cache:
            got = (vo.quality_depth(f[5], prm.min_avg_qual), vo.read_counts(f[4], f[5], prm.min_avg_qual))
            if cache is None:
                cache = {}
            cache[key] = got
        dp, c = cache[key]
        if dp < prm.min_coverage:
            continue
        ref = f[2].upper()[0]
        total = c.total()
        for allele in sorted(c.alt):
            fw, rv, qs = c.alt[allele]
            reads2 = fw + rv
            if ord(allele) == ref or reads2 == 0:
                continue
            if reads2 >= prm.min_reads2 and qs // reads2 >= prm.min_avg_qual and float(reads2) / float(total) >= prm.min_var_freq:
                out.append((start, depth, dp, total, c.ref[0], c.ref[1], c.ref[2], fw, rv, qs, ref, ord(allele)))
    return out
