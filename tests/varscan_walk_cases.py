"""Cases for the WALK of the site-calling scan (the exact read-base automaton behind phase B of k_varscan_scan,
snp_pipeline_amd/csrc/varscan.hip), and a CPU statement of the route a candidate line takes to it.

The automaton exists three times - varscan_line (byte-wise, global memory), varscan_core_lds behind the VS_W_PLAIN shortcut and
varscan_core_lds behind varscan_parse_lds - and which copy a line meets hangs on where the line lies, how many candidates its wave
has and how long they are.  The routes:

  A   ring strips, a VS_W_PLAIN entry still in the wave's LDS list when its tiles are done
  B   ring strips, an entry parsed by varscan_parse_lds
  C   ring strips, an entry read back from the wave's own stretch of the spill (flush() once n_local + 64 > VS_CAND_LOCAL)
  D   ring strips, rounds 2 to 4 of a group of up to 64
  E   epilogue strips (k_varscan_finish): a known-end entry that found no room in four rounds, or that flush() put on the shared list
  F1  epilogue, byte-wise: a VS_W_LONG entry (walk_entry_global finds the end at LF, CR or the end of the file)
  F2  epilogue, byte-wise: a known-end entry behind the first 32 KiB of its group of 64
  G   on the spot, byte-wise: the shared list is full

What lives here, all plain Python:

  plan()        per wave of a launch over ONE pileup with LF line ends: the order in which candidates enter cand_local (per tile the
                VS_W_LONG entry first, then the rounds of phase B, lane-minor, the carried line on the lowest lane without a line of
                its own), where flush() fires, whether a flush goes to the wave's stretch or to the shared list, the groups of 64 of
                the tail loop, the chunk count of every entry, the prefix-sum packing against the strip budget and the round an
                entry is walked in - or that it goes to the shared list.  Written from the kernel's comments with dealing(),
                filter_model() and effective() of tests/varscan_scan_cases.py.
  epilogue_fit() / epilogue_bounds()
                which entries of a group of 64 of the shared list fit the epilogue's 32 KiB: exactly where the list order is
                determined (all entries from one atomic of one wave, at the head of the list), else bounds by count.
  CATALOGUE     (read bases, qualities) tokens for every branch of the automaton, each in a PLAIN and a PARSED line shape.
  family_*      the pileups of tests/test_gpu_varscan_walk.py.

THE STATEMENT PROVES REACH, NEVER RESULTS: it shows that a case takes the route it is named for.  Every expected record comes from
oracle/threshold_cases.varscan_records through varscan_scan_cases.expected (oracle/varscan_oracle.py's counting, Python integers)."""
import os
import re
from collections import namedtuple

import numpy as np

from oracle import varscan_oracle as vo
from tests import varscan_scan_cases as vc

VS_TILE, VS_PAD, VS_RING, VS_CAND_LOCAL = vc.VS_TILE, vc.VS_PAD, vc.VS_RING, vc.VS_CAND_LOCAL
# what the statements below are written for; source_constants() reads the same from varscan.hip and the CPU suite compares
VS_DATA = 2 * (VS_PAD + VS_TILE)
VS_STR_WORDS, VS_STR_PAD = VS_RING // 32, 4
RING_STRIP_BYTES = VS_DATA + 3 * (VS_STR_WORDS + VS_STR_PAD) * 4 - 16      # 11 424: the slots, the strings and the counts, less one chunk
EPI_STRIP_BYTES = 32 * 1024
ROUNDS = 4
CAP_DIV, CAP_FLOOR, CAP_MAX = 128, 2 * vc.MAX_WAVES * 64, 1 << 23


def source_constants():
    src = open(os.path.join(vc.ROOT, "snp_pipeline_amd", "csrc", "varscan.hip")).read()
    one = lambda pat: re.search(pat, src).groups()                                       # noqa: E731
    a, b = one(r"const uint32_t strip_bytes = (\d+)u \* (\d+)u;")
    div, k, per = one(r"const uint64_t c = nbytes / (\d+) \+ (\d+) \* VARSCAN_MAX_WAVES \* (\d+);")
    return dict(VS_DATA="#define VS_DATA (2u * (VS_PAD + VS_TILE))" in src, VS_STR_WORDS="#define VS_STR_WORDS (VS_RING / 32u)" in src,
                VS_STR_PAD=int(one(r"#define VS_STR_PAD (\d+)u")[0]),
                ring_budget="walk_in_strips((uint4 *)ring, VS_DATA + 3u * (VS_STR_WORDS + VS_STR_PAD) * 4u - 16u, have, e, fo, prm)" in src,
                epi_budget=int(a) * int(b), epi_call="walk_in_strips(vs_strips, strip_bytes, have, e, o, prm)" in src,
                rounds=int(one(r"for \(int round = 0; round < (\d+) && __builtin_amdgcn_ballot_w64\(have\); \+\+round\)")[0]),
                cap=(int(div), int(k) * vc.source_constants()["MAX_WAVES"] * int(per), 1 << int(one(r"return \(uint32_t\)\(c < \(1ull << (\d+)\) \? c : \(1ull << \d+\)\);")[0])),
                halves="const uint32_t shared_cap = cand_cap / 2, spill_per_wave = (cand_cap - shared_cap) / n_waves_total;" in src,
                flush_at=src.count("if (n_local + 64u > VS_CAND_LOCAL) { flush(); dma_mask = 0; __builtin_amdgcn_wave_barrier(); }"),
                stretch_first="if (n_spilled + n_local <= spill_per_wave) {" in src,
                full=("if (base + k < cand_cap) cand[base + k] = e;" in src, "if (at < cand_cap) cand[at] = e;" in src),
                chunks="a0 = ((uintptr_t)o.buf + p0) & ~(uint64_t)15, a1 = (have && !is_long) ? (((uintptr_t)o.buf + end) + 15) & ~(uint64_t)15 : a0;" in src,
                lds_first="have ? (r + lane < n_local ? cand_local[r + lane] : my_spill[r + lane - n_local])" in src,
                guard=src.count("if (size < (1ull << 40)) size = size * 10 +"))


def cand_cap(nbytes):
    """varscan_cand_cap: entries of the candidate list of a launch over nbytes bytes."""
    return min(nbytes // CAP_DIV + CAP_FLOOR, CAP_MAX)


def caps(nbytes, n_waves):
    """(shared_cap, spill_per_wave) as varscan_launch splits the list."""
    cap = cand_cap(nbytes)
    return cap // 2, (cap - cap // 2) // n_waves


def chunks_of(x, length):
    """16-byte chunks walk_in_strips copies for a line of `length` bytes (terminator included) at aligned coordinate x."""
    return ((x & 15) + length + 15) // 16


# ---- the route of every candidate of a launch -------------------------------------------------------------------------------------
Cand = namedtuple("Cand", "line kind source route")
# line: index into the pileup's lines; kind: "plain" (VS_W_PLAIN) / "walk" (parsed) / "long" (VS_W_LONG); source: where the tail loop
# or the flush found the entry: "lds", "stretch", "flush" (flush() put it on the shared list); route: 1..4 = the round of its group
# of 64 it is walked in from the ring's strips, "shared" = onto the shared list (for the epilogue, or on the spot when that is full)


class WavePlan(object):
    def __init__(self, wave):
        self.wave, self.cands, self.flushes, self.atomics, self.groups = wave, [], [], [], []
        # flushes: [(entries, "stretch" | "shared")] in order; atomics: entries per atomicAdd on the shared list, in the wave's order;
        # groups: [[index into cands]] of the tail loop

    def count(self, route=None, source=None, kind=None):
        return sum(1 for c in self.cands if (route is None or c.route == route) and (source is None or c.source == source) and (kind is None or c.kind == kind))


def split_lf(data):
    """[(offset, content)] of a pileup whose lines all end with LF."""
    assert data.endswith(b"\n") and b"\r" not in data
    out, at = [], 0
    for ln in data[:-1].split(b"\n"):
        out.append((at, ln))
        at += len(ln) + 1
    return out


def plan(lines, nbytes, lo, n_cu, kw, _verdicts=None):
    """[WavePlan] of a launch over one pileup: `lines` = [(offset, content)] in file order, every line ended by one LF, the last one
    by the file's last byte; lo: the aligned coordinate of the file's first byte; kw: the parameter set (min_coverage and min_reads2
    decide which plain lines phase B drops).  Exact where every line has its first four TABs within its first 32 bytes (asserted:
    then the window phase B looks through does not depend on the other lanes' lines)."""
    p = vo.Params(**kw)
    T = VS_TILE
    n_tiles, runs = vc.dealing(nbytes, lo, n_cu)
    shared_cap, spw = caps(nbytes, len(runs))
    hi = lo + nbytes
    verdicts = {} if _verdicts is None else _verdicts
    terms = {}                                                  # tile -> [(position in the tile, the line that starts behind it or None)]
    ends, fate, xs = [], [], []

    def add(t_abs, li):
        terms.setdefault(t_abs // T, []).append((t_abs % T, li))

    add(lo - 1, 0 if lines else None)                           # the virtual terminator in front of the file
    for i, (off, c) in enumerate(lines):
        x, e = off + lo, off + len(c) + lo
        add(e, i + 1 if i + 1 < len(lines) else None)
        xs.append(x)
        ends.append(e)
        if not c:
            fate.append(None)                                   # an empty line: nothing
            continue
        if c not in verdicts:
            v = vc.filter_model(c, p.min_coverage, p.min_reads2)
            assert len([t for t in c[:32] if t == 9]) >= 4, c[:40]
            verdicts[c] = v
        k = (x - 1) // T
        e_rel = e - k * T
        fate.append(vc.effective(verdicts[c], vc.Where(k, x - k * T, None, None, e_rel, e_rel >= T, e_rel >= 2 * T)))
    assert ends[-1] == hi - 1, "the pileup ends with LF"
    add(hi, None)                                               # the virtual terminator behind the file
    out = []
    for g, (a, b) in enumerate(runs):
        w = WavePlan(g)
        local, spilled, shared = [], [], []                     # (line, kind) each

        def flush():
            if not local:
                return
            if len(spilled) + len(local) <= spw:
                spilled.extend(local)
                w.flushes.append((len(local), "stretch"))
            else:
                shared.extend(local)
                w.flushes.append((len(local), "shared"))
                w.atomics.append(len(local))
            del local[:]

        def push(items):
            local.extend(items)
            if len(local) + 64 > VS_CAND_LOCAL:
                flush()

        carried = None
        for k in range(a, min(b, n_tiles - 1) + 1):
            tl = terms.get(k, [])
            if carried is not None and not tl:                  # it runs on past this tile: end unknown
                push([(carried, "long")])
                carried = None
            lanes = {}
            if k < b:                                           # one of the wave's own tiles; else only the line carried into it
                for pos, li in tl:
                    lanes.setdefault(pos // 64, []).append(li)
            handed, r = None, 0
            while True:
                busy = sorted(L for L in lanes if len(lanes[L]) > r)
                if not busy and carried is None:
                    break
                taker = None
                if carried is not None:
                    bs = set(busy)
                    taker = next((L for L in range(64) if L not in bs), None)
                got = []
                for L in sorted(busy + ([taker] if taker is not None else [])):
                    if L == taker:
                        li, carried = carried, None
                    else:
                        li = lanes[L][r]
                        if li is None:                          # the terminator starts no line (it is behind the file's last byte)
                            continue
                        if ends[li] // T > k:                   # its line ends in a later tile: handed on
                            handed = li
                            continue
                    if fate[li] is not None and fate[li] != "dropped":
                        assert fate[li] in ("plain", "walk"), (li, fate[li])
                        got.append((li, fate[li]))
                if got:
                    push(got)
                r += 1
            carried = handed
        # the tail loop: first what is still in LDS, then the wave's stretch; groups of 64, four rounds each
        mine = [(li, kind, "lds") for li, kind in local] + [(li, kind, "stretch") for li, kind in spilled]
        route = {}
        for r0 in range(0, len(mine), 64):
            grp = list(range(r0, min(r0 + 64, len(mine))))
            w.groups.append(grp)
            have = list(grp)
            for rnd in range(1, ROUNDS + 1):
                if not have:
                    break
                tot, done = 0, []
                for idx in have:
                    li, kind, _ = mine[idx]
                    ch = 0 if kind == "long" else chunks_of(xs[li], ends[li] + 1 - xs[li])
                    alone = ch * 16 <= RING_STRIP_BYTES
                    tot += ch if alone else 0
                    if kind != "long" and alone and tot * 16 <= RING_STRIP_BYTES:
                        done.append(idx)
                if not done:
                    break
                for idx in done:
                    route[idx] = rnd
                have = [idx for idx in have if idx not in set(done)]
            if have:
                w.atomics.append(len(have))
        w.cands = [Cand(li, kind, src, route.get(idx, "shared")) for idx, (li, kind, src) in enumerate(mine)]
        w.cands += [Cand(li, kind, "flush", "shared") for li, kind in shared]
        w.shared_cap, w.spill_per_wave = shared_cap, spw
        out.append(w)
    return out


def epilogue_fit(entries):
    """entries: [(x, length, is_long)] of ONE group of 64 of the shared list, in list order -> per entry "E" (walked from the
    epilogue's strips), "F1" (end unknown: byte-wise) or "F2" (behind the 32 KiB: byte-wise).  One round: k_varscan_finish does not
    come back to a group."""
    assert len(entries) <= 64
    tot, out = 0, []
    for x, length, is_long in entries:
        ch = 0 if is_long else chunks_of(x, length)
        alone = ch * 16 <= EPI_STRIP_BYTES
        tot += ch if alone else 0
        out.append("F1" if is_long else "E" if alone and tot * 16 <= EPI_STRIP_BYTES else "F2")
    return out


def epilogue_bounds(n, min_bytes, max_bytes):
    """Where the order of the shared list is not determined: of n known-end entries of min_bytes..max_bytes each (terminator
    included, any alignment), at least how many are walked from the epilogue's strips and at least how many behind them - every full
    group of 64 packs at least floor(32 KiB / the largest chunked length) and at most floor(32 KiB / the smallest)."""
    big, small = 16 * ((15 + max_bytes + 15) // 16), 16 * ((min_bytes + 15) // 16)
    full = n // 64
    at_least_in = full * min(64, EPI_STRIP_BYTES // big)
    at_least_behind = full * max(0, 64 - EPI_STRIP_BYTES // small)
    return at_least_in, at_least_behind


# ---- parameter sets -------------------------------------------------------------------------------------------------------------------
Q0 = dict(min_coverage=1, min_reads2=2, min_avg_qual=0, min_var_freq=0.0001)       # the past-the-end qualities (0) count
Q15 = dict(min_coverage=1, min_reads2=2, min_avg_qual=15, min_var_freq=0.0001)     # the fast path for four reference matches is on
Q100 = dict(min_coverage=1, min_reads2=2, min_avg_qual=100, min_var_freq=0.0001)   # qmin 133: the fast path is off, only bytes >= 0x85 count
PARAM_SETS = {"Q0": Q0, "Q15": Q15, "Q100": Q100}


# ---- the token catalogue ----------------------------------------------------------------------------------------------------------------
def owners(bases):
    """How many bytes of a read-base string own a quality (only to give a token as many qualities as it asks for: no expected
    value comes from here)."""
    i = n = 0
    while i < len(bases):
        c = bases[i]
        if c in b".,ACGTacgtNn*":
            n += 1
        elif c in b"+-":
            k, size = i + 1, 0
            while k < len(bases) and 0x30 <= bases[k] <= 0x39:
                size, k = size * 10 + bases[k] - 0x30, k + 1
            if k > i + 1:
                i = k + size - 1
        elif c == 0x5E:
            i += 1
        i += 1
    return n


QUAL_POOL = b"05:?DI+!&NSX]bgl"                                 # Q15 and up, three below it ('+', '!', '&'), letters and not


def quals_of(n, k=0):
    return bytes(QUAL_POOL[(k + 5 * i) % 16] for i in range(n))


HEAD = (b"Gg", b"IF")                                            # in front of every token: two variant reads (min_reads2), so a wrong count changes a record
HEAD_HI = (b"Gg", b"\x90\x91")                                   # ... that also pass --min-avg-qual 100

Token = namedtuple("Token", "name ref bases quals sets eats")
# sets: the parameter sets under which the token's line yields a record; eats: it runs off the end of the column (a tail token only)


def _tok(name, core, delta=0, quals=None, ref=b"A", hi=False, eats=False, k=0, whole=None, sets=None):
    head = HEAD_HI if hi else HEAD
    bases = head[0] + core
    if whole is not None:
        q = whole
    elif quals is not None:
        q = head[1] + quals
    else:
        q = head[1] + quals_of(owners(core) + delta, k)
    return Token(name, ref, bases, q, sets or (("Q0", "Q15", "Q100") if hi else ("Q0", "Q15")), eats)


def _catalogue():
    t = []
    # reference matches: runs of 3, 4, 5, 8 (the 16 alignments of family i start each at every byte of a word)
    for n in (3, 4, 5, 8):
        t.append(_tok("run%d" % n, b"A" + b".,.,.,.,"[:n] + b"C", k=n))
    t.append(_tok("run8_dots", b"........c", k=3))
    t.append(_tok("run8_commas", b",,,,,,,,T", k=4))
    # a run of four at the end of the column whose qualities end 3, 4 and 5 bytes behind the cursor (j + 4 <= q1)
    for d in (-1, 0, 1):
        t.append(_tok("run4_quals_end_%d" % (4 + d), b"a.,.,", delta=d, k=6 + d))
    t.append(_tok("low_quality_in_a_fast_word", b".,.,.,.,", quals=b"5!5:5/0I"))             # '/' one below Q15, '0' at it
    t.append(_tok("high_quality_byte_in_a_fast_word", b".,.,.,.,", quals=b"5\x855\x80\xff5:\x84", hi=True))
    # bases and case
    t.append(_tok("every_base_ref_A", b"ACGTacgtNn*AACCGGTT", k=1))
    t.append(_tok("every_base_ref_c", b"ACGTacgtNn*aaccggtt", ref=b"c", k=2))
    t.append(_tok("every_base_ref_N", b"AaCcGgTt.,*nN", ref=b"N", k=3))
    t.append(_tok("every_base_ref_g", b"TtGgCcAa,.", ref=b"g", k=4))
    t.append(_tok("every_base_high_quality", b"ACGTacgt.,Nn*", quals=bytes(range(0x83, 0x90)), hi=True))
    # non-digit, non-base bytes
    t.append(_tok("dollar_skips_lone_digit", b".$,<A>#5,.", k=5))
    t.append(_tok("bit7_set", b".\xc7,\xae\xc1\xe7.\xac\xce\xaaA", k=6))                    # an allele or '.' / ',' / 'N' / '*' with bit 7 set: skipped, no quality
    t.append(_tok("control_bytes", b".\x01,\x0bA\x0c \x7f,", k=7))
    t.append(_tok("bytes_around_the_sets", b".@[`{/:-,a", k=8))                             # ('-' without a digit)
    # '^': the next byte is a mapping quality
    t.append(_tok("caret_dot", b".^.,A", k=9))
    t.append(_tok("caret_letter", b",^Ga.", k=10))
    t.append(_tok("caret_plus", b".^+2A,", k=11))
    t.append(_tok("caret_caret", b".^^A,", k=12))
    t.append(_tok("caret_last", b".,A^", k=13, eats=True))
    t.append(_tok("caret_then_last", b".,A^~", k=14))
    t.append(_tok("caret_then_run", b"A^F.,.,.,.,g", k=15))
    t.append(_tok("caret_tab_like", b".^$c^,,A", k=0))
    # indels: 1, 2, 3, 4 digits
    t.append(_tok("ins1", b".+1A,", k=1))
    t.append(_tok("del2", b".-2ac,C", k=2))
    t.append(_tok("ins12", b".+12ACGTACGTACGT,a", k=3))
    t.append(_tok("del100", b",-100" + b"acgt" * 25 + b"A.", k=4))
    t.append(_tok("ins1000", b".+1000" + b"ACGT" * 250 + b"c,", k=5))
    t.append(_tok("ins0003", b",+0003ACG.t", k=6))
    t.append(_tok("ins_ends_the_column", b".,A+3ACG", k=7, eats=True))
    t.append(_tok("ins_one_short", b".,A+2AC.", k=8))
    t.append(_tok("ins_one_past", b".,A+4ACG", k=9, eats=True))
    t.append(_tok("sign_no_digit", b".+A,-c", k=10))
    t.append(_tok("plus_last", b".,A+", k=11, eats=True))
    t.append(_tok("minus_last", b".,a-", k=12, eats=True))
    t.append(_tok("plus3_last", b".,A+3", k=13, eats=True))
    t.append(_tok("len_2p40_less_1", b".,A+1099511627775ACGT.,", k=14, eats=True))
    t.append(_tok("len_2p40", b".,A-1099511627776acgt.,", k=15, eats=True))
    t.append(_tok("len_2p64_plus_1", b".,A+18446744073709551617ACGT.,", k=0, eats=True))
    t.append(_tok("len_25_digits", b".,A+1844674407370955161600002ACGT.,", k=1, eats=True))  # 100 000 * 2^64 + 2
    t.append(_tok("indel_then_run", b"A-1c.,.,.,.,G", k=2))
    t.append(_tok("indel_then_caret", b".+2AC^!G,", k=3))
    t.append(_tok("indel_then_indel", b".+1A-1c+2GT,C", k=4))
    # qualities
    t.append(_tok("quals_short", b"ACGT.,.,acgt", delta=-5, k=5))
    t.append(_tok("quals_long", b"ACGT.,.,acgt", delta=4, k=6))
    t.append(_tok("quals_one_byte", b"A.,", whole=b"I", sets=("Q0",)))           # (past the end: quality 0, which only --min-avg-qual 0 counts)
    t.append(_tok("quals_with_space", b"A.,.,c", quals=b"I 5 :I", k=7))
    t.append(_tok("quals_all_high", b"AaCc.,.,.,", quals=b"\x84\x85\x86\x87\x84\x85\xfe\xff\x80\x85", hi=True))
    t.append(_tok("star_and_n_own_a_quality", b"*N.n*,A", k=8))
    # ... and the same length in a line short enough for family iv (its PARSED shape takes a seventh column: an even index)
    t.append(_tok("len_2p64_plus_1_short", b"+18446744073709551617AC", eats=True))
    assert len({x.name for x in t}) == len(t) and len(t) % 2 == 1
    return t


CATALOGUE = _catalogue()
PLAIN, PARSED = "plain", "parsed"


def shape_line(name, pos, ref, bases, quals, shape, k=0):
    """PLAIN: the depth column says len(quals), five TABs.  PARSED: the same line with a seventh column (k even) or with its
    depth written with five digits (k odd): the scan's shortcut cannot vouch for either."""
    depth = len(quals)
    assert 1 <= depth <= (9999 if shape == PLAIN else 99999)
    if shape == PLAIN:
        return vc.probe(name, pos, ref, b"%d" % depth, bases, quals)
    if k % 2 == 0:
        return vc.probe(name, pos, ref, b"%d" % depth, bases, quals) + b"\tx"
    return vc.probe(name, pos, ref, b"%05d" % depth, bases, quals)


def token_line(ti, shape, pad=0, pos=None):
    t = CATALOGUE[ti]
    return shape_line(b"c", 1 + ti if pos is None else pos, t.ref, b"$" * pad + t.bases, t.quals, shape, ti)


MID = b".,.,.,.,.,A.,.,c$.,^F.,.,.,.,.,*.,.,.,g.,N"


def combo_line(head, tail, mid_len, k, shape, pos):
    """A line with token `head` at the start of its read bases, token `tail` at their end and mid_len bytes (mostly reference
    matches, rotated by k) in between."""
    h, t = CATALOGUE[head], CATALOGUE[tail]
    assert not h.eats
    rot = MID[k % len(MID):] + MID[:k % len(MID)]
    mid = (rot * (mid_len // len(rot) + 1))[:mid_len - 1] + b"."
    quals = h.quals + quals_of(owners(mid), k) + t.quals
    return shape_line(b"c", pos, h.ref, h.bases + mid + t.bases, quals, shape, k)


HEADS = [i for i, t in enumerate(CATALOGUE) if not t.eats and len(t.bases) <= 64]
TAILS = [i for i, t in enumerate(CATALOGUE) if len(t.bases) <= 64]


class Text(object):
    """A pileup under construction: lines with one kind of line end; tags = {offset: what the line is}."""

    def __init__(self, name, lo, eol=b"\n"):
        self.name, self.lo, self.eol, self.chunks, self.size, self.tags, self.n_lines, self.data = name, lo, eol, [], 0, {}, 0, None

    def add(self, line, tag=None, eol=None):
        off = self.size
        eol = self.eol if eol is None else eol
        self.chunks.append(line + eol)
        self.size += len(line) + len(eol)
        self.n_lines += 1
        if tag is not None:
            self.tags[off] = tag
        return off

    def finish(self):
        self.data = b"".join(self.chunks)
        self.lines = None
        return self


def aligned_filler(size, lo, a):
    """A callable plain line (two variant reads) whose length puts the next line's first byte at address a mod 16."""
    n = (a - size - lo - 15) % 16 + 1
    return b"f" * n + b"\t1\tA\t2\tGg\tIF"


# ---- family i: the ring, routes A / B / C ------------------------------------------------------------------------------------------
def family_i(lo=vc.DEV_LO):
    """Every token x both shapes x the 16 alignments mod 16 of the line's first byte x 4 lengths of the read-base column mod 4
    ('$' in front).  A filler that is a candidate too in front of each, so the waves flush; (token, shape) cycles fastest.  Then
    one-wave files of at most 60 candidates: nothing flushes there, every entry is walked from the wave's LDS list."""
    out = []
    for a4 in range(4):
        b = Text("i%d" % a4, lo)
        for a in range(4 * a4, 4 * a4 + 4):
            for pad in range(4):
                for ti in range(len(CATALOGUE)):
                    for shape in (PLAIN, PARSED):
                        b.add(aligned_filler(b.size, lo, a))
                        b.add(token_line(ti, shape, pad), (ti, shape, a, pad))
        out.append(b.finish())
    b, n = None, 0
    for ti in range(len(CATALOGUE)):
        for shape in (PLAIN, PARSED):
            line = token_line(ti, shape, (ti + n) % 4)
            if b is None or len(b.tags) >= 60 or b.size + len(line) + 1 + lo >= 7 * VS_TILE:
                b = Text("i_lds%d" % len(out), lo)
                out.append(b)
            b.add(line, (ti, shape, (b.size + lo) % 16, (ti + n) % 4))
            n += 1
    return [x.finish() if x.data is None else x for x in out]


def reach(b, n_cu, kw=Q15, verdicts=None):
    """{(tag of the line, kind, source, route)} over the tagged lines of a Text with LF ends, and its [WavePlan]."""
    lines = split_lf(b.data)
    plans = plan(lines, len(b.data), b.lo, n_cu, kw, verdicts)
    seen = set()
    for w in plans:
        for c in w.cands:
            tag = b.tags.get(lines[c.line][0])
            if tag is not None:
                seen.add((tag, c.kind, c.source, c.route))
    return seen, plans


def check_family_i(files, n_cu):
    """Every (token, shape) is walked from the ring's strips out of the wave's LDS list and out of its stretch at least once, and
    at every address mod 4 (in fact at every address mod 16 and every pad); a PLAIN line as a VS_W_PLAIN entry (route A, or C), a
    PARSED one through varscan_parse_lds (B, or C).  Returns the counts per (kind, source)."""
    want = {(ti, shape) for ti in range(len(CATALOGUE)) for shape in (PLAIN, PARSED)}
    lds, stretch, phase, n = set(), set(), set(), {}
    verdicts = {}
    for b in files:
        seen, plans = reach(b, n_cu, Q15, verdicts)
        assert sum(len(w.cands) for w in plans) == b.n_lines, b.name          # fillers are candidates too
        for (ti, shape, a, pad), kind, source, route in seen:
            if route == "shared":
                continue
            n[(kind, source)] = n.get((kind, source), 0) + 1
            if kind == ("plain" if shape == PLAIN else "walk"):
                (lds if source == "lds" else stretch).add((ti, shape))
                phase.add((ti, shape, a, pad))
    assert lds == want, sorted(want - lds)[:5]
    assert stretch == want, sorted(want - stretch)[:5]
    assert phase == {(ti, shape, a, pad) for ti, shape in want for a in range(16) for pad in range(4)}, len(phase)
    return n


# ---- family ii: rounds, route D ------------------------------------------------------------------------------------------------------
def family_ii(lo=vc.DEV_LO):
    """One-wave files (at most 7 tiles: the plan does not depend on the machine) of 40 candidate lines of about 600 bytes, a token at
    the head of each and another at its tail, every line with counts of its own."""
    out = []
    for f in range(4):
        b = Text("ii%d" % f, lo)
        shape = (PLAIN, PARSED)[f % 2]
        for n in range(40):
            k = n + 40 * (f // 2)
            head, tail = HEADS[k % len(HEADS)], TAILS[(7 * k + 3) % len(TAILS)]
            b.add(combo_line(head, tail, 240 + 2 * n, k, shape, 100 + k), (head, tail, shape))
        out.append(b.finish())
    return out


def check_family_ii(files, n_cu):
    n = {}
    heads, tails = set(), set()
    for b in files:
        assert len(b.data) + b.lo < 7 * VS_TILE
        seen, plans = reach(b, n_cu)
        assert len(plans) == 1 and not plans[0].flushes and len(plans[0].cands) == 40 == len(seen) and len(plans[0].groups) == 1
        rounds = sorted(route for _, _, _, route in seen)
        assert set(rounds) == {1, 2, 3} and all(src == "lds" for _, _, src, _ in seen), rounds
        for (head, tail, shape), kind, _, route in seen:
            assert kind == ("plain" if shape == PLAIN else "walk")
            n[(kind, route)] = n.get((kind, route), 0) + 1
            heads.add(head)
            tails.add(tail)
    assert heads == set(HEADS) and len(tails) >= len(TAILS) - 8, (len(heads), len(tails))
    assert all(n.get((kind, r), 0) >= 2 for kind in ("plain", "walk") for r in (1, 2, 3)), n
    return n


# ---- family iii: long lines, route F1 ---------------------------------------------------------------------------------------------------
def family_iii(lo=vc.DEV_LO):
    """Lines of 8 200 to 9 000 bytes and one of 40 000, tokens in the first 64 bytes of the read bases and in the last 64; ends LF,
    CR LF, lone CR and the end of the file; one long line behind a lone-CR line in an earlier tile of the same (only) wave.
    -> [(Text, [(offset, offset of the terminator)] of its long lines)]"""
    out = []

    def long_line(k, length, shape):
        head, tail = HEADS[(3 * k) % len(HEADS)], TAILS[(5 * k + 1) % len(TAILS)]
        mid = length // 2                                       # one more byte in the middle: a read and, nearly always, its quality
        for _ in range(6):
            line = combo_line(head, tail, mid, k, shape, 7 + k)
            if abs(length - len(line)) <= 2:
                break
            mid += (length - len(line)) * 13 // 25
        return line

    def build(name, eol, ks, lengths=None):
        b, at = Text(name, lo, eol), []
        for n, k in enumerate(ks):
            length = lengths[n] if lengths else 8210 + (97 * k) % 780
            line = long_line(k, length, (PLAIN, PARSED)[k % 2])
            assert 8200 <= len(line) <= 9000 or (lengths and 39990 <= len(line) <= 40010), len(line)
            off = b.add(line, ("long", k))
            at.append((off, off + len(line) + len(eol) - 1))
            b.add(vc.CONTROL)
        return b.finish(), at

    out.append(build("iii_lf", vc.LF, range(0, 45)))
    out.append(build("iii_40000", vc.LF, [45, 46], lengths=[40000, 8300]))
    out.append(build("iii_crlf", vc.CRLF, range(47, 59)))
    out.append(build("iii_cr", vc.CR, range(59, 71)))
    # the end of the file without a terminator
    b, at = Text("iii_eof", lo, vc.LF), []
    b.add(vc.CONTROL)
    line = long_line(71, 8640, PLAIN)
    off = b.add(line, ("long", 71), eol=b"")
    at.append((off, off + len(line)))                           # (the virtual terminator behind the file)
    out.append((b.finish(), at))
    # a long line behind a lone-CR line in an earlier tile of the same wave: the wave is in its exact form already
    b, at = Text("iii_exact", lo, vc.LF), []
    b.add(token_line(0, PLAIN), eol=vc.CR)
    while b.size + lo < VS_TILE + 200:
        b.add(vc.filler(61))
    line = long_line(72, 8500, PARSED)
    off = b.add(line, ("long", 72))
    at.append((off, off + len(line)))
    b.add(vc.CONTROL)
    out.append((b.finish(), at))
    return out


def check_family_iii(files, n_cu):
    n = 0
    for b, at in files:
        n_tiles, runs = vc.dealing(len(b.data), b.lo, n_cu)
        for off, e_off in at:
            w = vc.locate(off, e_off, b.lo, runs)
            assert w.long_ and w.carried, (b.name, off, w)
            n += 1
        if b.name == "iii_exact":
            assert len(runs) == 1 and b.data.index(b"\r") + b.lo < VS_TILE <= at[0][0] + b.lo
        if b.name == "iii_eof":
            assert not b.data.endswith((b"\n", b"\r"))
    assert 60 <= n <= 150
    return n


# ---- family iv: saturation, routes E / G and flush() onto the shared list ------------------------------------------------------------
IV_FILLER = b"c\t1\tA\t0\t*\t*"                                  # depth 0: not plain, a candidate, calls nothing


def family_iv_block():
    """The block that family iv repeats: every token whose line is at most 40 bytes in both shapes, PLAIN then PARSED, two fillers
    behind each (a third of the lines are callable); its length is no multiple of 16.  -> (block, [callable lines])"""
    lines, callable_ = [], []
    for ti in range(len(CATALOGUE)):
        both = [token_line(ti, shape) for shape in (PLAIN, PARSED)]
        if max(len(x) for x in both) > 40 - 1 or "Q15" not in CATALOGUE[ti].sets:
            continue
        for x in both:
            lines += [x, IV_FILLER, IV_FILLER]
            callable_.append(x)
    block = b"".join(x + b"\n" for x in lines)
    if len(block) % 16 == 0:
        block += IV_FILLER + b"\n"
        lines.append(IV_FILLER)
    return block, lines, callable_


def family_iv_plan(n_cu, lo=vc.DEV_LO, margin=100000):
    """(block, repetitions, bytes, waves, lower bound of the entries the waves try to put on the shared list, shared_cap, lines).
    Every line of the block is a candidate, so a wave has as many candidates as lines start in its run (counted with dealing());
    a flush takes 73..136 entries and goes to the stretch while it fits, so at most spill_per_wave entries of a wave stay there and
    at most 72 in LDS: all others go to the shared list.  The smallest size, in steps of 4 MiB, at which the sum of those exceeds
    shared_cap by `margin`."""
    block, lines, callable_ = family_iv_block()
    offs = np.cumsum([0] + [len(x) + 1 for x in lines[:-1]])
    for mb in range(16, 400, 4):
        reps = (mb << 20) // len(block)
        nbytes = reps * len(block)
        n_tiles, runs = vc.dealing(nbytes, lo, n_cu)
        shared_cap, spw = caps(nbytes, len(runs))
        start = (np.arange(reps, dtype=np.int64)[:, None] * len(block) + offs[None, :]).ravel() + lo
        tile = (start - 1) // VS_TILE
        first = np.array([a for a, _ in runs], dtype=np.int64)
        per_wave = np.bincount(np.searchsorted(first, tile, side="right") - 1, minlength=len(runs))
        attempts = int(np.maximum(per_wave - spw - 72, 0).sum())
        if attempts >= shared_cap + margin:
            return block, reps, nbytes, len(runs), attempts, shared_cap, lines, callable_
    raise ValueError("family iv: no size below 400 MiB overfills the shared list")


# ---- family v: deep lines, round 4 and routes E / F2 ---------------------------------------------------------------------------------
def family_v_block():
    """64 distinct PLAIN lines of about 2.5 KB (depth about 1 200, a token at the head and another at the tail), then the same 64 in
    the PARSED shape."""
    lines = []
    for shape in (PLAIN, PARSED):
        for n in range(64):
            head, tail = HEADS[(5 * n + 1) % len(HEADS)], TAILS[(3 * n + 2) % len(TAILS)]
            lines.append(combo_line(head, tail, 1200 + n, n, shape, 1000 + n))
    return b"".join(x + b"\n" for x in lines), lines


def family_v_plan(n_cu, lo=vc.DEV_LO, tiles_per_run=16):
    """(block, lines of the block, repetitions, bytes, [WavePlan]): the smallest whole number of blocks at which the shortest run of
    the launch's n_cu * 12 waves has tiles_per_run tiles."""
    block, blines = family_v_block()
    want = min(n_cu * vc.WG_WAVES, vc.MAX_WAVES)
    weight = lambda w: vc.SHARES[(w >> 2) & 3]                   # noqa: E731
    cum = (want // vc.WG_WAVES) * sum(weight(w) for w in range(vc.WG_WAVES)) + sum(weight(w) for w in range(want % vc.WG_WAVES))
    n_tiles = -(-tiles_per_run * cum // min(vc.SHARES))
    reps = -(-(n_tiles * VS_TILE) // len(block))
    nbytes = reps * len(block)
    offs, at = [], 0
    for x in blines:
        offs.append(at)
        at += len(x) + 1
    lines = [(r * len(block) + o, x) for r in range(reps) for o, x in zip(offs, blines)]
    return block, blines, reps, nbytes, plan(lines, nbytes, lo, n_cu, Q15)


def check_family_v(plans, nbytes, lo, n_cu, blines):
    """Every wave walks entries in round 4 and sends entries to the shared list; the list holds whole groups of 64 of which, by
    count, some entries fit the epilogue's 32 KiB and some lie behind them."""
    n_tiles, runs = vc.dealing(nbytes, lo, n_cu)
    assert n_tiles // 4 >= n_cu * vc.WG_WAVES == len(runs) == len(plans) and min(b - a for a, b in runs) >= 15
    to_shared = 0
    for w in plans:
        assert w.count(route=4) >= 1 and w.count(route="shared") >= 1 and w.count(kind="long") == 0, (w.wave, len(w.cands))
        to_shared += w.count(route="shared")
    assert to_shared < plans[0].shared_cap                      # nothing of this family is walked on the spot
    lens = [len(x) + 1 for x in blines]
    e, f2 = epilogue_bounds(to_shared, min(lens), max(lens))
    assert e >= 64 and f2 >= 64, (to_shared, e, f2)
    return dict(waves=len(plans), candidates=sum(len(w.cands) for w in plans), round4=sum(w.count(route=4) for w in plans),
                plain_round4=sum(w.count(route=4, kind="plain") for w in plans), parsed_round4=sum(w.count(route=4, kind="walk") for w in plans),
                shared=to_shared, flush_to_stretch=sum(1 for w in plans for f in w.flushes if f[1] == "stretch"), E_at_least=e, F2_at_least=f2)
