"""The cases of tests/varscan_walk_cases.py checked on the CPU: the constants the routing statement is written for are the ones in
varscan.hip; every token of the catalogue is plain and callable in its PLAIN shape, not plain in its PARSED shape, accepted by the
oracle and yields a record under its parameter sets; the routing statement by hand on small pileups; families i to iii reach the
routes they are named for (outright: their plans do not depend on the machine beyond a handful of CUs), families iv and v for 256 CUs."""
from oracle import varscan_oracle as vo
from tests import varscan_scan_cases as vc
from tests import varscan_walk_cases as wc


def test_the_statement_is_written_for_the_constants_of_the_source():
    c = wc.source_constants()
    assert c["VS_DATA"] and c["VS_STR_WORDS"] and c["VS_STR_PAD"] == wc.VS_STR_PAD == 4 and c["ring_budget"] and c["epi_call"]
    assert wc.VS_DATA == 8320 and wc.VS_STR_WORDS == 256 and wc.RING_STRIP_BYTES == 11424
    assert c["epi_budget"] == wc.EPI_STRIP_BYTES == 32768 and c["rounds"] == wc.ROUNDS == 4
    assert c["cap"] == (wc.CAP_DIV, wc.CAP_FLOOR, wc.CAP_MAX) == (128, 2 * 16384 * 64, 1 << 23)
    assert c["halves"] and c["flush_at"] == 2 and c["stretch_first"] and c["full"] == (True, True) and c["chunks"] and c["lds_first"]
    assert c["guard"] == 2                                       # the size < 2^40 guard: once in varscan_line, once in varscan_core_lds
    # by hand: a 1.3 MB file has the floor of the list, 80 waves, stretches of over 13 000
    assert wc.cand_cap(1300000) == 1300000 // 128 + 2097152 and wc.caps(1300000, 80) == (1053654, 13170)
    assert wc.cand_cap(1 << 40) == 1 << 23
    assert [wc.chunks_of(x, n) for x, n in ((0, 16), (0, 17), (15, 1), (15, 2), (5, 600))] == [1, 2, 1, 2, 38]


def test_every_token_in_both_shapes():
    assert 45 <= len(wc.CATALOGUE) <= 60
    for ti, t in enumerate(wc.CATALOGUE):
        assert t.bases.startswith(b"Gg") and not set(t.quals) & {9, 10, 13} and not set(t.bases) & {9, 10, 13}, t.name
        for name, kw in sorted(wc.PARAM_SETS.items()):
            p = vo.Params(**kw)
            for pad in range(4):
                plain, parsed = wc.token_line(ti, wc.PLAIN, pad), wc.token_line(ti, wc.PARSED, pad)
                v = vc.filter_model(plain, p.min_coverage, p.min_reads2)
                assert v.plain and v.calls and v.window == 32 and v.depth == len(t.quals), (t.name, v)
                assert not vc.filter_model(parsed, p.min_coverage, p.min_reads2).plain, t.name
                assert parsed.count(b"\t") == 6 or len(parsed.split(b"\t")[3]) == 5
                got = [vc.expected(x + b"\n", kw, {}) for x in (plain, parsed)]
                assert got[0][0] != "error" and got[0] == got[1], t.name      # the same columns: the same records
                assert (len(got[0][0]) >= 1) or name not in t.sets, (t.name, name)
                if name in t.sets:                               # at least min_reads2 variant reads: a wrong count changes a record
                    assert any(r[7] + r[8] >= 2 for r in got[0][0]), (t.name, name)
    assert sum(1 for t in wc.CATALOGUE if "Q100" in t.sets) >= 3
    # the indel lengths the 2^40 guard is about, with what the oracle makes of them: everything behind them is inside the indel
    for name in ("len_2p40_less_1", "len_2p40", "len_2p64_plus_1", "len_25_digits"):
        t = [x for x in wc.CATALOGUE if x.name == name][0]
        c = vo.read_counts(t.bases, t.quals, 0)
        assert c.indel == 1 and c.ref[0] + c.ref[1] == 2 and sorted(c.alt) == ["A", "G"], name
    t = wc.CATALOGUE[-1]
    assert t.name == "len_2p64_plus_1_short" and max(len(wc.token_line(len(wc.CATALOGUE) - 1, shape)) for shape in (wc.PLAIN, wc.PARSED)) <= 39
    c = vo.read_counts(t.bases, t.quals, 0)
    assert c.indel == 1 and sorted(c.alt) == ["G"] and t in [wc.CATALOGUE[i] for i in wc.TAILS]


def test_the_routing_statement_by_hand():
    lo = vc.DEV_LO
    # 100 callable plain lines of 14 bytes (LF included) from coordinate 21 on, in one tile: one wave.  Terminators at 20 (the
    # virtual one), 34 + 14 i, and 1421 (virtual); lane L owns those in [64 L, 64 L + 64): lane 0 four, lanes 1..21 four or five
    # (twelve of them five), lane 22 the last line's and the virtual one, which start no line.  So phase B takes five rounds of
    # 22, 22, 22, 22 and 12 lines; the list reaches 73 with the fourth: one flush of 88 to the stretch, 12 stay in LDS, which the
    # tail loop reads first
    line = b"f\t1\tA\t2\tGg\tIF"
    data = (line + b"\n") * 100
    w, = wc.plan(wc.split_lf(data), len(data), lo, 256, wc.Q15)
    assert w.flushes == [(88, "stretch")] and w.atomics == [] and [len(g) for g in w.groups] == [64, 36]
    assert [c.source for c in w.cands] == ["lds"] * 12 + ["stretch"] * 88 and {c.route for c in w.cands} == {1} and {c.kind for c in w.cands} == {"plain"}
    # lane-minor: the first round holds the first line of every 64 bytes
    first_round = [c.line for c in w.cands[12:12 + 22]]
    assert first_round == sorted(first_round) and first_round[:4] == [0, 4, 8, 13] and w.cands[12 + 22].line == 1
    # a line that runs over two tiles is VS_W_LONG, first of its tile; one that ends in the next tile is carried and known-end
    long_line = vc.probe(b"c", 1, b"A", b"9000", b"Gg" + b"." * 8998, b"I" * 9000)
    mid_line = vc.probe(b"c", 2, b"A", b"3000", b"Gg" + b"." * 2998, b"I" * 3000)
    data = line + b"\n" + long_line + b"\n" + line + b"\n" + mid_line + b"\n"
    w, = wc.plan(wc.split_lf(data), len(data), lo, 256, wc.Q15)
    assert [(c.line, c.kind, c.route) for c in w.cands] == [(0, "plain", 1), (1, "long", "shared"), (2, "plain", 1), (3, "plain", 1)] and w.atomics == [1]
    assert wc.epilogue_fit([(lo + len(line) + 1, len(long_line) + 1, True)]) == ["F1"]
    # packing: seven lines of 3 900 bytes in a one-wave file: two per round (three need 11 700 > 11 424 bytes), the seventh in round 4
    big = vc.probe(b"c", 3, b"A", b"1940", b"Gg" + b"." * 1945, b"I" * 1940)
    data = (big + b"\n") * 7
    w, = wc.plan(wc.split_lf(data), len(data), lo, 256, wc.Q15)
    assert [c.route for c in w.cands] == [1, 1, 2, 2, 3, 3, 4] and w.atomics == [] and len(big) == 3899
    # the epilogue's 32 KiB: five fit (376 chunks each), the sixth lies behind them; bounds by count say the same for whole groups
    assert wc.epilogue_fit([(lo, 6000, False)] * 7) == ["E"] * 5 + ["F2"] * 2
    assert wc.epilogue_bounds(64, 6000, 6000) == (5, 59) and wc.epilogue_bounds(63, 6000, 6000) == (0, 0)
    # a stretch that is full sends the flush to the shared list
    n_tiles, runs = vc.dealing(50 << 20, lo, 256)
    assert len(runs) == 3072 and wc.caps(50 << 20, 3072) == ((2097152 + 409600) // 2, ((2097152 + 409600) // 2) // 3072)


def test_family_i_reaches_the_lds_list_and_the_stretch():
    files = wc.family_i()
    assert 300 * 1024 <= sum(len(b.data) for b in files) <= 700 * 1024
    for n_cu in (256, 304, 8):
        n = wc.check_family_i(files, n_cu)
        assert min(n.values()) > 100 and set(n) == {("plain", "lds"), ("plain", "stretch"), ("walk", "lds"), ("walk", "stretch")}, n
    # the device forms and the file form differ in the line addresses mod 16 only
    n = wc.check_family_i(wc.family_i(vc.FILE_LO), 256)
    assert min(n.values()) > 100


def test_family_ii_reaches_rounds_one_to_three():
    for lo in (vc.DEV_LO, vc.FILE_LO):
        for n_cu in (256, 1):
            wc.check_family_ii(wc.family_ii(lo), n_cu)


def test_family_iii_lines_have_no_known_end():
    for lo in (vc.DEV_LO, vc.FILE_LO):
        files = wc.family_iii(lo)
        assert wc.check_family_iii(files, 256) == wc.check_family_iii(files, 8)
        assert {b.eol for b, _ in files} == {vc.LF, vc.CRLF, vc.CR} and max(len(x) for b, _ in files for x in b.chunks) > 39000
        for b, at in files:                                      # the oracle accepts every file
            assert vc.expected(b.data, wc.Q15, {})[0] != "error", b.name


def test_family_iv_overfills_the_shared_list_for_256_cus():
    block, reps, nbytes, waves, attempts, shared_cap, lines, callable_ = wc.family_iv_plan(256)
    assert len(block) % 16 != 0 and nbytes == reps * len(block) and waves == 3072 and attempts >= shared_cap + 100000
    assert 4 * len(callable_) >= len(lines) and all(len(x) <= 40 for x in callable_) and nbytes < 120 << 20
    assert wc.token_line(len(wc.CATALOGUE) - 1, wc.PLAIN) in callable_ and wc.token_line(len(wc.CATALOGUE) - 1, wc.PARSED) in callable_
    p = vo.Params(**wc.Q15)
    shapes = [vc.filter_model(x, p.min_coverage, p.min_reads2) for x in callable_]
    assert sum(1 for v in shapes if v.plain and v.calls) == sum(1 for v in shapes if not v.plain) == len(callable_) // 2 >= 20
    v = vc.filter_model(wc.IV_FILLER, p.min_coverage, p.min_reads2)
    assert not v.plain and not v.dropped                         # depth 0: the scan cannot vouch for it, so it is a candidate
    recs, n_lines = vc.expected(block, wc.Q15, {})
    assert n_lines == len(lines) and {r[0] for r in recs} == {block.index(x + b"\n") for x in callable_}
    assert vc.expected(wc.IV_FILLER + b"\n", wc.Q0, {}) == ([], 1)
    # the statement on one repetition of the block: every line is a candidate
    w, = wc.plan(wc.split_lf(block), len(block), vc.DEV_LO, 256, wc.Q15)
    assert len(w.cands) == len(lines)


def test_family_v_reaches_round_four_and_the_epilogue_for_256_cus():
    block, blines, reps, nbytes, plans = wc.family_v_plan(256)
    n = wc.check_family_v(plans, nbytes, vc.DEV_LO, 256, blines)
    assert nbytes < 340 << 20 and len(blines) == 128 and all(2300 <= len(x) <= 2800 for x in blines), (nbytes, min(map(len, blines)), max(map(len, blines)))
    assert n["plain_round4"] > 1000 and n["parsed_round4"] > 1000 and n["shared"] > 20000, n
    p = vo.Params(**wc.Q15)
    for i, x in enumerate(blines):
        v = vc.filter_model(x, p.min_coverage, p.min_reads2)
        assert (v.plain and v.calls and 1100 <= v.depth <= 1400) if i < 64 else not v.plain, i
    recs, n_lines = vc.expected(block, wc.Q15, {})
    assert n_lines == 128 and len({r[0] for r in recs}) == 128 and len({r[1:] for r in recs}) >= 64       # every line with counts of its own
