"""merge_vcfs on the device in bounded memory (snpgpu_merge_vcf_files_opts under a budget: a key pass, then one reading of the input
per range of sites) against the reference's own snpma files, the Python statement of the merge rule (merge_vcfs.merge_texts) and the
single pass on the same input.  The budgets come from the plan: the smallest one that holds the wanted number of sites a round
(merge_bounded_cases.budget_for), and the merge has to report that same plan.

Between the largest bounded plan (n_sites - 1 sites a round) and the single pass sites_per_round takes no value: the single pass
needs the record bound's room, a step above, and its one round holds every site.  The cases `n_sites` and `n_sites + 1` therefore
both land on the smallest budget of the single pass, and have to read the input exactly once."""
import os

import pytest

import merge_bounded_cases as cases
import test_gpu_merge_vcfs as base

pytestmark = pytest.mark.gpu

TILE, WINDOW, STEP = base.TILE, base.WINDOW, base.STEP
OWN = b"##snpgpu_mergeVersion=x\n"
E_NOMEM, E_UNSUPPORTED = -3, -5


@pytest.fixture(scope="module")
def dev():
    from gpu_util import get_device
    return get_device()


def _single(dev, tmp_path, paths):
    out = str(tmp_path / "single.vcf")
    stats = dev.merge_vcf_files(paths, out, OWN)
    assert stats["input_passes"] == 1 and stats["site_rounds"] == 0
    return stats, open(out, "rb").read()


def _bounded(dev, tmp_path, paths, single_stats, single_text, want):
    """The merge under the smallest budget that holds `want` sites a round: the same bytes and totals as the single pass, and the plan."""
    n_sites = single_stats["sites"]
    budget, plan = cases.budget_for(paths, n_sites, want)
    out = str(tmp_path / ("bounded_%d.vcf" % want))
    stats = dev.merge_vcf_files(paths, out, OWN, device_bytes=budget)
    print("sites a round", want, "budget", budget, {k: stats[k] for k in ("input_passes", "site_rounds", "sites_per_round", "device_bytes", "rounds", "host_lines")})
    got = open(out, "rb").read()
    if got != single_text:
        g, w = got.split(b"\n"), single_text.split(b"\n")
        assert len(g) == len(w), (want, len(g), len(w))
        for i, (a, b) in enumerate(zip(g, w)):
            assert a == b, (want, i, a[:300], b[:300])
    for key in ("input_passes", "site_rounds", "sites_per_round", "device_bytes"):
        assert stats[key] == plan[key], (key, stats[key], plan)
    if want >= n_sites:
        assert stats["input_passes"] == 1                        # the unchanged route
    else:
        assert stats["input_passes"] == 1 + -(-n_sites // want) and stats["rounds"] >= stats["site_rounds"]
    for key in ("columns", "sites", "cells", "host_lines", "bytes"):
        assert stats[key] == single_stats[key], (key, stats[key], single_stats[key])
    assert not [name for name in os.listdir(str(tmp_path)) if ".snpgpu-merge." in name]      # the temporary name is gone
    return stats


# ---- 1. the bundled tree ----------------------------------------------------------------------------------------------------------
def test_lambda_in_site_rounds(dev, tmp_path):
    mv = base._mv()
    dirs, _ = base._lambda_dirs(tmp_path)
    for vcf, name in (("consensus.vcf", "snpma"), ("consensus_preserved.vcf", "snpma_preserved")):
        paths = [os.path.join(d, vcf) for d in mv.column_order(dirs)]
        work = tmp_path / name
        work.mkdir()
        single, text = _single(dev, work, paths)
        assert base._body(text) == base._body(base._fixture("lambdaVirus_" + name))
        n = single["sites"]
        assert n > 8
        for want in (1, 7, n - 1):
            _bounded(dev, work, paths, single, text, want)


# ---- 2. seeded trees --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_columns", [1, 2, 63, 64, 65, 130])
def test_seeded_trees_in_site_rounds(dev, tmp_path, n_columns):
    paths, texts = cases.tree(tmp_path / "tree", 200 + n_columns, n_columns)
    want_text = base._mv().merge_texts(texts, [OWN.rstrip(b"\n")])
    single, text = _single(dev, tmp_path, paths)
    assert text == want_text
    n = single["sites"]
    assert n == len(cases.rows_of(want_text)) and 10 < n < 60
    chroms = {r.split(b"\t")[0] for r in cases.rows_of(want_text)}
    assert chroms == set(cases.CONTIGS) or n_columns == 1
    for want in (1, 2, 5, n - 1, n, n + 1):
        _bounded(dev, tmp_path, paths, single, text, want)


# ---- 3. round edges ---------------------------------------------------------------------------------------------------------------
def test_round_edges(dev, tmp_path):
    last = 4
    after = {last: [cases.plain_row(b"ctg1", 1000),              # a site only the last column carries
                    cases.plain_row(b"late", 5), cases.plain_row(b"late", 9)]}      # a contig that appears in the last column first
    paths, texts = cases.tree(tmp_path / "tree", 31, 5, after=after, header_only=(2,))
    want_text = base._mv().merge_texts(texts, [OWN.rstrip(b"\n")])
    single, text = _single(dev, tmp_path, paths)
    assert text == want_text
    rows = [r.split(b"\t") for r in cases.rows_of(want_text)]
    n = len(rows)
    heads = [l for l in want_text.split(b"\n") if l.startswith(b"##contig=")]
    assert heads[-1] == b"##contig=<ID=late>" and [r[0] for r in rows[-2:]] == [b"late", b"late"] and rows[-3][:2] == [b"ctg1", b"1000"]
    assert [c != b".:.:.:.:.:.:.:.:." for c in rows[-3][9:]] == [False] * last + [True]
    assert all(r[9 + 2] == b".:.:.:.:.:.:.:.:." for r in rows)    # the file with a header only: a column of absent cells
    first_contig = sum(1 for r in rows if r[0] == rows[0][0])      # a round boundary exactly between two contigs
    assert 1 < first_contig < n - 1 and rows[first_contig][0] != rows[0][0]
    for want in sorted({first_contig, 2, 5}):
        # (sites a round 2: the two sites of `late` are the last round, and column 0 — two contigs only — has no record in many rounds)
        _bounded(dev, tmp_path, paths, single, text, want)
    # a list entry that cannot be read ends both forms alike, before anything is written
    budget, _ = cases.budget_for(paths, n, 5)
    for entry in ("", str(tmp_path / "missing.vcf")):
        broken = paths[:3] + [entry] + paths[3:]
        a = cases.raw_merge(dev, broken, str(tmp_path / "never_a.vcf"))
        b = cases.raw_merge(dev, broken, str(tmp_path / "never_b.vcf"), budget)
        assert a[0] == b[0] != 0 and a[1] == b[1] and a[2]["bad_file"] == b[2]["bad_file"] == 3
        assert not os.path.exists(str(tmp_path / "never_a.vcf")) and not os.path.exists(str(tmp_path / "never_b.vcf"))


# ---- 4. lines the host parses -----------------------------------------------------------------------------------------------------
def test_host_parsed_lines_in_the_first_a_middle_and_the_last_round(dev, tmp_path):
    ten = b"1:4000000000:0:4000000000:0:0:7:8:PASS"               # a count of ten digits
    long_a, long_b, long_c = b"A" * 5000, b"B" * WINDOW, b"C" * 4200      # lines of SNPGPU_VCF_LINE_WINDOW bytes or more
    ctg2 = cases.CONTIGS[1]
    before = {0: [cases.plain_row(long_a, 7), cases.plain_row(ctg2, 1, cell=ten), cases.plain_row(ctg2, 2, ns=b"NS=3")]}
    after = {0: [cases.plain_row(long_b, 7), cases.plain_row(b"z|3", 20, cell=ten), cases.plain_row(b"z|3", 22, ns=b"NS=3")],
             1: [cases.plain_row(b"ctg1", 999998, cell=ten), cases.plain_row(b"ctg1", 999999, ns=b"NS=3")],
             3: [cases.plain_row(long_c, 7)]}
    paths, texts = cases.tree(tmp_path / "tree", 41, 4, before=before, after=after)
    want_text = base._mv().merge_texts(texts, [OWN.rstrip(b"\n")])
    single, text = _single(dev, tmp_path, paths)
    assert text == want_text and single["host_lines"] == 9
    rows = [r.split(b"\t")[:2] for r in cases.rows_of(want_text)]
    n = len(rows)
    placed = (("long", [[long_a, b"7"], [long_b, b"7"], [long_c, b"7"]]),
              ("ten digits", [[ctg2, b"1"], [b"z|3", b"20"], [b"ctg1", b"999998"]]),
              ("NS", [[ctg2, b"2"], [b"z|3", b"22"], [b"ctg1", b"999999"]]))
    per_round = 5 if n % 5 == 0 or n % 5 >= 3 else 4              # (the last three sites are the last three lines above: one round)
    n_rounds = -(-n // per_round)
    where = {kind: [rows.index(site) // per_round for site in sites] for kind, sites in placed}
    print(n, "sites in rounds of", per_round, where)
    for kind, (first, middle, final) in where.items():
        assert first == 0 and 0 < middle < n_rounds - 1 and final == n_rounds - 1, (kind, first, middle, final, n_rounds)
    for want in (per_round, 1):
        stats = _bounded(dev, tmp_path, paths, single, text, want)
        assert stats["host_lines"] == 9 and stats["input_passes"] > 4      # once a line, not once a reading


# ---- 5. tile, part and piece edges of the key kernel ------------------------------------------------------------------------------
def _padded(tmp_path, build, targets):
    """build(dir, pad) -> (paths, texts).  targets: {column: byte offset at which a line terminator has to lie}: the column gets a header
    line that moves the nearest terminator in front of the offset onto it."""
    _, texts = build(tmp_path / "measure", None)
    pad = {}
    for c, target in targets.items():
        at = texts[c].rindex(b"\n", 0, target - 5)
        assert at > texts[c].index(b"\n#CHROM") + 200             # a data line's terminator
        pad[c] = b"##p=" + b"x" * (target - at - 5)
    paths, texts = build(tmp_path / "tree", pad)
    for c, target in targets.items():
        assert texts[c][target:target + 1] == b"\n" and texts[c][target - 1:target] != b"\n", (c, target)
    return paths, texts


def test_terminators_on_tile_edges(dev, tmp_path):
    """A terminator as the last and as the first byte of a 16 KiB tile, at the first tile edge and at 14 tiles, which is where the key
    pass starts a launch of its own while a batch holds its fewest keys (4096: budgets as small as these)."""
    targets = {0: TILE - 1, 1: TILE, 2: 14 * TILE - 1, 3: 14 * TILE}
    paths, texts = _padded(tmp_path, lambda d, pad: cases.tree(d, 51, 4, n_positions=2000, pad=pad), targets)
    assert all(len(t) > 14 * TILE + 1000 for t in texts)
    want_text = base._mv().merge_texts(texts, [OWN.rstrip(b"\n")])
    single, text = _single(dev, tmp_path, paths)
    assert text == want_text and single["host_lines"] == 0
    n = single["sites"]
    stats = _bounded(dev, tmp_path, paths, single, text, -(-n // 3))
    assert stats["site_rounds"] == 3
    _bounded(dev, tmp_path, paths, single, text, -(-n // 40))     # a smaller budget still: the key pass in more batches


def test_terminators_on_the_edges_of_a_streamed_piece(dev, tmp_path):
    """Two columns longer than a streamed piece: a terminator as the last byte the first piece owns, and as the first byte of the
    second.  (The single pass over such files is held against the Python rule in test_gpu_merge_vcfs.)"""
    def build(d, pad):
        paths, texts = [], []
        for c in range(2):
            head = base._header(b"smp%03d" % c)
            if pad:
                head = head.replace(b"##source=test\n", b"##source=test\n" + pad[c] + b"\n")
            body = b"".join(cases.plain_row(b"ctg%d" % (1 + pos % 2), 7 * pos + c * (pos % 3), ref=b"ACGT"[pos % 4:pos % 4 + 1], alt=b"N",
                                            cell=b"1:%d:0:%d:0:0:%d:%d:PASS" % (pos, pos % 977, pos % 13, pos % 7)) + b"\n" for pos in range(1, 200000))
            p = d / ("d%d" % c)
            p.mkdir(parents=True)
            (p / "consensus.vcf").write_bytes(head + body)
            paths.append(str(p / "consensus.vcf"))
            texts.append(head + body)
        return paths, texts
    paths, texts = _padded(tmp_path, build, {0: STEP - 1, 1: STEP})
    assert all(STEP + 2 * TILE < len(t) < 2 * STEP for t in texts)
    single, text = _single(dev, tmp_path, paths)
    n = single["sites"]
    assert single["host_lines"] == 0 and n > 200000 and single["cells"] == 2 * 199999
    stats = _bounded(dev, tmp_path, paths, single, text, -(-n // 3))
    assert stats["site_rounds"] == 3


# ---- 6. errors --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["outside the rule", "a position twice", "different REF"])
def test_errors_equal_the_single_pass_and_leave_no_file(dev, tmp_path, case):
    after = {}
    if case == "a position twice":                              # (ctg1 is the last contig and 5000 its last position: the last round)
        after = {1: [cases.plain_row(b"ctg1", 5000), cases.plain_row(b"ctg1", 5000)]}
    elif case == "different REF":
        after = {1: [cases.plain_row(b"ctg1", 5000, ref=b"A")], 2: [cases.plain_row(b"ctg1", 5000, ref=b"C")]}
    paths, texts = cases.tree(tmp_path / "tree", 61, 3, after=after)
    if case == "outside the rule":
        with open(paths[1], "ab") as f:
            f.write(b"ctg1\t5\t.\tAC\tG\t.\tPASS\tNS=1\t" + base.FORMAT + b"\t1:4:0:4:0:0:2:2:PASS\n")      # a REF of two bases
    n = len({tuple(r.split(b"\t")[:2]) for t in texts for r in cases.rows_of(t)})
    budget, plan = cases.budget_for(paths, n, 5)
    assert plan["site_rounds"] >= 3
    work = tmp_path / "out"
    work.mkdir()
    fresh, kept = str(work / "fresh.vcf"), str(work / "kept.vcf")
    with open(kept, "wb") as f:
        f.write(b"what was here before\n")
    want = cases.raw_merge(dev, paths, str(tmp_path / "single.vcf"))
    assert want[0] == E_UNSUPPORTED and not os.path.exists(str(tmp_path / "single.vcf"))
    for out in (fresh, kept):
        got = cases.raw_merge(dev, paths, out, budget)
        print(case, got[0], got[1], got[2]["bad_file"], got[2]["bad_offset"])
        assert got[0] == want[0] and got[1] == want[1]
        assert got[2]["bad_file"] == want[2]["bad_file"] and got[2]["bad_offset"] == want[2]["bad_offset"]
    if case == "outside the rule":
        assert want[2]["bad_file"] == 1 and want[2]["bad_offset"] == len(texts[1]) and "byte %d" % len(texts[1]) in want[1]
    elif case == "a position twice":
        assert want[2]["bad_file"] == 1 and "comes twice" in want[1] and want[2]["bad_offset"] in (len(texts[1]) - len(after[1][1]) - 1, len(texts[1]) - 2 * len(after[1][1]) - 2)
    else:
        assert "different REF" in want[1]
    assert not os.path.exists(fresh) and open(kept, "rb").read() == b"what was here before\n" and os.listdir(str(work)) == ["kept.vcf"]


# ---- 7. a budget below one site -----------------------------------------------------------------------------------------------------
def test_a_budget_below_one_site_writes_nothing(dev, tmp_path):
    import re
    from snp_pipeline_amd.device import Device, SnpGpuError
    paths, texts = cases.tree(tmp_path / "tree", 71, 3)
    n = len({tuple(r.split(b"\t")[:2]) for t in texts for r in cases.rows_of(t)})
    smallest, _ = cases.budget_for(paths, n, 1)
    with pytest.raises(SnpGpuError) as err:
        Device.merge_plan(3, n, sum(len(t) for t in texts), smallest - 1)
    needed = int(re.search(r"needs (\d+) bytes", str(err.value)).group(1))
    assert needed == smallest
    work = tmp_path / "out"
    work.mkdir()
    rc, message, stats = cases.raw_merge(dev, paths, str(work / "never.vcf"), smallest - 1)
    print(rc, message)
    assert rc == E_NOMEM and "needs %d bytes" % needed in message and os.listdir(str(work)) == []
    with pytest.raises(SnpGpuError):
        dev.merge_vcf_files(paths, str(work / "never.vcf"), OWN, device_bytes=1)
    assert os.listdir(str(work)) == []


# ---- 8. the commands --------------------------------------------------------------------------------------------------------------
def _run_logged(line, capsys):
    from snp_pipeline_amd import cfsan_snp_pipeline as cli
    args = cli.parse_argument_list([w.replace("\x00", " ") for w in line.split()])
    args.verbose = 1
    capsys.readouterr()
    assert cli.run_command_from_args(args) == 0
    return capsys.readouterr().out


def test_merge_vcfs_command_under_a_budget(dev, tmp_path, monkeypatch, capsys):
    mv = base._mv()
    dirs, listing = base._lambda_dirs(tmp_path)
    monkeypatch.setenv("SNPGPU_VCF_MERGER", "device")
    monkeypatch.delenv("BcftoolsMerge_ExtraParams", raising=False)
    monkeypatch.delenv("SNPGPU_MERGE_DEVICE_BYTES", raising=False)
    for vcf, name in (("consensus.vcf", "snpma"), ("consensus_preserved.vcf", "snpma_preserved")):
        paths = [os.path.join(d, vcf) for d in mv.column_order(dirs)]
        plain, bounded, by_env = (str(tmp_path / (name + tail)) for tail in (".vcf", ".bounded.vcf", ".env.vcf"))
        log = _run_logged("merge_vcfs -f -n %s -o %s %s" % (vcf, plain, listing), capsys)
        assert "# device route, single pass, 1 reading of the input" in log
        n = mv.merge_sample_dirs.last_stats["sites"]
        budget, plan = cases.budget_for(paths, n, 7)
        log = _run_logged("merge_vcfs -f -n %s -o %s --mergeDeviceBytes %d %s" % (vcf, bounded, budget, listing), capsys)
        assert "# device route, %d site rounds of 7 sites, %d readings of the input" % (plan["site_rounds"], plan["input_passes"]) in log
        monkeypatch.setenv("SNPGPU_MERGE_DEVICE_BYTES", str(budget))
        log = _run_logged("merge_vcfs -f -n %s -o %s %s" % (vcf, by_env, listing), capsys)
        assert "site rounds of 7 sites" in log
        monkeypatch.delenv("SNPGPU_MERGE_DEVICE_BYTES")
        body = base._body(open(plain, "rb").read())
        assert base._body(open(bounded, "rb").read()) == body == base._body(open(by_env, "rb").read()) == base._body(base._fixture("lambdaVirus_" + name))
    with pytest.raises(SystemExit):
        _run_logged("merge_vcfs -f -o %s --mergeDeviceBytes some %s" % (str(tmp_path / "no.vcf"), listing), capsys)
    assert not os.path.exists(str(tmp_path / "no.vcf"))


def test_hot_path_batch_merge_vcfs_under_a_budget(dev, tmp_path, monkeypatch, capsys):
    import test_gpu_pipeline as tp
    mv = base._mv()
    ref_path, dirs, dirs_file, piles = tp._outbreak_tree(tmp_path)
    monkeypatch.setenv("VarscanMpileup2snp_ExtraParams", tp.VARSCAN_EXTRA)
    monkeypatch.setenv("SNPGPU_VCF_MERGER", "device")
    monkeypatch.delenv("SNPGPU_MERGE_DEVICE_BYTES", raising=False)
    monkeypatch.chdir(tmp_path)
    line = ("hot_path_batch -f --mergeVcfs %s %s --filterRegionsExtraParams=%s --callConsensusExtraParams=%s"
            % (dirs_file, ref_path, "--edge_length 100 --window_size 1000 125 15 --max_snp 3 2 1 --mode all".replace(" ", "\x00"),
               tp.CONSENSUS_EXTRA.replace(" ", "\x00")))
    log = _run_logged(line, capsys)
    assert log.count("# device route, single pass") == 2
    want = {out: open(str(tmp_path / out), "rb").read() for out in ("snpma.vcf", "snpma_preserved.vcf")}
    budgets = []
    for out, vcf, listing in (("snpma.vcf", "consensus.vcf", dirs_file + ".OrigVCF.filtered"), ("snpma_preserved.vcf", "consensus_preserved.vcf", dirs_file + ".PresVCF.filtered")):
        listed = [d for d in open(listing).read().split("\n") if d]
        paths = [os.path.join(d, vcf) for d in mv.column_order(listed)]
        budgets.append(cases.budget_for(paths, len(cases.rows_of(want[out])), 9)[0])
        os.remove(str(tmp_path / out))
    log = _run_logged(line + " --mergeDeviceBytes %d" % min(budgets), capsys)
    assert log.count("site rounds of ") == 2 and "site rounds of 9 sites" in log
    for out in want:
        assert base._body(open(str(tmp_path / out), "rb").read()) == base._body(want[out]) and want[out].count(b"\n") > 30, out
    with pytest.raises(SystemExit):
        _run_logged(line + " --mergeDeviceBytes -4", capsys)
