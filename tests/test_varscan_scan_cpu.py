"""The cases of tests/varscan_scan_cases.py checked on the CPU: the constants the Python statements are written for are the ones
in varscan.hip; the line filter of k_varscan_scan, as designed (filter_model), drops no line the oracle calls anything on; every
case of every family reaches the branch it is named for (check_reach: no case is skipped, a generator that cannot build a cell
raises); fillers and controls yield no record."""
import random

import pytest

from oracle import fuzz
from oracle import threshold_cases as tc
from oracle import varscan_oracle as vo
from tests import varscan_scan_cases as vc


@pytest.fixture(scope="module")
def families():
    return vc.all_families()


PARAM_SETS = [vc.D2, vc.R1, vc.R0, vc.V1] + [vc.cov(d) for d in sorted(vc.DEPTH_OF_DIGITS.values())] + [vc.cov(2), dict(vo.PIPELINE_DEFAULTS)]


def test_the_statements_are_written_for_the_constants_of_the_source():
    c = vc.source_constants()
    assert (c["VS_TILE"], c["VS_RING"], c["VS_PAD"], c["VS_CAND_LOCAL"], c["WG_WAVES"], c["SHARES"], c["MAX_WAVES"]) == \
        (vc.VS_TILE, vc.VS_RING, vc.VS_PAD, vc.VS_CAND_LOCAL, vc.WG_WAVES, vc.SHARES, vc.MAX_WAVES) == (4096, 8192, 64, 136, 12, (140, 100, 66, 66), 16384)
    assert c["tiles"] and c["want"] and c["share_of"]
    # the dealing by hand: 33 tiles -> 8 waves, weights 140 x 4, 100 x 4 of 960
    n_tiles, runs = vc.dealing(33 * 4096 - 121, 21, 256)
    assert n_tiles == 33 and runs == [(0, 4), (4, 9), (9, 14), (14, 19), (19, 22), (22, 26), (26, 29), (29, 33)]
    assert vc.dealing(100, 16, 256) == (1, [(0, 1)]) and vc.dealing(11 * 4096 - 121, 21, 256)[1] == [(0, 5), (5, 11)]
    n_tiles, runs = vc.dealing(1 << 30, 16, 256)                  # a full launch: 3072 waves, every tile dealt once
    assert len(runs) == 3072 and runs[0][0] == 0 and runs[-1][1] == n_tiles and all(a[1] == b[0] for a, b in zip(runs, runs[1:]))
    assert runs[0][1] - runs[0][0] > 2 * (runs[11][1] - runs[11][0]) - 2


def test_the_filter_as_designed_drops_nothing_the_oracle_calls(families):
    """About 52 000 distinct lines (seeded fuzz pileups, adversarial read-base text, every probe) under every parameter set used by
    the GPU tests, about half a minute: a line with a record is never "dropped"."""
    lines = set()
    for seed in range(1, 7):
        lines.update(fuzz.varscan_pileup(seed, 5000).split(b"\n"))
        lines.update(fuzz.varscan_pileup(100 + seed, 400, depths=(150, 300, 8, 1500)).split(b"\n"))
        lines.update(fuzz.varscan_adversarial(seed, 2500).split(b"\n"))
    for fam in families.values():
        for b in fam:
            lines.update(p.line for p in b.probes if len(p.line) < 3000)
    lines.discard(b"")
    lines = sorted(ln for ln in lines if vc._valid(ln) and b"\r" not in ln)
    assert len(lines) > 40000
    n_rec = n_drop = 0
    for kw in PARAM_SETS:
        p = vo.Params(**kw)
        for ln in lines:
            v = vc.filter_model(ln, p.min_coverage, p.min_reads2)
            n_drop += v.dropped
            if tc.varscan_records(ln, p):
                n_rec += 1
                assert not v.dropped, (kw, ln, v)
    assert n_rec > 5000 and n_drop > 50000                       # both sides of the filter are well populated


def test_every_case_is_what_its_name_says(families):
    n = {}
    for fam, files in families.items():
        fates = {}
        for b in files:
            assert b.probes, b.name
            assert 40 * 1024 <= len(b.data) <= 140 * 1024, (b.name, len(b.data))
            for p in b.probes:
                fate = vc.check_reach(b, p)
                fates[fate] = fates.get(fate, 0) + 1
        n[fam] = fates
    assert set(n) == {"A", "B", "C", "D", "E_crlf", "E_cr", "F"}
    assert n["A"]["plain"] > 2400 and n["A"]["walk"] > 100 and n["F"] == {"plain": 6, "long": 2}
    for fam in ("B", "E_crlf", "E_cr"):
        assert n[fam]["plain"] > 600 and n[fam]["walk"] >= 2


def test_family_a_takes_every_value_of_the_fourth_tab(families):
    r3 = set()
    for b in families["A"]:
        for p in b.probes:
            r3.add(p.line.replace(b"\t", b"x", 3).index(b"\t"))
    assert r3 >= set(range(8, 67))
    lengths = {len(p.line) for b in families["A"] if b.name == "A_short" for p in b.probes}
    assert lengths == set(range(11, 65))


def test_family_b_has_every_cell(families):
    for fam in ("B", "E_crlf", "E_cr"):
        seen = set()
        for b in [x for x in families[fam] if x.name.startswith("B")]:
            n_tiles, runs = vc.dealing(len(b.data), b.lo, 256)
            kinds = vc._edge_kinds(n_tiles, runs)
            for p in b.probes:
                x = p.off + b.lo
                e = (x + vc.VS_TILE // 2) // vc.VS_TILE
                seen.add((kinds[e], x - e * vc.VS_TILE, len(p.line) > 64))
        for kind in ("in_odd", "in_even", "first", "last"):
            assert {d for k, d, _ in seen if k == kind} >= set(range(-70, 7)), (fam, kind)
            assert {d for k, d, long_ in seen if k == kind and not long_} >= set(range(-40, 7)), (fam, kind)
        assert {d for _, d, _ in seen} >= set(range(-70, 128)), fam
        r63 = {(kinds_, d) for kinds_, d, long_ in seen if long_ and d in (-64, -63, -62, -1, 0)}
        assert len(r63) >= 10


def test_fillers_and_controls_yield_no_record(families):
    shapes = {vc.CONTROL}
    for fam in families.values():
        for b in fam:
            shapes |= b.fillers
    assert len(shapes) > 60
    for kw in PARAM_SETS + [dict(min_coverage=1, min_reads2=0, min_var_freq=0.0, min_avg_qual=0)]:
        p = vo.Params(**kw)
        for ln in shapes:
            assert vc._valid(ln) and tc.varscan_records(ln, p) == [] and vc.filter_model(ln, p.min_coverage, p.min_reads2).plain, ln
    for seed in range(20):                                      # ... and fillers of any length
        n = random.Random(seed).randint(11, 9000)
        assert len(vc.filler(n)) == n and tc.varscan_records(vc.filler(n), vo.Params(min_coverage=1, min_reads2=0, min_var_freq=0.0)) == []
    for n in range(11, 400):
        assert len(vc.filler(n)) == n and vc.filter_model(vc.filler(n), 1, 0).dropped


def test_family_g_is_placed_on_the_wraps():
    """The plan of family G for 256 and 304 CUs: every run long enough, one probe per chosen run, at least eight on each wrap."""
    for n_cu in (256, 304, 64):
        fl, nbytes, n_tiles, runs, probes, kinds = vc.family_g_plan(n_cu)
        assert nbytes % len(fl) == 0 and len(runs) == 12 * n_cu and kinds["letters"] >= 8 and kinds["tabs"] >= 8 and kinds["neither"] >= 8
        assert len({vc.locate(o, o + len(ln), vc.DEV_LO, runs).wave for o, ln in probes}) == len(probes) >= 24
        assert all(o % len(fl) == 0 for o, _ in probes)
    assert nbytes // (1 << 20) < 1200
