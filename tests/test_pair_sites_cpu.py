"""The statements of tests/pair_sites_cases.py pinned on the reference's own tables, the host writer of the sites files, and the
options of ``distance`` / ``hot_path_batch`` — nothing here needs a GPU."""
import os

import numpy as np
import pytest

from tests import clusters_cases as cc
from tests import pair_sites_cases as pc
from tests.conftest import load_golden


def test_rows_per_pair_are_the_matrix_entries_of_every_fixture(fixture_trees):
    """The predicate on the reference's own tables: for every pair i < j of the bundled snpma files the number of differing columns is
    the entry of the bundled matrix — and the bundled snplist has exactly one line per column."""
    for ds in ("lambdaVirus", "agona", "listeria"):
        root = fixture_trees[ds][0]
        for sfx in ("", "_preserved"):
            ids, sym = pc.read_fasta(os.path.join(root, "snpma%s.fasta" % sfx))
            want_ids, mat = cc.read_matrix_tsv(os.path.join(root, "snp_distance_matrix%s.tsv" % sfx))
            assert ids == want_ids, (ds, sfx)
            n = len(ids)
            a, b = np.triu_indices(n, 1)
            off, site, bases = pc.pair_sites(sym, a, b)
            assert np.array_equal(np.diff(off).astype(np.int64), mat[a, b].astype(np.int64)), (ds, sfx)
            assert len(pc.read_snp_list(os.path.join(root, "snplist%s.txt" % sfx))) == sym.shape[1], (ds, sfx)
            # ascending inside a pair, and the bases are the bytes of the two rows
            pair = np.searchsorted(off, np.arange(len(site), dtype=np.uint64), "right") - 1
            assert len(site) == int(mat[a, b].sum()) and (np.diff(site.astype(np.int64))[np.diff(pair) == 0] > 0).all()
            assert np.array_equal(np.frombuffer(pc.LETTERS.encode(), np.uint8)[bases & 7], sym[a[pair], site])
            assert np.array_equal(np.frombuffer(pc.LETTERS.encode(), np.uint8)[bases >> 4], sym[b[pair], site])


def test_rows_per_pair_on_every_run_of_the_reference_driver():
    from oracle import fuzz
    from oracle import steps_oracle as so
    texts = dict(fuzz.untidy_snpmas())
    seen = 0
    for run in load_golden("distance_runs.json.gz")["runs"]:
        if "pairwise" not in run:
            continue
        ids, mat = cc.read_pairwise_text(run["pairwise"])
        seqs = so.parse_snpma(texts[run["name"]].replace("\r\n", "\n"))
        got_ids, sym = pc.rows_of_seqs(dict(seqs))
        assert got_ids == sorted(ids), run["name"]
        order = [ids.index(i) for i in got_ids]
        assert np.array_equal(pc.counts(sym), mat[np.ix_(order, order)]), run["name"]
        seen += 1
    assert seen >= 3


def test_pairs_of_csr_against_the_statement():
    from snp_pipeline_amd import distance
    rng = np.random.default_rng(5)
    for n in (0, 1, 2, 7, 40):
        mat = rng.integers(0, 9, size=(n, n)).astype(np.int32)
        mat = np.minimum(mat, mat.T)
        np.fill_diagonal(mat, 0)
        for widest, t in ((8, 8), (8, 3), (3, 3), (0, 0)):
            csr = cc.filter_rows(mat, widest)
            got = distance.pairs_of_csr(*csr, t)
            want = pc.pairs_of_csr(*csr, t)
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), (n, widest, t)
            assert np.array_equal(got[0], pc.close_pairs(mat, t)[0]) and np.array_equal(got[1], pc.close_pairs(mat, t)[1])
            assert got[0].dtype == np.uint32 and got[1].dtype == np.uint32


def _write(path, ids, sym, a, b, snp_list=None):
    from snp_pipeline_amd import distance
    distance.write_pair_sites(path, ids, a, b, *pc.pair_sites(sym, a, b), snp_list=snp_list)
    with open(path, encoding="utf-8") as f:
        return f.read()


def test_writer_against_the_text_statement(tmp_path):
    from snp_pipeline_amd import distance
    path = str(tmp_path / "sites.tsv")
    ids = ["b sample", "S2_é", "'quoted'", "plain", "tab-less,comma"]          # ids go out as they are: no quoting rule
    sym = np.frombuffer(b"ACGTacgtNN-A" b"ACGTACGTACGT" b"acgtTGCAnn-c" b"ACGTacgtNN-A" b"TTTTttttTTTT", dtype=np.uint8).reshape(5, 12)
    snp_list = [("chr%d" % (k // 5), 10 + 7 * k) for k in range(12)]
    a, b = np.asarray([0, 2, 0, 3, 1, 4, 4], dtype=np.uint32), np.asarray([1, 0, 3, 3, 2, 0, 4], dtype=np.uint32)
    for table in (None, snp_list):
        got = _write(path, ids, sym, a, b, table)
        assert got == pc.text(ids, a, b, *pc.pair_sites(sym, a, b), snp_list=table) == pc.text_of_rows(ids, sym, a, b, snp_list=table)
        assert got.startswith(pc.HEADER_SITE if table is None else pc.HEADER_POS)
        assert "b sample\tplain\t" not in got                                      # rows 0 and 3 are equal: a pair with no rows
    got = _write(path, ids, sym, a, b)
    assert "b sample\tS2_é\t12\tA\tT\n" in got and "'quoted'\tb sample\t1\ta\tA\n" not in got and "'quoted'\tb sample\t5\tT\ta\n" in got
    assert "tab-less,comma\tb sample\t12\tT\tA\n" in got
    assert "b sample\tS2_é\tchr2\t87\tA\tT\n" in _write(path, ids, sym, a, b, snp_list)
    # m = 0: the header alone, with and without a table (also one without columns)
    none = np.zeros(0, dtype=np.uint32)
    assert _write(path, ids, sym, none, none) == pc.HEADER_SITE
    assert _write(path, ids, sym, none, none, snp_list) == pc.HEADER_POS
    assert _write(path, [], np.zeros((0, 0), np.uint8), none, none, []) == pc.HEADER_POS
    # enough entries for the writer's threads, in few pairs of unequal size: the block offsets must add up
    rng = np.random.default_rng(3)
    big = np.frombuffer(b"ACGTacgt", dtype=np.uint8)[rng.integers(0, 8, size=(6, 400000))]
    big[5] = big[0]
    big[5, ::1000] = ord("N")
    many = ["s%d" % i for i in range(6)]
    a, b = np.asarray([0, 0, 5, 2, 3, 4, 1, 0, 0, 0, 0, 0, 0], np.uint32), np.asarray([1, 5, 0, 3, 3, 0, 2, 2, 3, 4, 1, 2, 3], np.uint32)
    a, b = np.concatenate((a, b[:8])), np.concatenate((b, a[:8]))                # (and some of them the other way round)
    positions = [("contig_%d" % (k % 3), k * 3 + 1) for k in range(big.shape[1])]
    off, site, bases = pc.pair_sites(big, a, b)
    assert int(off[-1]) > 1 << 22
    for table in (None, positions):
        distance.write_pair_sites(path, many, a, b, off, site, bases, snp_list=table)
        with open(path) as f:
            got = f.read()
        assert got.count("\n") == int(off[-1]) + 1 and got == pc.text(many, a, b, off, site, bases, snp_list=table)
    with pytest.raises(IOError):
        distance.write_pair_sites(str(tmp_path / "no_such_dir" / "s.tsv"), ["a", "b"], [0], [1], [0, 0], [], [])
    with pytest.raises(ValueError):
        distance.write_pair_sites(path, ["a", "b"], [0], [2], [0, 0], [], [])       # a sample outside the ids
    with pytest.raises(ValueError):
        distance.write_pair_sites(path, ["a", "b"], [0], [1], [0, 1], [12], [0x10], snp_list=snp_list)   # a site outside the table


def test_new_options_keep_the_reference_namespace():
    from snp_pipeline_amd import cfsan_snp_pipeline as cli
    plain = vars(cli.parse_command_line("distance -p p.tsv x.fasta"))
    full = vars(cli.parse_command_line("distance -p p.tsv x.fasta --amdMaxPairDistance 9 --amdClosePairSites c.tsv --amdMstSites t.tsv --amdPairSitesPairs in.tsv "
                                       "--amdPairSitesOut out.tsv --amdSnpList snplist.txt"))
    added = {"amdClosePairSitesFile", "amdMstSitesFile", "amdPairSitesPairsFile", "amdPairSitesOutFile", "amdSnpListFile"}
    assert added <= set(full) and set(full) == set(plain) and all(plain[k] is None for k in added)
    assert [full[k] for k in sorted(added)] == ["c.tsv", "t.tsv", "out.tsv", "in.tsv", "snplist.txt"]
    assert {k: v for k, v in full.items() if not k.startswith("amd")} == {k: v for k, v in plain.items() if not k.startswith("amd")}
    assert vars(cli.parse_command_line("hot_path_batch dirs ref --closePairs 5 --pairSites"))["pairSites"] is True
    assert vars(cli.parse_command_line("hot_path_batch dirs ref"))["pairSites"] is False


def test_option_validation_exits_100(tmp_path, monkeypatch, capsys):
    from snp_pipeline_amd import cfsan_snp_pipeline as cli
    log = tmp_path / "error.log"
    monkeypatch.setenv("errorOutputFile", str(log))
    fasta = tmp_path / "snpma.fasta"
    fasta.write_text(">a\nACGT\n>b\nACGA\n")
    pairs = tmp_path / "pairs.tsv"
    pairs.write_text("Seq1\tSeq2\na\tb\nb\tnobody\n")
    short = tmp_path / "snplist.txt"
    short.write_text("chr\t1\t1\ta\nchr\t5\t1\tb\nchr\t9\t1\tb\n")
    out = str(tmp_path / "out.tsv")
    for line, msg in (("distance %s --amdClosePairSites %s" % (fasta, out), "--amdClosePairSites needs --amdMaxPairDistance"),
                      ("distance %s --amdClosePairSites %s --amdMaxPairDistance -1" % (fasta, out), "a distance threshold cannot be negative"),
                      ("distance %s --amdPairSitesPairs %s" % (fasta, pairs), "--amdPairSitesPairs and --amdPairSitesOut go together"),
                      ("distance %s --amdPairSitesOut %s" % (fasta, out), "--amdPairSitesPairs and --amdPairSitesOut go together"),
                      ("distance %s --amdPairSitesPairs %s --amdPairSitesOut %s" % (fasta, tmp_path / "absent.tsv", out), "without the pair list file"),
                      ("distance %s --amdMstSites %s --amdSnpList %s" % (fasta, out, tmp_path / "absent.txt"), "without the snplist file"),
                      ("distance %s --amdPairSitesPairs %s --amdPairSitesOut %s" % (fasta, pairs, out), "the id nobody of"),
                      ("distance %s --amdMstSites %s --amdSnpList %s" % (fasta, out, short), "lists 3 sites, the snp matrix has 4 columns"),
                      ("distance %s --amdSnpList %s --amdMaxPairDistance 3" % (fasta, short), "no output file specified")):
        if log.exists():
            log.unlink()
        args = cli.parse_command_line(line)
        with pytest.raises(SystemExit) as ei:
            args.func(args)
        assert ei.value.code == 100, line
        assert msg in log.read_text(), line
        assert not os.path.exists(out)
    (tmp_path / "dirs.txt").write_text("%s\n" % (tmp_path / "sample"))
    for line in ("hot_path_batch %s %s --pairSites" % (tmp_path / "dirs.txt", fasta),):
        if log.exists():
            log.unlink()
        args = cli.parse_command_line(line)
        with pytest.raises(SystemExit) as ei:
            args.func(args)
        assert ei.value.code == 100 and "--pairSites needs --closePairs or --mst" in log.read_text()
    capsys.readouterr()
