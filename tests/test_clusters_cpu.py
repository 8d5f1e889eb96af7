"""The statements of tests/clusters_cases.py pinned on the reference's own tables, the host writers of the two new files, and
the options of ``distance`` — nothing here needs a GPU."""
import os

import numpy as np
import pytest

from tests import clusters_cases as cc
from tests.conftest import load_golden

THRESHOLDS = (0, 5, 20, 100, cc.INT_MAX)


def _fixture_text(fixture_trees, ds, name):
    with open(os.path.join(fixture_trees[ds][0], name)) as f:
        return f.read()


def test_close_pairs_statement_is_the_filtered_pairwise_file_of_every_fixture(fixture_trees):
    for ds in ("lambdaVirus", "agona", "listeria"):
        pairwise = _fixture_text(fixture_trees, ds, "snp_distance_pairwise.tsv")
        ids, mat = cc.read_matrix_tsv(os.path.join(fixture_trees[ds][0], "snp_distance_matrix.tsv"))
        assert cc.pairwise_text(ids, mat) == pairwise
        for t in THRESHOLDS:
            want = cc.close_pairs_text_of_pairwise(pairwise, t)
            assert cc.close_pairs_text(ids, mat, t) == want, (ds, t)
            assert want.count("\n") - 1 >= len(ids), (ds, t)                    # the diagonal is always there
        assert cc.close_pairs_text(ids, mat, cc.INT_MAX) == pairwise


def test_close_pairs_statement_on_every_run_of_the_reference_driver():
    seen = 0
    for run in load_golden("distance_runs.json.gz")["runs"]:
        if "pairwise" not in run:
            continue
        ids, mat = cc.read_pairwise_text(run["pairwise"])
        for t in THRESHOLDS:
            assert cc.close_pairs_text(ids, mat, t) == cc.close_pairs_text_of_pairwise(run["pairwise"], t), (run["name"], t)
        seen += 1
    assert seen >= 3


def test_listeria_counts_are_the_literals(fixture_trees):
    ids, mat = cc.read_matrix_tsv(os.path.join(fixture_trees["listeria"][0], "snp_distance_matrix.tsv"))
    assert len(ids) == 48 and mat.min() == 0 and mat.max() == 10033
    got = {}
    for t in cc.LISTERIA_COUNTS:
        pairs = int((np.triu(mat <= t, 1)).sum())
        numbers = cc.cluster_numbers(mat, t)
        got[t] = (pairs, int(numbers.max()))
        # the numbering rule: cluster k's smallest member comes before cluster k + 1's, and the first sample is in cluster 1
        firsts = [int(np.flatnonzero(numbers == k)[0]) for k in range(1, int(numbers.max()) + 1)]
        assert firsts == sorted(firsts) and numbers[0] == 1
    assert got == {0: (98, 23), 2: (246, 9), 5: (290, 6), 10: (512, 3), 20: (531, 3), 50: (841, 2)}
    assert got == cc.LISTERIA_COUNTS


def test_component_statement_against_scipy(fixture_trees):
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    ids, mat = cc.read_matrix_tsv(os.path.join(fixture_trees["listeria"][0], "snp_distance_matrix.tsv"))
    for t in list(cc.LISTERIA_COUNTS) + [10033, 10032]:
        n_comp, lab = csgraph.connected_components(mat <= t, directed=False)
        numbers = cc.cluster_numbers(mat, t)
        assert n_comp == numbers.max()
        # same partition: scipy's labels and ours determine each other
        assert len(set(zip(lab.tolist(), numbers.tolist()))) == n_comp
        first = cc.union_find_labels(len(ids), np.argwhere(mat <= t))
        assert np.array_equal(cc.numbers_of_labels(first), numbers)


def test_thresholds_are_sorted_and_made_unique():
    from snp_pipeline_amd import distance
    assert distance.cluster_thresholds([20, 0, 5, 20, 0]) == [0, 5, 20] == cc.thresholds_in_order([20, 0, 5, 20, 0])
    mat = np.array([[0, 3, 9], [3, 0, 1], [9, 1, 0]])
    assert cc.clusters_text(["a", "b", "c"], mat, [5, 1, 5]) == "Id\t1\t5\na\t1\t1\nb\t2\t1\nc\t2\t1\n"
    assert cc.clusters_text([], np.zeros((0, 0)), [7, 2]) == "Id\t2\t7\n"


def test_filter_pairs_of_a_wider_csr():
    from snp_pipeline_amd import distance
    rng = np.random.default_rng(5)
    mat = rng.integers(0, 30, size=(37, 37)).astype(np.int32)
    wide = cc.filter_rows(mat, 20)
    for t in (0, 7, 20):
        got = distance.filter_pairs(wide[0], wide[1], wide[2], t)
        want = cc.filter_rows(mat, t)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), t


def test_host_writers_against_the_text_statements(tmp_path):
    from snp_pipeline_amd import distance
    path = str(tmp_path / "out.tsv")
    rng = np.random.default_rng(11)
    for n in (0, 1, 2, 40):
        ids = ["S%d_é" % i if i % 5 == 2 else "sample%d" % i for i in range(n)]
        mat = rng.integers(0, 12, size=(n, n)).astype(np.int32)
        mat = np.minimum(mat, mat.T)
        np.fill_diagonal(mat, 0)
        for t in (0, 3, cc.INT_MAX):
            distance.write_close_pairs(path, ids, *cc.filter_rows(mat, t))
            assert open(path, encoding="utf-8").read() == cc.close_pairs_text(ids, mat, t), (n, t)
        thresholds = [0, 2, 5, 11]
        numbers = np.asarray([cc.cluster_numbers(mat, t) for t in thresholds], dtype=np.uint32).reshape(len(thresholds), n)
        distance.write_clusters(path, ids, thresholds, numbers)
        assert open(path, encoding="utf-8").read() == cc.clusters_text(ids, mat, thresholds), n
    # enough values for the writers' threads: the block offsets must add up
    n = 2100
    ids = ["s%05d" % i for i in range(n)]
    mat = rng.integers(0, 1000, size=(n, n)).astype(np.int32)
    row_off, col, dist = cc.filter_rows(mat, cc.INT_MAX)
    distance.write_close_pairs(path, ids, row_off, col, dist)
    text = open(path).read()
    assert text.count("\n") == n * n + 1 and text == cc.pairwise_text(ids, mat)
    # the same for the clusters file: n * k values over 2^22, cluster numbers of 1 ... 7 digits
    n, thresholds = 850000, [0, 3, 17, 250, 10000]
    ids = ["s%d" % i for i in range(n)]
    numbers = (rng.integers(1, 10, size=(len(thresholds), n)) * 10 ** rng.integers(0, 7, size=(len(thresholds), n))).astype(np.uint32)
    assert n * len(thresholds) > 1 << 22 and numbers.min() < 10 and numbers.max() >= 10 ** 6
    distance.write_clusters(path, ids, thresholds, numbers)
    rows = map("\t".join, zip(ids, *(map(str, row.tolist()) for row in numbers)))
    assert open(path).read() == "Id\t0\t3\t17\t250\t10000\n" + "\n".join(rows) + "\n"
    with pytest.raises(IOError):
        distance.write_close_pairs(str(tmp_path / "no_such_dir" / "p.tsv"), ["a"], [0, 1], [0], [0])
    with pytest.raises(IOError):
        distance.write_clusters(str(tmp_path / "no_such_dir" / "c.tsv"), ["a"], [3], [[1]])


def test_new_options_keep_the_reference_namespace():
    from snp_pipeline_amd import cfsan_snp_pipeline as cli
    plain = vars(cli.parse_command_line("distance -p p.tsv -m m.tsv x.fasta"))
    full = vars(cli.parse_command_line("distance -p p.tsv -m m.tsv x.fasta --amdClosePairs c.tsv --amdMaxPairDistance 20 --amdClusters k.tsv --amdClusterThresholds 20 0 5"))
    added = {"amdClosePairsFile", "amdMaxPairDistance", "amdClustersFile", "amdClusterThresholds"}
    assert added <= set(full) and set(full) == set(plain)
    assert all(plain[k] is None for k in added)
    assert {k: v for k, v in full.items() if not k.startswith("amd")} == {k: v for k, v in plain.items() if not k.startswith("amd")}
    assert (full["amdClosePairsFile"], full["amdMaxPairDistance"], full["amdClustersFile"], full["amdClusterThresholds"]) == ("c.tsv", 20, "k.tsv", [20, 0, 5])
    batch = vars(cli.parse_command_line("hot_path_batch dirs ref --closePairs 20 --clusters 0 5 20"))
    assert (batch["closePairs"], batch["clusters"]) == (20, [0, 5, 20])
    none = vars(cli.parse_command_line("hot_path_batch dirs ref"))
    assert (none["closePairs"], none["clusters"]) == (None, None)


def test_option_validation_exits_100(tmp_path, monkeypatch, capsys):
    from snp_pipeline_amd import cfsan_snp_pipeline as cli
    log = tmp_path / "error.log"
    monkeypatch.setenv("errorOutputFile", str(log))
    fasta = tmp_path / "snpma.fasta"
    fasta.write_text(">a\nACGT\n>b\nACGA\n")
    out = str(tmp_path / "out.tsv")
    for line, msg in (("distance %s --amdClosePairs %s" % (fasta, out), "--amdClosePairs needs --amdMaxPairDistance"),
                      ("distance %s --amdClusters %s" % (fasta, out), "--amdClusters needs at least one threshold"),
                      ("distance %s --amdClosePairs %s --amdMaxPairDistance -1" % (fasta, out), "a distance threshold cannot be negative"),
                      ("distance %s --amdClusters %s --amdClusterThresholds 5 -2" % (fasta, out), "a distance threshold cannot be negative"),
                      ("distance %s --amdMaxPairDistance 3 --amdClusterThresholds 5" % fasta, "no output file specified"),
                      ("distance %s" % fasta, "no output file specified")):
        if log.exists():
            log.unlink()
        args = cli.parse_command_line(line)
        with pytest.raises(SystemExit) as ei:
            args.func(args)
        assert ei.value.code == 100, line
        assert msg in log.read_text(), line
        assert not os.path.exists(out)
    capsys.readouterr()
