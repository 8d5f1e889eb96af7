"""The statements of tests/mst_cases.py pinned on the reference's own tables, the host code of the tree (Kruskal over an edge list,
the two writers), and the options of ``distance`` / ``hot_path_batch`` — nothing here needs a GPU."""
import os

import numpy as np
import pytest

from tests import clusters_cases as cc
from tests import mst_cases as mc


def _matrix(fixture_trees, ds):
    return cc.read_matrix_tsv(os.path.join(fixture_trees[ds][0], "snp_distance_matrix.tsv"))


def test_trees_of_the_fixtures_are_the_literals(fixture_trees):
    for ds, n, total in (("lambdaVirus", 4, 239), ("agona", 6, 2663), ("listeria", 48, 9986)):
        ids, mat = _matrix(fixture_trees, ds)
        tree = mc.mst_of_matrix(mat)
        assert len(ids) == n and len(tree) == n - 1 and mc.weight(tree) == total, ds
        assert tree == sorted(tree) and all(i < j for _, i, j in tree)
        both, rounds = mc.boruvka(mat)
        assert both == tree and 1 <= rounds <= mc.ceil_log2(n), ds
        assert mc.kruskal(n, [(mat[i][j], j, i) for i in range(n) for j in range(n) if i != j]) == tree
    ids, mat = _matrix(fixture_trees, "listeria")
    tree = mc.mst_of_matrix(mat)
    assert sum(1 for e in tree if e[0] == 0) == 25
    assert tree[-1] == (9903, 36, 42)
    assert tree[:3] == [(0, 2, 4), (0, 2, 6), (0, 2, 11)]


def test_tree_edges_within_a_threshold_have_the_clusters_of_that_threshold(fixture_trees):
    ids, mat = _matrix(fixture_trees, "listeria")
    n = len(ids)
    tree = mc.mst_of_matrix(mat)
    for t, (_, clusters) in cc.LISTERIA_COUNTS.items():
        assert n - sum(1 for e in tree if e[0] <= t) == clusters, t
    for t in sorted(set(e[0] for e in tree)):
        labels = cc.union_find_labels(n, [(i, j) for d, i, j in tree if d <= t])
        assert np.array_equal(cc.numbers_of_labels(labels), cc.cluster_numbers(mat, t)), t


def test_total_weight_against_scipy(fixture_trees):
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    for ds in ("lambdaVirus", "agona", "listeria"):
        ids, mat = _matrix(fixture_trees, ds)
        n = len(ids)
        # (csgraph reads 0 as "no edge": every weight is raised by one, n - 1 edges carry the difference)
        total = int(csgraph.minimum_spanning_tree(np.asarray(mat, dtype=np.int64) + 1).sum()) - (n - 1)
        assert total == mc.weight(mc.mst_of_matrix(mat)), ds


@pytest.mark.parametrize("bands", [[(0, 16), (16, 32), (32, 48)], [(0, 20), (20, 40), (40, 48)], [(0, 1), (1, 48)], [(0, 0), (0, 48)]])
def test_forests_of_row_bands_merge_into_the_tree(fixture_trees, bands):
    ids, mat = _matrix(fixture_trees, "listeria")
    n = len(ids)
    tree = mc.mst_of_matrix(mat)
    merged = []
    for lo, hi in bands:
        forest, rounds = mc.boruvka(mat, lo, hi)
        assert forest == mc.mst_of_matrix(mat, lo, hi) and rounds <= mc.ceil_log2(n)
        assert len(forest) == (n - 1 if hi > lo else 0)              # a band's rows reach every sample
        merged += forest
    assert mc.kruskal(n, merged) == tree


def test_xor_matrix_pairs_components_up():
    mat = mc.xor_matrix(300)
    tree, rounds = mc.boruvka(mat)
    assert tree == mc.mst_of_matrix(mat) and mc.weight(tree) == 593 and rounds == 8
    band, band_rounds = mc.boruvka(mat, 128, 256)
    assert band == mc.mst_of_matrix(mat, 128, 256) and band_rounds == 7
    tie = mc.seeded_matrix(300, 17)
    tree = mc.mst_of_matrix(tie)
    assert [e[0] for e in tree] == [1] * 299 and mc.boruvka(tie)[0] == tree


def _of_edges(n, edges):
    from snp_pipeline_amd import distance
    u, v, d = mc.arrays(edges)
    return mc.edges_of_arrays(*distance.mst_of_edges(n, u, v, d))


def test_kruskal_over_an_edge_list_against_the_statement():
    from snp_pipeline_amd import distance
    rng = np.random.default_rng(23)
    for n, m in ((2, 1), (5, 30), (40, 25), (40, 400), (300, 200), (300, 5000)):
        edges = []
        for _ in range(m):
            u, v = (int(x) for x in rng.choice(n, size=2, replace=False))
            edges.append((int(rng.integers(0, 6)), u, v))                          # either orientation, many ties
        edges += [(d, v, u) for d, u, v in edges[::3]] + edges[::5]                # reversed edges and duplicates
        edges.append((mc.INT_MAX, 0, 1))
        want = mc.kruskal(n, edges)
        got = _of_edges(n, edges)
        assert got == want and got == sorted(got), (n, m)
        if (n, m) in ((40, 25), (300, 200)):
            assert len(want) < n - 1                                               # disconnected: a forest
    assert _of_edges(0, []) == [] and _of_edges(1, []) == [] and _of_edges(7, []) == []
    for bad in ([(1, 0, 3)], [(1, 3, 0)], [(1, 2, 2)]):
        with pytest.raises(ValueError):
            _of_edges(3, bad)
    with pytest.raises(ValueError):
        _of_edges(0, [(1, 0, 1)])
    # the merge of band forests, through the library
    mat = mc.random_matrix(97, 3, high=9)
    pieces = mc.mst_of_matrix(mat, 0, 40) + mc.mst_of_matrix(mat, 40, 80) + mc.mst_of_matrix(mat, 80, 97)
    assert _of_edges(97, pieces) == mc.mst_of_matrix(mat)
    assert distance.mst_of_edges(97, *mc.arrays(pieces))[0].dtype == np.uint32


def _read(path):
    with open(path, "rb") as f:
        return f.read().decode("utf-8")


def test_newick_statement_by_hand():
    assert mc.newick_text([], []) == ";\n" and mc.newick_text(["a"], []) == "a;\n" and mc.newick_text(["a_b"], []) == "'a_b';\n"
    assert mc.newick_text(["a", "b"], [(3, 0, 1)]) == "(a:1.5,b:1.5);\n"
    assert mc.newick_text(["a", "b"], [(0, 0, 1)]) == "(a:0,b:0);\n"
    # c joins b first; a, the smaller sample, is written first at the root; odd and even lengths
    assert mc.newick_text(["a", "b", "c"], [(2, 1, 2), (7, 0, 1)]) == "(a:3.5,(b:1,c:1):2.5);\n"
    # equal distances: nested nodes with zero-length branches
    assert mc.newick_text(["a", "b", "c"], [(4, 0, 1), (4, 0, 2)]) == "((a:2,b:2):0,c:2);\n"
    assert mc.label("it's") == "'it''s'" and mc.label("A.b|c-9") == "A.b|c-9" and mc.label("a b") == "'a b'" and mc.label("é") == "'é'"
    assert mc.label("x(1)") == "'x(1)'" and mc.label("a_b") == "'a_b'"


def test_host_writers_against_the_text_statements(tmp_path):
    from snp_pipeline_amd import distance
    path = str(tmp_path / "out.txt")
    odd = ["S_é", "two words", "it's", "par(en)", "under_score", "plain-1.2|x"]
    for n in (0, 1, 2, 3, 40):
        ids = [odd[i % 7] + str(i) if i % 7 < 6 else "sample%d" % i for i in range(n)]
        for high in (1, 3, 1000):                                    # all equal; many ties; odd and even distances
            mat = mc.random_matrix(n, 100 + n + high, high=high)
            tree = mc.mst_of_matrix(mat)
            distance.write_mst(path, ids, *mc.arrays(tree))
            assert _read(path) == mc.mst_text(ids, tree), (n, high)
            distance.write_dendrogram(path, ids, *mc.arrays(tree))
            text = _read(path)
            assert text == mc.newick_text(ids, tree), (n, high)
            assert text.endswith(";\n") and text.count("\n") == 1 and text.count("):") + text.count(");") == max(n - 1, 0)
    tree = [(2, 1, 2), (7, 0, 1)]
    distance.write_dendrogram(path, ["a", "b", "c"], *mc.arrays(tree))
    assert _read(path) == "(a:3.5,(b:1,c:1):2.5);\n"
    distance.write_dendrogram(path, ["a", "b", "c"], *mc.arrays([(4, 0, 1), (4, 0, 2)]))
    assert _read(path) == "((a:2,b:2):0,c:2);\n"
    distance.write_dendrogram(path, ["a", "b"], *mc.arrays([(mc.INT_MAX, 0, 1)]))
    assert _read(path) == "(a:1073741823.5,b:1073741823.5);\n"
    distance.write_mst(path, ["a", "b"], *mc.arrays([(mc.INT_MAX, 0, 1)]))
    assert _read(path) == mc.HEADER + "a\tb\t2147483647\n"


def test_a_chain_of_ten_thousand_joins_is_written_without_recursion(tmp_path):
    from snp_pipeline_amd import distance
    n = 10000
    ids = ["s%05d" % i for i in range(n)]
    tree = mc.chain_edges(n)
    assert mc.kruskal(n, tree) == tree
    path = str(tmp_path / "chain.nwk")
    distance.write_dendrogram(path, ids, *mc.arrays(tree))
    text = _read(path)
    assert text == mc.newick_text(ids, tree)
    assert text.startswith("(" * (n - 1) + "s00000:0.5,s00001:0.5):0,s00002:0.5):0,") and text.endswith(",s09999:0.5);\n")
    distance.write_mst(path, ids, *mc.arrays(tree))
    assert _read(path) == mc.mst_text(ids, tree)


def test_writers_refuse_what_is_not_a_tree_and_what_cannot_be_written(tmp_path):
    from snp_pipeline_amd import distance
    path = str(tmp_path / "out.nwk")
    ids = ["a", "b", "c"]
    for edges in ([(1, 0, 1)],                                      # too few edges
                  [(1, 0, 1), (2, 0, 1)],                           # a cycle
                  [(2, 0, 1), (1, 1, 2)],                           # descending
                  [(1, 1, 2), (1, 0, 1)],                           # ties out of (i, j) order
                  [(1, 0, 1), (2, 1, 3)],                           # an index past n
                  [(1, 0, 1), (2, 2, 2)]):
        with pytest.raises(ValueError):
            distance.write_dendrogram(path, ids, *mc.arrays(edges))
    with pytest.raises(ValueError):
        distance.write_mst(path, ids, *mc.arrays([(1, 0, 3)]))
    with pytest.raises(IOError):
        distance.write_mst(str(tmp_path / "no_such_dir" / "m.tsv"), ["a", "b"], *mc.arrays([(1, 0, 1)]))
    with pytest.raises(IOError):
        distance.write_dendrogram(str(tmp_path / "no_such_dir" / "d.nwk"), ["a", "b"], *mc.arrays([(1, 0, 1)]))


def test_new_options_keep_the_reference_namespace():
    from snp_pipeline_amd import cfsan_snp_pipeline as cli
    plain = vars(cli.parse_command_line("distance -p p.tsv -m m.tsv x.fasta"))
    full = vars(cli.parse_command_line("distance -p p.tsv -m m.tsv x.fasta --amdMst t.tsv --amdDendrogram d.nwk"))
    added = {"amdMstFile", "amdDendrogramFile"}
    assert added <= set(full) and set(full) == set(plain)
    assert all(plain[k] is None for k in added)
    assert {k: v for k, v in full.items() if k not in added} == {k: v for k, v in plain.items() if k not in added}
    assert (full["amdMstFile"], full["amdDendrogramFile"]) == ("t.tsv", "d.nwk")
    assert vars(cli.parse_command_line("hot_path_batch dirs ref --mst"))["mst"] is True
    assert vars(cli.parse_command_line("hot_path_batch dirs ref"))["mst"] is False


def test_option_validation_exits_100(tmp_path, monkeypatch, capsys):
    from snp_pipeline_amd import cfsan_snp_pipeline as cli
    log = tmp_path / "error.log"
    monkeypatch.setenv("errorOutputFile", str(log))
    fasta = tmp_path / "snpma.fasta"
    fasta.write_text(">a\nACGT\n>b\nACGA\n")
    out = str(tmp_path / "out.tsv")
    for line, msg in (("distance %s" % fasta, "no output file specified"),
                      ("distance %s --amdMst %s --amdClosePairs %s" % (fasta, out, out), "--amdClosePairs needs --amdMaxPairDistance"),
                      ("distance %s --amdDendrogram %s --amdClusters %s" % (fasta, out, out), "--amdClusters needs at least one threshold"),
                      ("distance %s --amdMst %s" % (tmp_path / "missing.fasta", out), "cannot calculate sequence distances without the snp matrix file")):
        if log.exists():
            log.unlink()
        args = cli.parse_command_line(line)
        with pytest.raises(SystemExit) as ei:
            args.func(args)
        assert ei.value.code == 100, line
        assert msg in log.read_text(), line
        assert not os.path.exists(out)
    capsys.readouterr()
