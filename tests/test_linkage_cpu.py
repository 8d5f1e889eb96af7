"""The statements of tests/linkage_cases.py pinned on themselves (the round form against the greedy definition, the properties of
the two linkages), on the reference's own tables, and the host code of the trees (the cut, the two writers) against them — nothing
here needs a GPU."""
import os

import numpy as np
import pytest

from tests import clusters_cases as cc
from tests import linkage_cases as lc
from tests import mst_cases as mc


def _tie_cases():
    """520 matrices of n <= 14 with entries 0 ... high, seeded: the fewer values, the more ties."""
    for seed in range(520):
        high = (1, 2, 3, 5, 50)[seed % 5]
        n = 2 + (seed * 7 + seed // 5) % 13
        yield n, high, seed, lc.tie_matrix(n, high, seed)


def test_merging_every_reciprocal_pair_per_round_builds_the_greedy_tree():
    """The exactness argument of csrc/linkage.hip.  Should this ever fail, `greedy` is the definition."""
    sizes = set()
    for n, high, seed, mat in _tie_cases():
        sizes.add(n)
        for kind in lc.KINDS:
            want = lc.greedy(mat, kind)
            got, count = lc.rounds(mat, kind)
            assert got == want, (n, high, seed, kind)
            assert 1 <= count <= n - 1
            keys = [lc.key(kind, m) for m in want]
            assert keys == sorted(keys) and len(set(keys)) == n - 1, (n, high, seed, kind)
            assert all(a < b for a, b, _, _, _ in want) and sum(1 for _ in want) == n - 1
    assert sizes == set(range(2, 15))
    for mat in (lc.planted_matrix(40, 300, 5), lc.hamming_matrix(lc.planted_symbols(30, 40, 30, seed=3)), lc.line_matrix(20), lc.xor_matrix(32)):
        for kind in lc.KINDS:
            assert lc.rounds(mat, kind)[0] == lc.greedy(mat, kind)


def test_identical_samples_merge_one_per_round():
    for kind in lc.KINDS:
        merges, count = lc.rounds(lc.zero_matrix(9), kind)
        assert merges == lc.greedy(lc.zero_matrix(9), kind) == [(0, j, j, 1, 0) for j in range(1, 9)] and count == 8
    merges, count = lc.rounds(lc.xor_matrix(64), "complete")
    assert count == 6 and merges == lc.greedy(lc.xor_matrix(64), "complete")


def test_sums_are_exact_at_the_largest_entries():
    mat = np.full((5, 5), cc.INT_MAX, dtype=np.int32)
    np.fill_diagonal(mat, 0)
    assert lc.greedy(mat, "average") == [(0, j, j, 1, j * cc.INT_MAX) for j in range(1, 5)]
    assert lc.greedy(mat, "complete") == [(0, j, j, 1, cc.INT_MAX) for j in range(1, 5)]


def _groups(numbers):
    groups = {}
    for i, c in enumerate(numbers):
        groups.setdefault(c, []).append(i)
    assert sorted(groups) == list(range(1, len(groups) + 1))
    assert [g[0] for _, g in sorted(groups.items())] == sorted(g[0] for g in groups.values())      # numbered by smallest sample
    return [g for _, g in sorted(groups.items())]


def test_complete_linkage_clusters_have_diameter_within_the_threshold_and_cannot_grow():
    for n, high, seed, mat in list(_tie_cases())[::4] + [(40, 0, 0, lc.planted_matrix(40, 300, 5))]:
        merges = lc.greedy(mat, "complete")
        for t in sorted(set([0, 1, 2, high // 2, high, high + 1] + [m[4] for m in merges])):
            groups = _groups(lc.cut(merges, "complete", n, t))
            for g in groups:
                assert lc.diameter(mat, g) <= t, (n, high, seed, t)
            for x in range(len(groups)):
                for y in range(x + 1, len(groups)):
                    assert lc.diameter(mat, groups[x] + groups[y]) > t, (n, high, seed, t)
        root = merges[-1][4]
        assert lc.cut(merges, "complete", n, root) == [1] * n and lc.cut(merges, "complete", n, root + 7) == [1] * n
        assert lc.cut(merges, "complete", n, -1) == list(range(1, n + 1))
        average = lc.greedy(mat, "average")
        a, b, sa, sb, num = average[-1]
        assert lc.cut(average, "average", n, -(-num // (sa * sb))) == [1] * n
        if num % (sa * sb):
            assert max(lc.cut(average, "average", n, num // (sa * sb))) > 1


def test_complete_linkage_newick_is_the_pinned_writer_fed_the_merges_as_edges():
    ids = ["s%d" % i for i in range(14)]
    for n, high, seed, mat in list(_tie_cases())[::7]:
        merges = lc.greedy(mat, "complete")
        edges = [(num, a, b) for a, b, _, _, num in merges]
        assert lc.newick_text(ids[:n], merges, "complete") == mc.newick_text(ids[:n], edges), (n, high, seed)


def test_text_statements_by_hand():
    assert lc.newick_text([], [], "average") == ";\n" and lc.newick_text(["a_b"], [], "complete") == "'a_b';\n"
    assert lc.newick_text(["a", "b", "c"], [(1, 2, 1, 1, 2), (0, 1, 1, 2, 14)], "complete") == "(a:7,(b:1,c:1):6);\n"
    assert lc.newick_text(["a", "b", "c"], [(1, 2, 1, 1, 2), (0, 1, 1, 2, 15)], "average") == "(a:3.75,(b:1,c:1):2.75);\n"
    assert lc.merges_text(["a", "b", "c"], [(1, 2, 1, 1, 2), (0, 1, 1, 2, 15)], "average") == lc.HEADER + "b\tc\t1\t1\t2.000000\na\tb\t1\t2\t7.500000\n"
    assert lc.merges_text(["a", "b", "c"], [(1, 2, 1, 1, 2), (0, 1, 1, 2, 15)], "complete") == lc.HEADER + "b\tc\t1\t1\t2\na\tb\t1\t2\t15\n"
    # S = 1 over 2 x 4 pairs: 0.125 exactly; the height 0.0625 is 62 500 millionths exactly: nothing is rounded
    assert lc.six_decimals(lc.half_up(1 * lc.MILLION, 2 * 4)) == "0.125000" and lc.height("average", (0, 2, 2, 4, 1)) == 62500
    # S = 1 over 8 x 16 pairs: 0.0078125, the seventh decimal is the half: up.  The height over 8 x 8: 7 812.5 millionths: up
    assert lc.six_decimals(lc.half_up(1 * lc.MILLION, 8 * 16)) == "0.007813" and lc.height("average", (0, 8, 8, 8, 1)) == 7813
    assert lc.length(0) == "0" and lc.length(7500000) == "7.5" and lc.length(62500) == "0.0625" and lc.length(3000001) == "3.000001"


def _star(first, count):
    """`count` identical samples from `first` on, as merges."""
    return [(first, first + j, j, 1, 0) for j in range(1, count)]


def _read(path):
    with open(path, "rb") as f:
        return f.read().decode("utf-8")


def test_host_writers_and_the_cut_against_the_statements(tmp_path):
    from snp_pipeline_amd import distance
    path = str(tmp_path / "out.txt")
    odd = ["S_é", "two words", "it's", "par(en)", "under_score", "plain-1.2|x"]
    for n in (0, 1, 2, 3, 14, 40):
        ids = [odd[i % 7] + str(i) if i % 7 < 6 else "sample%d" % i for i in range(n)]
        for high in (0, 2, 999):
            mat = lc.tie_matrix(n, high, 100 + n + high)
            for kind in lc.KINDS:
                merges = lc.greedy(mat, kind)
                distance.write_linkage_merges(path, ids, kind, *lc.arrays(merges))
                assert _read(path) == lc.merges_text(ids, merges, kind), (n, high, kind)
                distance.write_linkage_dendrogram(path, ids, kind, *lc.arrays(merges))
                text = _read(path)
                assert text == lc.newick_text(ids, merges, kind), (n, high, kind)
                assert text.endswith(";\n") and text.count("\n") == 1
                thresholds = [0, 1, 2, 500, 999, 1000]
                numbers, counts = distance.linkage_cut(kind, n, *(lc.arrays(merges) + (thresholds,)))
                assert numbers.shape == (len(thresholds), n) and numbers.dtype == np.uint32
                for row, t, count in zip(numbers, thresholds, counts):
                    assert row.tolist() == lc.cut(merges, kind, n, t) and count == (max(row) if n else 0), (n, high, kind, t)
                distance.write_linkage_outputs(ids, kind, lc.arrays(merges), None, None, path, [500, 0, 2, 2])
                assert _read(path) == lc.clusters_text(ids, merges, kind, [0, 2, 500])
    # the half-up rule at exact halves, and the case without rounding
    ids = ["s%02d" % i for i in range(24)]
    merges = _star(0, 8) + _star(8, 16) + [(0, 8, 8, 16, 1)]
    distance.write_linkage_merges(path, ids, "average", *lc.arrays(merges))
    assert _read(path) == lc.merges_text(ids, merges, "average") and _read(path).endswith("s00\ts08\t8\t16\t0.007813\n")
    merges = _star(0, 8) + _star(8, 8) + [(0, 8, 8, 8, 1)]
    distance.write_linkage_dendrogram(path, ids[:16], "average", *lc.arrays(merges))
    assert _read(path) == lc.newick_text(ids[:16], merges, "average") and _read(path).endswith(",s15:0):0.007813);\n")
    merges = _star(0, 2) + _star(2, 4) + [(0, 2, 2, 4, 1)]
    distance.write_linkage_merges(path, ids[:6], "average", *lc.arrays(merges))
    assert _read(path).endswith("s00\ts02\t2\t4\t0.125000\n")
    distance.write_linkage_dendrogram(path, ids[:6], "average", *lc.arrays(merges))
    assert _read(path) == "((s00:0,s01:0):0.0625,(((s02:0,s03:0):0,s04:0):0,s05:0):0.0625);\n"
    # the largest numbers: 2^31 - 1 between two samples; a sum of four of them
    distance.write_linkage_dendrogram(path, ["a", "b"], "complete", *lc.arrays([(0, 1, 1, 1, cc.INT_MAX)]))
    assert _read(path) == "(a:1073741823.5,b:1073741823.5);\n"
    merges = [(0, 1, 1, 1, 0), (2, 3, 1, 1, 0), (0, 2, 2, 2, 4 * cc.INT_MAX)]
    distance.write_linkage_merges(path, ["a", "b", "c", "d"], "average", *lc.arrays(merges))
    assert _read(path).endswith("a\tc\t2\t2\t2147483647.000000\n")


def test_a_chain_of_ten_thousand_joins_is_written_without_recursion(tmp_path):
    from snp_pipeline_amd import distance
    n = 10000
    ids = ["s%05d" % i for i in range(n)]
    merges = [(0, j, j, 1, j) for j in range(1, n)]
    path = str(tmp_path / "chain.nwk")
    distance.write_linkage_dendrogram(path, ids, "complete", *lc.arrays(merges))
    text = _read(path)
    assert text == lc.newick_text(ids, merges, "complete")
    assert text.startswith("(" * (n - 1) + "s00000:0.5,s00001:0.5):0.5,s00002:1):0.5,") and text.endswith(",s09999:4999.5);\n")


def test_writers_refuse_what_is_not_a_tree_and_what_cannot_be_written(tmp_path):
    from snp_pipeline_amd import distance
    path = str(tmp_path / "out.nwk")
    ids = ["a", "b", "c"]
    for merges in ([(0, 1, 1, 1, 1)],                                # too few merges
                   [(0, 1, 1, 1, 1), (1, 2, 1, 1, 2)],               # cluster 1 has retired
                   [(0, 1, 1, 1, 1), (0, 2, 1, 1, 2)],               # a wrong size
                   [(1, 0, 1, 1, 1), (0, 2, 2, 1, 2)],               # a > b
                   [(0, 1, 1, 1, 1), (0, 3, 2, 1, 2)],               # an index past n
                   [(0, 1, 1, 1, 5), (0, 2, 2, 1, 4)]):              # a parent below its child
        with pytest.raises(ValueError):
            distance.write_linkage_dendrogram(path, ids, "complete", *lc.arrays(merges))
    with pytest.raises(ValueError):
        distance.write_linkage_merges(path, ids, "average", *lc.arrays([(0, 3, 1, 1, 1)]))
    with pytest.raises(ValueError):
        distance.linkage_cut("complete", 3, *(lc.arrays([(2, 1, 1, 1, 1)]) + ([1],)))
    with pytest.raises(ValueError):                                 # cluster 1 has retired: the cut checks the tree as the writers do
        distance.linkage_cut("complete", 3, *(lc.arrays([(0, 1, 1, 1, 1), (1, 2, 1, 1, 2)]) + ([1],)))
    with pytest.raises(ValueError):                                 # a wrong size
        distance.linkage_cut("average", 3, *(lc.arrays([(0, 1, 1, 1, 1), (0, 2, 1, 1, 2)]) + ([1],)))
    # a distance whose millionths leave 64 bits: refused where millionths are written, written where they are not
    huge = [(0, 1, 1, 1, 2 ** 64 - 1)]
    for kind in lc.KINDS:
        with pytest.raises(ValueError):
            distance.write_linkage_dendrogram(path, ["a", "b"], kind, *lc.arrays(huge))
    with pytest.raises(ValueError):
        distance.write_linkage_merges(path, ["a", "b"], "average", *lc.arrays(huge))
    distance.write_linkage_merges(path, ["a", "b"], "complete", *lc.arrays(huge))
    assert _read(path) == lc.HEADER + "a\tb\t1\t1\t18446744073709551615\n"
    most = (2 ** 64 - 1) // 10 ** 6                                 # the largest distance whose millionths fit 64 bits
    distance.write_linkage_dendrogram(path, ["a", "b"], "complete", *lc.arrays([(0, 1, 1, 1, most)]))
    assert _read(path) == lc.newick_text(["a", "b"], [(0, 1, 1, 1, most)], "complete")
    with pytest.raises(ValueError):
        distance.write_linkage_dendrogram(path, ["a", "b"], "complete", *lc.arrays([(0, 1, 1, 1, most + 1)]))
    with pytest.raises(ValueError):
        distance.write_linkage_merges(path, ids, "single", *lc.arrays([(0, 1, 1, 1, 1)]))
    for write in (distance.write_linkage_merges, distance.write_linkage_dendrogram):
        with pytest.raises(IOError):
            write(str(tmp_path / "no_such_dir" / "x"), ["a", "b"], "average", *lc.arrays([(0, 1, 1, 1, 1)]))


@pytest.mark.parametrize("ds,n", [("lambdaVirus", 4), ("agona", 6)])
def test_both_linkages_on_the_tables_of_the_fixtures(fixture_trees, tmp_path, ds, n):
    from snp_pipeline_amd import distance
    ids, mat = cc.read_matrix_tsv(os.path.join(fixture_trees[ds][0], "snp_distance_matrix.tsv"))
    mat = np.asarray(mat, dtype=np.int32)
    assert len(ids) == n
    single = mc.mst_of_matrix(mat)
    for kind in lc.KINDS:
        merges = lc.greedy(mat, kind)
        assert lc.rounds(mat, kind)[0] == merges and len(merges) == n - 1
        assert merges[0][4] == single[0][0] and merges[0][:2] == single[0][1:]          # the closest pair merges first in every linkage
        heights = [lc.height(kind, m) for m in merges]
        assert heights == sorted(heights)
        path = str(tmp_path / (kind + ".nwk"))
        distance.write_linkage_dendrogram(path, ids, kind, *lc.arrays(merges))
        assert _read(path) == lc.newick_text(ids, merges, kind)
    complete = lc.greedy(mat, "complete")
    assert complete[-1][4] == int(mat.max())                         # the root of complete linkage lies at the largest distance
    for t in sorted(set(int(x) for x in mat.reshape(-1))):
        for g in _groups(lc.cut(complete, "complete", n, t)):
            assert lc.diameter(mat, g) <= t
        single_groups = _groups(cc.numbers_of_labels(cc.union_find_labels(n, [(i, j) for d, i, j in single if d <= t])).tolist())
        assert len(single_groups) <= len(_groups(lc.cut(complete, "complete", n, t)))    # single linkage chains: never more groups


def test_new_options_keep_the_reference_namespace():
    from snp_pipeline_amd import cfsan_snp_pipeline as cli
    plain = vars(cli.parse_command_line("distance -p p.tsv -m m.tsv x.fasta"))
    full = vars(cli.parse_command_line("distance -p p.tsv -m m.tsv x.fasta --amdLinkage average --amdLinkageMerges a.tsv --amdLinkageDendrogram b.nwk "
                                       "--amdLinkageClusters c.tsv --amdClusterThresholds 3"))
    added = {"amdLinkage", "amdLinkageMergesFile", "amdLinkageDendrogramFile", "amdLinkageClustersFile"}
    assert added <= set(full) and set(full) == set(plain) and all(plain[k] is None for k in added)
    assert [full[k] for k in sorted(added)] == ["average", "c.tsv", "b.nwk", "a.tsv"]
    with pytest.raises(SystemExit):
        cli.parse_command_line("distance x.fasta --amdLinkage single --amdLinkageMerges a.tsv")


def test_option_validation_exits_100(tmp_path, monkeypatch, capsys):
    from snp_pipeline_amd import cfsan_snp_pipeline as cli
    log = tmp_path / "error.log"
    monkeypatch.setenv("errorOutputFile", str(log))
    fasta = tmp_path / "snpma.fasta"
    fasta.write_text(">a\nACGT\n>b\nACGA\n")
    out = str(tmp_path / "out.tsv")
    for line, msg in (("distance %s --amdLinkageMerges %s" % (fasta, out), "need --amdLinkage"),
                      ("distance %s --amdLinkageDendrogram %s -p %s" % (fasta, out, out), "need --amdLinkage"),
                      ("distance %s --amdLinkage complete" % fasta, "--amdLinkage needs at least one of"),
                      ("distance %s --amdLinkage complete -p %s" % (fasta, out), "--amdLinkage needs at least one of"),
                      ("distance %s --amdLinkage average --amdLinkageClusters %s" % (fasta, out), "--amdLinkageClusters needs at least one threshold")):
        if log.exists():
            log.unlink()
        args = cli.parse_command_line(line)
        with pytest.raises(SystemExit) as ei:
            args.func(args)
        assert ei.value.code == 100, line
        assert msg in log.read_text(), line
        assert not os.path.exists(out)
    capsys.readouterr()
