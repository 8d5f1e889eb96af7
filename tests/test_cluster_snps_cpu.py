"""The statements of the site counts and the cluster-defining SNPs (tests/cluster_snps_cases.py) pinned against a second loop over
sets and Counters and against the bundled listeria matrix, the two host writers, and the options of ``distance --amdSiteCounts /
--amdClusterSnps``, whose errors must reach the user before a device is needed.  No GPU."""
import collections
import os

import numpy as np
import pytest

from tests import cluster_snps_cases as sc
from tests import clusters_cases as cc
from tests import nearest_cases as nc


def _by_hand(sym, labels, n_clusters):
    """Column by column with a Counter per cluster: (counts rows, {(cluster, site): (base, members)})."""
    def letter(c):
        c = int(c)
        if 97 <= c <= 122:
            c -= 32
        return chr(c) if chr(c) in "ACGT" else None

    n, s = sym.shape
    counts, rows = [], {}
    for col in range(s):
        held = [letter(sym[r, col]) for r in range(n)]
        all_of = collections.Counter(x for x in held if x)
        counts.append([all_of.get(x, 0) for x in "ACGT"])
        for c in range(1, n_clusters + 1):
            mine = collections.Counter(held[r] for r in range(n) if labels[r] == c and held[r])
            if len(set(mine)) != 1:
                continue
            (base, members), = mine.items()
            outside = set(held[r] for r in range(n) if labels[r] != c)
            if base not in outside:
                rows[(c, col)] = ("ACGT".index(base), members)
    return counts, rows


@pytest.mark.parametrize("n,s,seed,every_byte", [(1, 9, 1, False), (2, 40, 2, False), (9, 70, 3, False), (23, 33, 4, True), (12, 64, 5, False)])
def test_the_statements_are_the_loop_over_sets_and_counters(n, s, seed, every_byte):
    for name, labels in sc.labellings(n, seed).items():
        sym = sc.random_symbols(n, s, seed, every_byte) if every_byte or name == "interleaved" else sc.planted_symbols(n, s, labels, seed)
        if n >= 9:
            sym[1, :8] = np.frombuffer(b"acgtnN-.", dtype=np.uint8)
            sym[:, 9] = np.frombuffer(b"Aa", dtype=np.uint8)[np.arange(n) % 2]             # one allele in both cases: the all-samples cluster's
            sym[:, 10] = 0x2D                                                               # nobody holds a base
        n_clusters = int(labels.max())
        counts, rows = _by_hand(sym, labels, n_clusters)
        assert sc.site_counts(sym).tolist() == counts, name
        off, site, base, members = sc.cluster_snps(sym, labels)
        assert len(off) == n_clusters + 1 and off[0] == 0 and off[-1] == len(site) == len(rows), name
        got = {}
        for c in range(n_clusters):
            cols = site[int(off[c]):int(off[c + 1])]
            assert (np.diff(cols.astype(np.int64)) > 0).all(), name
            for e in range(int(off[c]), int(off[c + 1])):
                got[(c + 1, int(site[e]))] = (int(base[e]), int(members[e]))
        assert got == rows, name
        per_site = collections.Counter(col for _, col in rows)
        assert max(per_site.values() or [0]) <= 4
        if name == "one" and n >= 9:
            assert (1, 9) in rows and rows[(1, 9)] == (0, n) and (1, 10) not in rows
        if name == "singletons":                                    # a singleton lists its private alleles
            assert all(m == 1 for _, m in rows.values())


@pytest.fixture(scope="module")
def listeria(fixture_trees):
    tree = fixture_trees["listeria"][0]
    ids, mat = cc.read_matrix_tsv(os.path.join(tree, "snp_distance_matrix.tsv"))
    fasta_ids, rows = nc.read_fasta_rows(os.path.join(tree, "snpma.fasta"))
    assert fasta_ids == ids and rows.shape == (48, 10102)
    return ids, rows, mat


# threshold -> (clusters, sizes or None, rows, rows with Members == Size)
LISTERIA = {0: (23, None, 37, 33), 5: (6, [5, 11, 20, 10, 1, 1], 50, 36), 20: (3, [7, 31, 10], 10058, 9871), 50: (2, [7, 41], 20050, 19834)}


def test_the_listeria_clusters_own_the_snps_the_issue_counted(listeria):
    ids, rows, mat = listeria
    counts = sc.site_counts(rows)
    assert counts[0].tolist() == [7, 0, 41, 0]
    alleles = (counts > 0).sum(axis=1)
    assert [int((alleles == k).sum()) for k in (0, 1, 2, 3, 4)] == [0, 1, 10100, 1, 0]
    for t, (clusters, sizes, n_rows, n_full) in LISTERIA.items():
        labels = cc.cluster_numbers(mat, t)
        assert int(labels.max()) == clusters == cc.LISTERIA_COUNTS[t][1]
        size = sc.sizes_of(labels)
        if sizes is not None:
            assert size.tolist() == sizes
        off, site, base, members = sc.cluster_snps(rows, labels)
        of_entry = np.repeat(np.arange(clusters), np.diff(off.astype(np.int64)))
        assert (len(site), int((members == size[of_entry]).sum())) == (n_rows, n_full), t
        assert (members <= size[of_entry]).all() and (members > 0).all()
        assert np.array_equal(members, counts[site, base])           # every holder of the base is a member


def _read(path):
    with open(str(path), "rb") as f:
        return f.read().decode("utf-8")


def test_the_writers_give_the_texts_of_the_statement(tmp_path):
    from snp_pipeline_amd import distance
    path = str(tmp_path / "out.tsv")
    for n, s, seed in ((0, 0, 1), (3, 0, 2), (0, 5, 3), (1, 1, 4), (14, 90, 5), (30, 41, 6)):
        labs = sc.labellings(n, seed)
        sym = sc.planted_symbols(n, s, labs["planted"], seed) if n else np.zeros((0, s), dtype=np.uint8)
        snp_list = [("chr%d|é" % (k // 30), 7 * k + 1) for k in range(s)]
        for named in (None, snp_list):
            distance.write_site_counts(path, sc.site_counts(sym), n, snp_list=named)
            assert _read(path) == sc.site_counts_text(sym, named), (n, s)
            thresholds = [0, 3, 17, 2 ** 31 - 1]
            chosen = [labs[k] for k in ("singletons", "planted", "interleaved", "one")]
            got = [sc.cluster_snps(sym, lab) for lab in chosen]
            base0 = np.cumsum([0] + [len(g[1]) for g in got])
            distance.write_cluster_snps(path, thresholds, [sc.sizes_of(lab) for lab in chosen], [g[0] + np.uint64(b) for g, b in zip(got, base0)],
                                        np.concatenate([g[1] for g in got]), np.concatenate([g[2] for g in got]), np.concatenate([g[3] for g in got]),
                                        columns=s, snp_list=named)
            assert _read(path) == sc.cluster_snps_text(sym, thresholds, chosen, named), (n, s)
    assert sc.site_counts_text(np.frombuffer(b"AaC-", dtype=np.uint8).reshape(4, 1)) == "Site\tA\tC\tG\tT\tOther\n1\t2\t1\t0\t0\t1\n"
    distance.write_cluster_snps(path, [], [], [], [], [], [], columns=0)
    assert _read(path) == sc.SNPS_HEADER == "Threshold\tCluster\tSite\tBase\tMembers\tSize\n"


def test_the_writers_refuse_what_is_not_a_result(tmp_path):
    from snp_pipeline_amd import distance
    path = str(tmp_path / "bad.tsv")
    with pytest.raises(ValueError):
        distance.write_site_counts(path, [[1, 1, 1, 1]], 3)
    with pytest.raises(ValueError):
        distance.write_site_counts(path, [[1, -1, 0, 0]], 3)
    with pytest.raises(ValueError):
        distance.write_site_counts(path, [[1, 0, 0, 0]], 3, snp_list=[("c", 1), ("c", 2)])
    for site, base, off in (([5], [0], [0, 1]), ([0], [4], [0, 1]), ([0], [0], [1, 1]), ([0, 1], [0, 0], [0, 1])):
        with pytest.raises(ValueError):
            distance.write_cluster_snps(path, [3], [[2]], [off], site, base, [1] * len(site), columns=5)
    assert not os.path.exists(path)
    with pytest.raises(IOError):
        distance.write_site_counts(str(tmp_path / "no_such_dir" / "n.tsv"), [[1, 0, 0, 0]], 1)


def test_new_options_keep_the_reference_namespace():
    from snp_pipeline_amd import cfsan_snp_pipeline as cli
    plain = vars(cli.parse_command_line("distance -p p.tsv x.fasta"))
    full = vars(cli.parse_command_line("distance -p p.tsv x.fasta --amdSiteCounts c.tsv --amdClusterSnps s.tsv --amdClusterThresholds 5 0"))
    assert {"amdSiteCountsFile", "amdClusterSnpsFile"} <= set(full) and set(full) == set(plain)
    assert plain["amdSiteCountsFile"] is None and plain["amdClusterSnpsFile"] is None
    assert (full["amdSiteCountsFile"], full["amdClusterSnpsFile"]) == ("c.tsv", "s.tsv")
    assert {k: v for k, v in full.items() if not k.startswith("amd")} == {k: v for k, v in plain.items() if not k.startswith("amd")}


def test_option_validation_exits_100_without_a_device(tmp_path, monkeypatch, capsys):
    from snp_pipeline_amd import cfsan_snp_pipeline as cli
    from snp_pipeline_amd import device

    def no_device():
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(device, "default_device", no_device)
    log = tmp_path / "error.log"
    monkeypatch.setenv("errorOutputFile", str(log))
    fasta = tmp_path / "snpma.fasta"
    fasta.write_text(">a\nACGT\n>b\nACGA\n")
    short = tmp_path / "snplist.txt"
    short.write_text("chr\t1\t2\ta\tb\nchr\t5\t1\ta\n")
    out = str(tmp_path / "out.tsv")
    absent = tmp_path / "absent.txt"
    for line, msg in (("distance %s --amdClusterSnps %s" % (fasta, out), "--amdClusterSnps needs at least one threshold in --amdClusterThresholds"),
                      ("distance %s --amdClusterSnps %s --amdClusters %s" % (fasta, out, out), "--amdClusterSnps needs at least one threshold"),
                      ("distance %s --amdClusterSnps %s --amdClusterThresholds 3 -1" % (fasta, out), "a distance threshold cannot be negative"),
                      ("distance %s --amdSiteCounts %s --amdSnpList %s" % (fasta, out, absent), "--amdSnpList"),
                      ("distance %s --amdClusterSnps %s --amdClusterThresholds 1 --amdSnpList %s" % (fasta, out, absent), "--amdSnpList"),
                      ("distance %s --amdSiteCounts %s --amdSnpList %s" % (fasta, out, short), "lists 2 sites, the snp matrix has 4 columns"),
                      ("distance %s --amdClusterSnps %s --amdClusterThresholds 1 --amdSnpList %s" % (fasta, out, short), "lists 2 sites, the snp matrix has 4 columns"),
                      ("distance %s --amdSiteCounts %s" % (tmp_path / "absent.fasta", out), "without the snp matrix file")):
        if log.exists():
            log.unlink()
        args = cli.parse_command_line(line)
        with pytest.raises(SystemExit) as ei:
            args.func(args)
        assert ei.value.code == 100, line
        assert msg in log.read_text(), line
        assert not os.path.exists(out)
    # nothing to count: a file without records or without columns, and still no device
    empty = tmp_path / "empty.fasta"
    empty.write_text("")
    bare = tmp_path / "bare.fasta"
    bare.write_text(">b\n>a\n")
    for source in (empty, bare):
        args = cli.parse_command_line("distance -f %s --amdSiteCounts %s" % (source, out))
        args.verbose = 0
        args.func(args)
        assert _read(out) == sc.COUNTS_HEADER
        os.remove(out)
    capsys.readouterr()
