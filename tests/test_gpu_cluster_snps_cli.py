"""The site counts and the cluster-defining SNPs through the command: ``distance --amdSiteCounts`` and ``--amdClusterSnps`` on the
bundled listeria SNP matrix, against the statements of tests/cluster_snps_cases.py."""
import os
import shutil
import time

import pytest

from tests import cluster_snps_cases as sc
from tests import clusters_cases as cc
from tests import nearest_cases as nc
from tests import pair_sites_cases as pc
from tests.test_gpu_distance_clusters_cli import _read, _run

pytestmark = pytest.mark.gpu

THRESHOLDS = [0, 5, 20, 50]


def test_distance_writes_the_site_counts_and_the_cluster_snps(tmp_path, fixture_trees):
    """(Before the options existed argparse left with status 2 here.)"""
    tree = fixture_trees["listeria"][0]
    fasta, snplist = str(tmp_path / "snpma.fasta"), str(tmp_path / "snplist.txt")
    shutil.copyfile(os.path.join(tree, "snpma.fasta"), fasta)
    shutil.copyfile(os.path.join(tree, "snplist.txt"), snplist)
    old = time.time() - 1000
    for path in (fasta, snplist):
        os.utime(path, (old, old))
    ids, mat = cc.read_matrix_tsv(os.path.join(tree, "snp_distance_matrix.tsv"))
    fasta_ids, sym = nc.read_fasta_rows(fasta)
    assert fasta_ids == ids and sym.shape == (48, 10102)
    positions = pc.read_snp_list(snplist)
    labellings = [cc.cluster_numbers(mat, t) for t in THRESHOLDS]
    want = {(kind, named): text for named, table in ((False, None), (True, positions))
            for kind, text in (("counts", sc.site_counts_text(sym, table)), ("snps", sc.cluster_snps_text(sym, THRESHOLDS, labellings, table)))}
    assert want["snps", False].count("\n") - 1 == 37 + 50 + 10058 + 20050 and want["counts", False].count("\n") - 1 == 10102

    # each alone, with and without the names of the sites: nothing else is written
    for named in (False, True):
        alone = tmp_path / ("alone%d" % named)
        alone.mkdir()
        more = " --amdSnpList %s" % snplist if named else ""
        _run("distance %s --amdSiteCounts %s%s" % (fasta, alone / "counts.tsv", more))
        assert os.listdir(str(alone)) == ["counts.tsv"] and _read(alone / "counts.tsv") == want["counts", named]
        _run("distance %s --amdClusterSnps %s --amdClusterThresholds 50 0 20 5 20%s" % (fasta, alone / "snps.tsv", more))
        assert sorted(os.listdir(str(alone))) == ["counts.tsv", "snps.tsv"] and _read(alone / "snps.tsv") == want["snps", named]

    # next to the clusters, the tables and the close pairs: the same file, and the others byte for byte what they are without it
    out, plain = tmp_path / "out", tmp_path / "plain"
    out.mkdir()
    plain.mkdir()
    others = "-p %s -m %s --amdClusters %s --amdClusterThresholds 0 5 20 50 --amdClosePairs %s --amdMaxPairDistance 20"
    names = ("pairwise.tsv", "matrix.tsv", "clusters.tsv", "close.tsv")
    line = "distance %s " % fasta + others % tuple(out / x for x in names) + " --amdClusterSnps %s --amdSiteCounts %s" % (out / "snps.tsv", out / "counts.tsv")
    _run(line)
    _run("distance %s " % fasta + others % tuple(plain / x for x in names))
    for name in names:
        assert _read(out / name) == _read(plain / name), name
    assert _read(out / "snps.tsv") == want["snps", False] and _read(out / "counts.tsv") == want["counts", False]
    assert _read(out / "clusters.tsv") == cc.clusters_text(ids, mat, THRESHOLDS)

    # every Cluster / Size of the file is a cluster of the clusters file of the same command, with that many members
    clusters = [ln.split("\t") for ln in _read(out / "clusters.tsv").splitlines()]
    assert clusters[0] == ["Id"] + [str(t) for t in THRESHOLDS]
    size = {}
    for fields in clusters[1:]:
        for t, number in zip(THRESHOLDS, fields[1:]):
            size[t, int(number)] = size.get((t, int(number)), 0) + 1
    seen = set()
    for ln in _read(out / "snps.tsv").splitlines()[1:]:
        t, c, _, base, members, sz = ln.split("\t")
        assert size[int(t), int(c)] == int(sz) and 1 <= int(members) <= int(sz) and base in "ACGT"
        seen.add((int(t), int(c)))
    assert {t for t, _ in seen} == set(THRESHOLDS) and (50, 1) in seen and (50, 2) in seen

    # the path that answers site files from a kept packed matrix writes the same file
    _run("distance %s --amdMst %s --amdMstSites %s --amdClusterSnps %s --amdClusterThresholds 0 5 20 50 --amdSnpList %s"
         % (fasta, out / "mst.tsv", out / "sites.tsv", out / "snps2.tsv", snplist))
    assert _read(out / "snps2.tsv") == want["snps", True]

    # freshness: nothing is rewritten while the inputs are older; -f rewrites
    paths = [str(out / x) for x in names + ("snps.tsv", "counts.tsv")]
    wanted = {path: _read(path) for path in paths}
    for path in paths:
        with open(path, "w") as f:
            f.write("kept\n")
    _run(line)
    assert all(_read(path) == "kept\n" for path in paths)
    _run(line.replace("distance ", "distance -f ", 1))
    assert all(_read(path) == text for path, text in wanted.items())
    k = str(out / "snps.tsv")
    with open(k, "w") as f:
        f.write("kept\n")
    alone_line = "distance %s --amdClusterSnps %s --amdClusterThresholds 0 5 20 50" % (fasta, k)
    _run(alone_line)
    assert _read(k) == "kept\n"
    _run(alone_line.replace("distance ", "distance -f ", 1))
    assert _read(k) == want["snps", False]
