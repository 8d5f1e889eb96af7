"""The differing sites of close pairs, tree edges and chosen pairs through the commands: ``distance --amdClosePairSites /
--amdMstSites / --amdPairSitesPairs`` on the bundled SNP matrices, and ``hot_path_batch --pairSites`` with one rank and with two."""
import os
import shutil
import time

import numpy as np
import pytest

from tests import clusters_cases as cc
from tests import mst_cases as mc
from tests import pair_sites_cases as pc
from tests.ranks_util import ROOT, run_ranks
from tests.test_gpu_distance_clusters_cli import _read, _run
from tests.test_gpu_pipeline import CONSENSUS_EXTRA, VARSCAN_EXTRA, _outbreak_tree

pytestmark = pytest.mark.gpu

T = 5


def _tree_pairs(mat):
    tree = mc.mst_of_matrix(mat)
    return np.asarray([e[1] for e in tree], dtype=np.uint32), np.asarray([e[2] for e in tree], dtype=np.uint32)


@pytest.mark.parametrize("ds", ["lambdaVirus", "listeria"])
def test_distance_writes_the_sites_alone_and_next_to_everything_else(tmp_path, fixture_trees, ds):
    """(Before the options existed argparse left with status 2 here.)"""
    tree_dir = fixture_trees[ds][0]
    fasta, snplist = str(tmp_path / "snpma.fasta"), str(tmp_path / "snplist.txt")
    shutil.copyfile(os.path.join(tree_dir, "snpma.fasta"), fasta)
    shutil.copyfile(os.path.join(tree_dir, "snplist.txt"), snplist)
    old = time.time() - 1000
    for path in (fasta, snplist):
        os.utime(path, (old, old))
    ids, sym = pc.read_fasta(fasta)
    positions = pc.read_snp_list(snplist)
    want_ids, mat = cc.read_matrix_tsv(os.path.join(tree_dir, "snp_distance_matrix.tsv"))
    assert ids == want_ids and len(positions) == sym.shape[1]
    close, tree = pc.close_pairs(mat, T), _tree_pairs(mat)
    n = len(ids)
    chosen = (np.asarray([n - 1, 0, 1, 0, n - 1], dtype=np.uint32), np.asarray([0, n - 1, 1, 1, 0], dtype=np.uint32))     # reversed, a == b, repeated
    pairs_in = tmp_path / "pairs.tsv"
    pairs_in.write_text("Seq1\tSeq2\tNote\n" + "".join("%s\t%s\tkept for later\n" % (ids[i], ids[j]) for i, j in zip(*chosen)))
    os.utime(str(pairs_in), (old, old))
    want = {(kind, table is not None): pc.text_of_rows(ids, sym, a, b, snp_list=table)
            for kind, (a, b) in (("close", close), ("tree", tree), ("chosen", chosen)) for table in (None, positions)}
    assert want["tree", False].count("\n") - 1 == int(mat[tree].sum()) and want["close", True].count("\n") - 1 == int(mat[close].sum())
    assert want["chosen", False].count("\n") - 1 == int(mat[chosen].sum()) > 0
    if ds == "listeria":
        assert want["tree", False].count("\n") - 1 == 9986 and len(close[0]) == cc.LISTERIA_COUNTS[T][0]

    # each new output alone, without and with the site list: nothing else is written
    alone = tmp_path / "alone"
    alone.mkdir()
    for with_list in (False, True):
        more = " --amdSnpList %s" % snplist if with_list else ""
        tag = "p" if with_list else "s"
        _run("distance %s --amdClosePairSites %s --amdMaxPairDistance %d%s" % (fasta, alone / ("c_%s.tsv" % tag), T, more))
        _run("distance %s --amdMstSites %s%s" % (fasta, alone / ("t_%s.tsv" % tag), more))
        _run("distance %s --amdPairSitesPairs %s --amdPairSitesOut %s%s" % (fasta, pairs_in, alone / ("u_%s.tsv" % tag), more))
        assert _read(alone / ("c_%s.tsv" % tag)) == want["close", with_list]
        assert _read(alone / ("t_%s.tsv" % tag)) == want["tree", with_list]
        assert _read(alone / ("u_%s.tsv" % tag)) == want["chosen", with_list]
    assert sorted(os.listdir(str(alone))) == ["c_p.tsv", "c_s.tsv", "t_p.tsv", "t_s.tsv", "u_p.tsv", "u_s.tsv"]

    # together with everything else: the two reference tables stay the fixture's bytes, the other files what they are alone
    out = tmp_path / "out"
    out.mkdir()
    p, m, c, k, t, d, cs, ts, us = (str(out / name) for name in ("pairwise.tsv", "matrix.tsv", "close.tsv", "clusters.tsv", "mst.tsv", "dendrogram.nwk",
                                                                 "close_sites.tsv", "mst_sites.tsv", "chosen_sites.tsv"))
    line = ("distance %s -p %s -m %s --amdClosePairs %s --amdMaxPairDistance %d --amdClusters %s --amdClusterThresholds 20 0 --amdMst %s --amdDendrogram %s "
            "--amdClosePairSites %s --amdMstSites %s --amdPairSitesPairs %s --amdPairSitesOut %s --amdSnpList %s" % (fasta, p, m, c, T, k, t, d, cs, ts, pairs_in, us, snplist))
    _run(line)
    pairwise = _read(os.path.join(tree_dir, "snp_distance_pairwise.tsv"))
    assert _read(p) == pairwise and _read(m) == _read(os.path.join(tree_dir, "snp_distance_matrix.tsv"))
    edges = mc.mst_of_matrix(mat)
    assert _read(c) == cc.close_pairs_text_of_pairwise(pairwise, T) and _read(k) == cc.clusters_text(ids, mat, [0, 20])
    assert _read(t) == mc.mst_text(ids, edges) and _read(d) == mc.newick_text(ids, edges)
    assert _read(cs) == want["close", True] and _read(ts) == want["tree", True] and _read(us) == want["chosen", True]
    # the clusters ask for a wider threshold than the pairs: the sites are still those of the pairs within T
    _run("distance %s --amdClusters %s --amdClusterThresholds 20 --amdClosePairSites %s --amdMaxPairDistance %d" % (fasta, out / "k2.tsv", out / "cs2.tsv", T))
    assert _read(out / "cs2.tsv") == want["close", False] and _read(out / "k2.tsv") == cc.clusters_text(ids, mat, [20])
    _run("distance %s -m %s --amdPairSitesPairs %s --amdPairSitesOut %s" % (fasta, out / "m2.tsv", pairs_in, out / "us2.tsv"))
    assert _read(out / "us2.tsv") == want["chosen", False] and _read(out / "m2.tsv") == _read(m)

    # freshness: nothing is rewritten while the inputs are older; a missing new file counts on its own; a newer site list counts
    everything = (p, m, c, k, t, d, cs, ts, us)
    for path in everything:
        with open(path, "w") as f:
            f.write("kept\n")
    _run(line)
    assert all(_read(path) == "kept\n" for path in everything)
    os.remove(ts)
    _run(line)
    assert _read(ts) == want["tree", True] and _read(cs) == want["close", True] and _read(p) == pairwise
    with open(cs, "w") as f:
        f.write("kept\n")
    _run("distance %s --amdClosePairSites %s --amdMaxPairDistance %d" % (fasta, cs, T))
    assert _read(cs) == "kept\n"
    _run("distance -f %s --amdClosePairSites %s --amdMaxPairDistance %d" % (fasta, cs, T))
    assert _read(cs) == want["close", False]
    now = time.time() + 10
    os.utime(snplist, (now, now))
    with open(ts, "w") as f:
        f.write("kept\n")
    _run("distance %s --amdMstSites %s --amdSnpList %s" % (fasta, ts, snplist))
    assert _read(ts) == want["tree", True]


NEW_FILES = ("snp_close_pair_sites.tsv", "snp_close_pair_sites_preserved.tsv", "snp_mst_sites.tsv", "snp_mst_sites_preserved.tsv")


@pytest.mark.parametrize("world", [1, 2])
def test_hot_path_batch_writes_the_sites_of_its_own_pairs_and_tree(tmp_path, monkeypatch, world):
    """Seven samples; rank 0 asks the packed matrix every rank holds for the sites behind the gathered pairs and the merged tree."""
    work = tmp_path
    ref_path, dirs, dirs_file, _ = _outbreak_tree(work, n_samples=7)
    filter_extra = "--edge_length 100 --window_size 1000 125 15 --max_snp 3 2 1 --mode all"
    line = ("hot_path_batch -f %s %s --closePairs %d --mst --pairSites --filterRegionsExtraParams=%s --callConsensusExtraParams=%s --varscanExtraParams=%s"
            % (dirs_file, ref_path, T, filter_extra.replace(" ", "\x00"), CONSENSUS_EXTRA.replace(" ", "\x00"), VARSCAN_EXTRA.replace(" ", "\x00")))
    monkeypatch.chdir(work)
    if world == 1:
        _run(line)
    else:
        run_ranks(world, [os.path.join(ROOT, "bin", "cfsan_snp_pipeline")] + [w.replace("\x00", " ") for w in line.split()] + ["-v", "0"], work)
    got = {name: _read(work / name) for name in NEW_FILES}
    rows = 0
    for suffix in ("", "_preserved"):
        ids, sym = pc.read_fasta(str(work / ("snpma%s.fasta" % suffix)))
        positions = pc.read_snp_list(str(work / ("snplist%s.txt" % suffix)))
        want_ids, mat = cc.read_matrix_tsv(str(work / ("snp_distance_matrix%s.tsv" % suffix)))
        assert ids == want_ids and len(ids) == 7 and len(positions) == sym.shape[1]
        assert got["snp_close_pair_sites%s.tsv" % suffix] == pc.text_of_rows(ids, sym, *pc.close_pairs(mat, T), snp_list=positions)
        assert got["snp_mst_sites%s.tsv" % suffix] == pc.text_of_rows(ids, sym, *_tree_pairs(mat), snp_list=positions)
        assert got["snp_mst_sites%s.tsv" % suffix].count("\n") - 1 == int(mat[_tree_pairs(mat)].sum())
        rows += got["snp_mst_sites%s.tsv" % suffix].count("\n") - 1
    assert rows > 0
