"""The minimum spanning tree and the dendrogram through the commands: ``distance --amdMst / --amdDendrogram`` on the bundled SNP
matrices, and ``hot_path_batch --mst`` with one rank and with three."""
import os
import shutil
import time

import pytest

from tests import clusters_cases as cc
from tests import mst_cases as mc
from tests.ranks_util import ROOT, run_ranks
from tests.test_gpu_distance_clusters_cli import _read, _run
from tests.test_gpu_pipeline import CONSENSUS_EXTRA, VARSCAN_EXTRA, _outbreak_tree

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("ds", ["listeria", "agona"])
def test_distance_writes_the_tree_alone_and_next_to_the_reference_tables(tmp_path, fixture_trees, ds):
    """(Before the options existed argparse left with status 2 here.)"""
    tree_dir = fixture_trees[ds][0]
    fasta = str(tmp_path / "snpma.fasta")
    shutil.copyfile(os.path.join(tree_dir, "snpma.fasta"), fasta)
    old = time.time() - 1000
    os.utime(fasta, (old, old))
    ids, mat = cc.read_matrix_tsv(os.path.join(tree_dir, "snp_distance_matrix.tsv"))
    tree = mc.mst_of_matrix(mat)
    want_mst, want_nwk = mc.mst_text(ids, tree), mc.newick_text(ids, tree)
    assert want_mst.count("\n") == len(ids) and (ds != "listeria" or want_mst.endswith("\t9903\n"))

    # the new outputs alone, together and one at a time: nothing else is written
    alone = tmp_path / "alone"
    alone.mkdir()
    _run("distance %s --amdMst %s --amdDendrogram %s" % (fasta, alone / "t.tsv", alone / "d.nwk"))
    assert sorted(os.listdir(str(alone))) == ["d.nwk", "t.tsv"]
    assert _read(alone / "t.tsv") == want_mst and _read(alone / "d.nwk") == want_nwk
    _run("distance %s --amdDendrogram %s" % (fasta, alone / "d2.nwk"))
    _run("distance %s --amdMst %s" % (fasta, alone / "t2.tsv"))
    assert sorted(os.listdir(str(alone))) == ["d.nwk", "d2.nwk", "t.tsv", "t2.tsv"]
    assert _read(alone / "t2.tsv") == want_mst and _read(alone / "d2.nwk") == want_nwk

    # with the close pairs and clusters, without a table
    _run("distance %s --amdMst %s --amdClosePairs %s --amdMaxPairDistance 5 --amdClusters %s --amdClusterThresholds 20 0"
         % (fasta, alone / "t3.tsv", alone / "c3.tsv", alone / "k3.tsv"))
    pairwise = _read(os.path.join(tree_dir, "snp_distance_pairwise.tsv"))
    assert _read(alone / "t3.tsv") == want_mst and _read(alone / "c3.tsv") == cc.close_pairs_text_of_pairwise(pairwise, 5)
    assert _read(alone / "k3.tsv") == cc.clusters_text(ids, mat, [0, 20])

    # together with everything else: the two reference tables stay the fixture's bytes, the new files the same
    out = tmp_path / "out"
    out.mkdir()
    p, m, k, t, d = (str(out / name) for name in ("pairwise.tsv", "matrix.tsv", "clusters.tsv", "mst.tsv", "dendrogram.nwk"))
    line = "distance %s -p %s -m %s --amdClusters %s --amdClusterThresholds 20 0 5 --amdMst %s --amdDendrogram %s" % (fasta, p, m, k, t, d)
    _run(line)
    assert _read(p) == pairwise and _read(m) == _read(os.path.join(tree_dir, "snp_distance_matrix.tsv"))
    assert _read(k) == cc.clusters_text(ids, mat, [0, 5, 20]) and _read(t) == want_mst and _read(d) == want_nwk
    _run("distance -f %s -m %s --amdDendrogram %s" % (fasta, m, d))
    assert _read(m) == _read(os.path.join(tree_dir, "snp_distance_matrix.tsv")) and _read(d) == want_nwk

    # freshness: nothing is rewritten while the input is older; a missing new file counts on its own; -f rewrites
    for path in (p, m, k, t, d):
        with open(path, "w") as f:
            f.write("kept\n")
    _run(line)
    assert all(_read(path) == "kept\n" for path in (p, m, k, t, d))
    os.remove(d)
    _run(line)
    assert _read(d) == want_nwk and _read(t) == want_mst and _read(p) == pairwise
    with open(t, "w") as f:
        f.write("kept\n")
    _run("distance %s --amdMst %s" % (fasta, t))
    assert _read(t) == "kept\n"
    _run("distance -f %s --amdMst %s" % (fasta, t))
    assert _read(t) == want_mst
    now = time.time() + 10
    os.utime(fasta, (now, now))
    with open(d, "w") as f:
        f.write("kept\n")
    _run("distance %s --amdDendrogram %s" % (fasta, d))
    assert _read(d) == want_nwk


NEW_FILES = ("snp_mst.tsv", "snp_mst_preserved.tsv", "snp_dendrogram.nwk", "snp_dendrogram_preserved.nwk")


@pytest.mark.parametrize("world", [1, 3])
def test_hot_path_batch_writes_what_distance_writes_from_its_matrices(tmp_path, monkeypatch, world):
    """Seven samples: one 128-row tile, so of three ranks one holds the band with every row and two hold empty bands (no edges),
    and the matrix is padded from 7 to 128 rows and columns of zeros that must never appear as an edge.  (Bands that hold rows on
    every rank: tests/test_gpu_mst_ranks.py.)"""
    work = tmp_path
    ref_path, dirs, dirs_file, _ = _outbreak_tree(work, n_samples=7)
    filter_extra = "--edge_length 100 --window_size 1000 125 15 --max_snp 3 2 1 --mode all"
    line = ("hot_path_batch -f %s %s --mst --filterRegionsExtraParams=%s --callConsensusExtraParams=%s --varscanExtraParams=%s"
            % (dirs_file, ref_path, filter_extra.replace(" ", "\x00"), CONSENSUS_EXTRA.replace(" ", "\x00"), VARSCAN_EXTRA.replace(" ", "\x00")))
    monkeypatch.chdir(work)
    if world == 1:
        _run(line)
    else:
        run_ranks(world, [os.path.join(ROOT, "bin", "cfsan_snp_pipeline")] + [w.replace("\x00", " ") for w in line.split()] + ["-v", "0"], work)
    got = {name: _read(work / name) for name in NEW_FILES}
    assert not os.path.exists(str(work / "snp_clusters.tsv"))
    for suffix in ("", "_preserved"):
        fasta = work / ("snpma%s.fasta" % suffix)
        t, d = work / ("want_mst%s.tsv" % suffix), work / ("want_dendrogram%s.nwk" % suffix)
        _run("distance -f %s --amdMst %s --amdDendrogram %s" % (fasta, t, d))
        assert got["snp_mst%s.tsv" % suffix] == _read(t)
        assert got["snp_dendrogram%s.nwk" % suffix] == _read(d)
        # and both are the statements applied to the table the job wrote
        ids, mat = cc.read_matrix_tsv(str(work / ("snp_distance_matrix%s.tsv" % suffix)))
        tree = mc.mst_of_matrix(mat)
        assert len(ids) == 7 and len(tree) == 6
        assert _read(t) == mc.mst_text(ids, tree) and _read(d) == mc.newick_text(ids, tree)
