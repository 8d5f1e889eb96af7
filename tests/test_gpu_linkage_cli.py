"""The complete- and average-linkage outputs through the commands: ``distance --amdLinkage ...`` on the bundled SNP matrices, and
``hot_path_batch --linkage`` against ``distance`` on the snpma.fasta the job wrote."""
import os
import pathlib
import shutil
import time

import numpy as np
import pytest

from tests import clusters_cases as cc
from tests import linkage_cases as lc
from tests.ranks_util import ROOT, run_ranks
from tests.test_gpu_distance_clusters_cli import _read, _run
from tests.test_gpu_pipeline import CONSENSUS_EXTRA, VARSCAN_EXTRA, _outbreak_tree

pytestmark = pytest.mark.gpu


def _old_fasta(tmp_path, tree_dir):
    fasta = str(tmp_path / "snpma.fasta")
    shutil.copyfile(os.path.join(tree_dir, "snpma.fasta"), fasta)
    old = time.time() - 1000
    os.utime(fasta, (old, old))
    return fasta


@pytest.mark.parametrize("kind", lc.KINDS)
@pytest.mark.parametrize("ds", ["listeria", "agona"])
def test_distance_writes_the_linkage_files_alone_and_next_to_everything_else(tmp_path, fixture_trees, ds, kind):
    """(Before the options existed argparse left with status 2 here.)"""
    tree_dir = fixture_trees[ds][0]
    fasta = _old_fasta(tmp_path, tree_dir)
    ids, mat = cc.read_matrix_tsv(os.path.join(tree_dir, "snp_distance_matrix.tsv"))
    merges = lc.greedy(np.asarray(mat, dtype=np.int32), kind)
    thresholds = [20, 0, 5, 5]
    want = {"m": lc.merges_text(ids, merges, kind), "d": lc.newick_text(ids, merges, kind), "k": lc.clusters_text(ids, merges, kind, thresholds)}
    assert want["m"].count("\n") == len(ids) and want["k"].startswith("Id\t0\t5\t20\n")
    options = {"m": "--amdLinkageMerges", "d": "--amdLinkageDendrogram", "k": "--amdLinkageClusters"}
    thr = " --amdClusterThresholds " + " ".join(str(t) for t in thresholds)

    # each new output alone, then the three together: nothing else is written
    alone = tmp_path / "alone"
    alone.mkdir()
    for which in "mdk":
        _run("distance %s --amdLinkage %s %s %s%s" % (fasta, kind, options[which], alone / which, thr if which == "k" else ""))
        assert _read(alone / which) == want[which], which
    assert sorted(os.listdir(str(alone))) == ["d", "k", "m"]
    three = tmp_path / "three"
    three.mkdir()
    _run("distance %s --amdLinkage %s %s%s" % (fasta, kind, " ".join("%s %s" % (options[w], three / w) for w in "mdk"), thr))
    assert sorted(os.listdir(str(three))) == ["d", "k", "m"] and all(_read(three / w) == want[w] for w in "mdk")

    # next to the tree, the close pairs and the single-linkage clusters without a table: the linkage computes the matrix once more
    beside = tmp_path / "beside"
    beside.mkdir()
    _run("distance %s --amdMst %s/t --amdClosePairs %s/q --amdMaxPairDistance 5 --amdClusters %s/c%s --amdLinkage %s %s"
         % (fasta, beside, beside, beside, thr, kind, " ".join("%s %s" % (options[w], beside / ("linkage_" + w)) for w in "mdk")))
    assert sorted(os.listdir(str(beside))) == ["c", "linkage_d", "linkage_k", "linkage_m", "q", "t"]
    assert all(_read(beside / ("linkage_" + w)) == want[w] for w in "mdk")

    # next to the tables, the tree and the single-linkage clusters: the earlier outputs are the bytes of a run without the new options
    before, after = tmp_path / "before", tmp_path / "after"
    before.mkdir()
    after.mkdir()
    rest = "-p %s/p -m %s/m --amdMst %s/t --amdClusters %s/c" + thr
    _run("distance %s %s" % (fasta, rest % ((before,) * 4)))
    _run("distance %s %s --amdLinkage %s %s" % (fasta, rest % ((after,) * 4), kind, " ".join("%s %s" % (options[w], after / ("linkage_" + w)) for w in "mdk")))
    assert sorted(os.listdir(str(after))) == ["c", "linkage_d", "linkage_k", "linkage_m", "m", "p", "t"]
    for name in "pmtc":
        assert _read(after / name) == _read(before / name), name
    assert _read(after / "p") == _read(os.path.join(tree_dir, "snp_distance_pairwise.tsv"))
    assert _read(after / "c") == cc.clusters_text(ids, mat, [0, 5, 20])
    assert all(_read(after / ("linkage_" + w)) == want[w] for w in "mdk")
    assert _read(beside / "t") == _read(after / "t") and _read(beside / "c") == _read(after / "c")
    assert _read(beside / "q") == cc.close_pairs_text_of_pairwise(_read(after / "p"), 5)


def test_linkage_next_to_the_sites_of_the_tree_edges(tmp_path, fixture_trees):
    """The path of ``distance`` that keeps the packed matrix on the device: with a table the linkage comes from its matrix, without
    one from a computation of its own."""
    tree_dir = fixture_trees["agona"][0]
    fasta = _old_fasta(tmp_path, tree_dir)
    ids, mat = cc.read_matrix_tsv(os.path.join(tree_dir, "snp_distance_matrix.tsv"))
    out = tmp_path / "out"
    out.mkdir()
    for kind in lc.KINDS:
        merges = lc.greedy(np.asarray(mat, dtype=np.int32), kind)
        _run("distance -f %s -m %s --amdLinkage %s --amdLinkageMerges %s --amdMstSites %s" % (fasta, out / "matrix", kind, out / "merges", out / "sites"))
        assert _read(out / "matrix") == _read(os.path.join(tree_dir, "snp_distance_matrix.tsv"))
        assert _read(out / "merges") == lc.merges_text(ids, merges, kind)
        _run("distance -f %s --amdLinkage %s --amdLinkageDendrogram %s --amdMstSites %s" % (fasta, kind, out / "nwk", out / "sites2"))
        assert _read(out / "nwk") == lc.newick_text(ids, merges, kind) and _read(out / "sites2") == _read(out / "sites")


def test_misuse_is_a_global_error(tmp_path, monkeypatch, capsys, fixture_trees):
    from snp_pipeline_amd import cfsan_snp_pipeline as cli
    log = tmp_path / "error.log"
    monkeypatch.setenv("errorOutputFile", str(log))
    fasta = _old_fasta(tmp_path, fixture_trees["agona"][0])
    out = str(tmp_path / "out.tsv")
    for line, msg in (("distance %s --amdLinkageDendrogram %s" % (fasta, out), "need --amdLinkage"),
                      ("distance %s --amdLinkage average -p %s" % (fasta, out), "--amdLinkage needs at least one of"),
                      ("distance %s --amdLinkage complete --amdLinkageClusters %s" % (fasta, out), "--amdLinkageClusters needs at least one threshold")):
        if log.exists():
            log.unlink()
        args = cli.parse_command_line(line)
        with pytest.raises(SystemExit) as ei:
            args.func(args)
        assert ei.value.code == 100 and msg in log.read_text(), line
        assert not os.path.exists(out)
    capsys.readouterr()


def test_freshness_skips_and_rebuilds(tmp_path, fixture_trees):
    tree_dir = fixture_trees["agona"][0]
    fasta = _old_fasta(tmp_path, tree_dir)
    ids, mat = cc.read_matrix_tsv(os.path.join(tree_dir, "snp_distance_matrix.tsv"))
    merges = lc.greedy(np.asarray(mat, dtype=np.int32), "average")
    want_m, want_d = lc.merges_text(ids, merges, "average"), lc.newick_text(ids, merges, "average")
    m, d = str(tmp_path / "merges.tsv"), str(tmp_path / "tree.nwk")
    line = "distance %s --amdLinkage average --amdLinkageMerges %s --amdLinkageDendrogram %s" % (fasta, m, d)
    _run(line)
    assert _read(m) == want_m and _read(d) == want_d
    for path in (m, d):
        with open(path, "w") as f:
            f.write("kept\n")
    _run(line)
    assert _read(m) == "kept\n" and _read(d) == "kept\n"             # fresh: nothing is rewritten
    os.remove(d)
    _run(line)
    assert _read(m) == want_m and _read(d) == want_d                 # a missing new file counts on its own
    with open(m, "w") as f:
        f.write("kept\n")
    _run(line.replace("distance ", "distance -f "))
    assert _read(m) == want_m
    now = time.time() + 10
    os.utime(fasta, (now, now))
    with open(d, "w") as f:
        f.write("kept\n")
    _run(line)
    assert _read(d) == want_d                                        # the input is newer


NEW_FILES = ("snp_linkage.tsv", "snp_linkage_preserved.tsv", "snp_linkage.nwk", "snp_linkage_preserved.nwk", "snp_linkage_clusters.tsv",
             "snp_linkage_clusters_preserved.tsv")


@pytest.mark.parametrize("world", [1, 3])
def test_hot_path_batch_writes_what_distance_writes_from_its_matrices(tmp_path, monkeypatch, world):
    """One rank builds the tree from its device matrix (padded from 7 to 128 rows and columns that must never be taken); with three
    ranks rank 0 builds it from the matrix it gathers for the tables."""
    work = tmp_path
    ref_path, dirs, dirs_file, _ = _outbreak_tree(work, n_samples=7)
    filter_extra = "--edge_length 100 --window_size 1000 125 15 --max_snp 3 2 1 --mode all"
    line = ("hot_path_batch -f %s %s --linkage average --clusters 2 5 --filterRegionsExtraParams=%s --callConsensusExtraParams=%s --varscanExtraParams=%s"
            % (dirs_file, ref_path, filter_extra.replace(" ", "\x00"), CONSENSUS_EXTRA.replace(" ", "\x00"), VARSCAN_EXTRA.replace(" ", "\x00")))
    monkeypatch.chdir(work)
    if world == 1:
        _run(line)
    else:
        run_ranks(world, [os.path.join(ROOT, "bin", "cfsan_snp_pipeline")] + [w.replace("\x00", " ") for w in line.split()] + ["-v", "0"], work)
    _compare_with_distance(work, 7)


def test_hot_path_batch_on_the_lambda_virus_tree(tmp_path, monkeypatch, fixture_trees):
    """The bundled lambdaVirus samples (their own var.flt.vcf files, --siteCalling existing): both flows against ``distance`` on the
    snpma.fasta the job wrote."""
    from tests.test_gpu_pipeline import _foreign_tree
    root, work, ref_path, names, dirs, dirs_file, piles = _foreign_tree(tmp_path, fixture_trees, "lambdaVirus")
    monkeypatch.chdir(work)
    monkeypatch.delenv("SNPGPU_SITE_CALLING", raising=False)
    filter_extra = "--edge_length 500 --window_size 1000 125 15 --max_snp 3 2 1 --mode all"
    _run("hot_path_batch -f --siteCalling existing %s %s --linkage average --clusters 2 5 --filterRegionsExtraParams=%s --callConsensusExtraParams=%s"
         % (dirs_file, ref_path, filter_extra.replace(" ", "\x00"), CONSENSUS_EXTRA.replace(" ", "\x00")))
    _compare_with_distance(work, len(names))
    assert len(names) == 4 and cc.read_matrix_tsv(os.path.join(str(work), "snp_distance_matrix.tsv"))[0] == sorted(names)


def _compare_with_distance(work, n):
    """The six files of a job in `work` against ``distance`` on the job's own snpma*.fasta and against the statements."""
    work = pathlib.Path(str(work))
    got = {name: _read(work / name) for name in NEW_FILES}
    for suffix in ("", "_preserved"):
        fasta = work / ("snpma%s.fasta" % suffix)
        m, d, k = (work / ("want_%s%s" % (name, suffix)) for name in ("merges", "tree", "clusters"))
        _run("distance -f %s --amdLinkage average --amdLinkageMerges %s --amdLinkageDendrogram %s --amdLinkageClusters %s --amdClusterThresholds 2 5" % (fasta, m, d, k))
        assert got["snp_linkage%s.tsv" % suffix] == _read(m)
        assert got["snp_linkage%s.nwk" % suffix] == _read(d)
        assert got["snp_linkage_clusters%s.tsv" % suffix] == _read(k)
        # and all are the statements applied to the table the job wrote
        ids, mat = cc.read_matrix_tsv(str(work / ("snp_distance_matrix%s.tsv" % suffix)))
        merges = lc.greedy(np.asarray(mat, dtype=np.int32), "average")
        assert len(ids) == n and _read(m) == lc.merges_text(ids, merges, "average") and _read(d) == lc.newick_text(ids, merges, "average")
        assert _read(k) == lc.clusters_text(ids, merges, "average", [2, 5])
