"""The close-pairs and clusters outputs through the commands: ``distance --amdClosePairs / --amdClusters`` on the bundled SNP
matrices, and ``hot_path_batch --closePairs / --clusters`` with one rank and with three."""
import os
import shutil
import time

import pytest

from tests import clusters_cases as cc
from tests.ranks_util import ROOT, run_ranks
from tests.test_gpu_pipeline import CONSENSUS_EXTRA, VARSCAN_EXTRA, _outbreak_tree

pytestmark = pytest.mark.gpu


def _run(line):
    from snp_pipeline_amd import cfsan_snp_pipeline as cli
    args = cli.parse_argument_list([w.replace("\x00", " ") for w in line.split()])
    args.verbose = 0
    assert cli.run_command_from_args(args) == 0


def _read(path):
    with open(str(path), "rb") as f:
        return f.read().decode("utf-8")


@pytest.mark.parametrize("ds", ["listeria", "agona"])
def test_distance_writes_the_new_files_next_to_the_reference_tables(tmp_path, fixture_trees, ds):
    """(Before the options existed argparse left with status 2 here.)"""
    tree = fixture_trees[ds][0]
    fasta = str(tmp_path / "snpma.fasta")
    shutil.copyfile(os.path.join(tree, "snpma.fasta"), fasta)
    old = time.time() - 1000
    os.utime(fasta, (old, old))
    out = tmp_path / "out"
    out.mkdir()
    p, m, c, k = (str(out / name) for name in ("pairwise.tsv", "matrix.tsv", "close.tsv", "clusters.tsv"))
    _run("distance %s -p %s -m %s --amdClosePairs %s --amdMaxPairDistance 20 --amdClusters %s --amdClusterThresholds 20 0 5 5" % (fasta, p, m, c, k))
    pairwise = _read(os.path.join(tree, "snp_distance_pairwise.tsv"))
    assert _read(p) == pairwise and _read(m) == _read(os.path.join(tree, "snp_distance_matrix.tsv"))
    ids, mat = cc.read_matrix_tsv(os.path.join(tree, "snp_distance_matrix.tsv"))
    want_close, want_clusters = cc.close_pairs_text_of_pairwise(pairwise, 20), cc.clusters_text(ids, mat, [0, 5, 20])
    assert _read(c) == want_close and want_close.count("\n") - 1 > len(ids)
    assert _read(k) == want_clusters and want_clusters.startswith("Id\t0\t5\t20\n")
    if ds == "listeria":
        last = [int(ln.split("\t")[-1]) for ln in want_clusters.splitlines()[1:]]
        assert max(last) == cc.LISTERIA_COUNTS[20][1]

    # the new outputs alone: no table is written, and the pairs within 20 are the same rows
    alone = tmp_path / "alone"
    alone.mkdir()
    _run("distance %s --amdClosePairs %s --amdMaxPairDistance 20" % (fasta, alone / "c.tsv"))
    assert os.listdir(str(alone)) == ["c.tsv"] and _read(alone / "c.tsv") == want_close
    _run("distance %s --amdClusters %s --amdClusterThresholds 5" % (fasta, alone / "k.tsv"))
    assert sorted(os.listdir(str(alone))) == ["c.tsv", "k.tsv"] and _read(alone / "k.tsv") == cc.clusters_text(ids, mat, [5])
    # a pair threshold below the cluster thresholds: the file is cut at its own threshold, not at the widest
    _run("distance -f %s --amdClosePairs %s --amdMaxPairDistance 0 --amdClusters %s --amdClusterThresholds 50" % (fasta, alone / "c0.tsv", alone / "k50.tsv"))
    assert _read(alone / "c0.tsv") == cc.close_pairs_text_of_pairwise(pairwise, 0) and _read(alone / "k50.tsv") == cc.clusters_text(ids, mat, [50])

    # freshness: nothing is rewritten while the input is older, everything once it is newer
    line = "distance %s -p %s -m %s --amdClosePairs %s --amdMaxPairDistance 20 --amdClusters %s --amdClusterThresholds 0 5 20" % (fasta, p, m, c, k)
    for path in (p, m, c, k):
        with open(path, "w") as f:
            f.write("kept\n")
    _run(line)
    assert all(_read(path) == "kept\n" for path in (p, m, c, k))
    now = time.time() + 10
    os.utime(fasta, (now, now))
    _run(line)
    assert _read(p) == pairwise and _read(c) == want_close and _read(k) == want_clusters
    # ... and each new file counts on its own
    os.utime(fasta, (old, old))
    for path in (p, m, k):
        with open(path, "w") as f:
            f.write("kept\n")
    os.remove(c)
    _run(line)
    assert _read(c) == want_close and _read(k) == want_clusters and _read(p) == pairwise


NEW_FILES = ("snp_distance_close_pairs.tsv", "snp_distance_close_pairs_preserved.tsv", "snp_clusters.tsv", "snp_clusters_preserved.tsv")


@pytest.mark.parametrize("world", [1, 3])
def test_hot_path_batch_writes_what_distance_writes_from_its_matrices(tmp_path, monkeypatch, world):
    """Seven samples: one 128-row tile, so of three ranks one holds the band with every row and two hold empty bands, and the
    matrix is padded from 7 to 128 rows and columns of zeros that no threshold may let through.  (Bands that hold rows on every
    rank, a band that begins past row 0 and the joining of several pieces: tests/test_gpu_clusters_ranks.py, where a 300-row matrix
    takes the place of 300 pileups.)"""
    from snp_pipeline_amd import sharding
    work = tmp_path
    ref_path, dirs, dirs_file, _ = _outbreak_tree(work, n_samples=7)
    bands = sharding.RowBands(7, 3)
    assert bands.n_padded == 128 > 7 and sorted(hi - lo for lo, hi in bands.bands) == [0, 0, 1]
    filter_extra = "--edge_length 100 --window_size 1000 125 15 --max_snp 3 2 1 --mode all"
    line = ("hot_path_batch -f %s %s --closePairs 20 --clusters 0 5 20 --filterRegionsExtraParams=%s --callConsensusExtraParams=%s --varscanExtraParams=%s"
            % (dirs_file, ref_path, filter_extra.replace(" ", "\x00"), CONSENSUS_EXTRA.replace(" ", "\x00"), VARSCAN_EXTRA.replace(" ", "\x00")))
    monkeypatch.chdir(work)
    if world == 1:
        _run(line)
    else:
        run_ranks(world, [os.path.join(ROOT, "bin", "cfsan_snp_pipeline")] + [w.replace("\x00", " ") for w in line.split()] + ["-v", "0"], work)
    got = {name: _read(work / name) for name in NEW_FILES}
    for suffix in ("", "_preserved"):
        fasta = work / ("snpma%s.fasta" % suffix)
        c, k = work / ("want_close%s.tsv" % suffix), work / ("want_clusters%s.tsv" % suffix)
        _run("distance -f %s --amdClosePairs %s --amdMaxPairDistance 20 --amdClusters %s --amdClusterThresholds 0 5 20" % (fasta, c, k))
        assert got["snp_distance_close_pairs%s.tsv" % suffix] == _read(c)
        assert got["snp_clusters%s.tsv" % suffix] == _read(k)
        # and both are the statements applied to the tables the job wrote
        pairwise = _read(work / ("snp_distance_pairwise%s.tsv" % suffix))
        ids, mat = cc.read_matrix_tsv(str(work / ("snp_distance_matrix%s.tsv" % suffix)))
        assert len(ids) == 7
        assert _read(c) == cc.close_pairs_text_of_pairwise(pairwise, 20) and _read(k) == cc.clusters_text(ids, mat, [0, 5, 20])
