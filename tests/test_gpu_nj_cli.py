"""The neighbour-joining tree through the commands: ``distance --amdNj`` on the bundled SNP matrices, and ``hot_path_batch --nj``
against ``distance`` on the snpma.fasta the job wrote."""
import os
import pathlib

import numpy as np
import pytest

from tests import clusters_cases as cc
from tests import nj_cases as nc
from tests.test_gpu_distance_clusters_cli import _read, _run
from tests.test_gpu_linkage_cli import _old_fasta
from tests.test_gpu_pipeline import CONSENSUS_EXTRA, VARSCAN_EXTRA, _outbreak_tree

pytestmark = pytest.mark.gpu


def _want(table):
    ids, mat = cc.read_matrix_tsv(str(table))
    return nc.newick_text(ids, nc.nj_numpy(np.asarray(mat, dtype=np.int32))), len(ids)


@pytest.mark.parametrize("ds", ["listeria", "lambdaVirus"])
def test_distance_writes_the_tree_alone_and_next_to_everything_else(tmp_path, fixture_trees, ds):
    """(Before the option existed argparse left with status 2 here.)"""
    tree_dir = fixture_trees[ds][0]
    fasta = _old_fasta(tmp_path, tree_dir)
    want, n = _want(os.path.join(tree_dir, "snp_distance_matrix.tsv"))
    assert want.count("\n") == 1 and want.endswith(");\n") and want.count(",") == n - 1 and want.count("(") == n - 2

    # alone: nothing else is written, and the n x n matrix stays on the device
    alone = tmp_path / "alone"
    alone.mkdir()
    _run("distance %s --amdNj %s" % (fasta, alone / "nj"))
    assert _read(alone / "nj") == want and os.listdir(str(alone)) == ["nj"]

    # with the tables, from their matrix: the tables are the bytes of a run without the option
    before, after = tmp_path / "before", tmp_path / "after"
    before.mkdir()
    after.mkdir()
    _run("distance %s -p %s/p -m %s/m" % (fasta, before, before))
    _run("distance %s -p %s/p -m %s/m --amdNj %s/nj" % (fasta, after, after, after))
    assert sorted(os.listdir(str(before))) == ["m", "p"] and sorted(os.listdir(str(after))) == ["m", "nj", "p"]
    for name in "pm":
        assert _read(after / name) == _read(before / name), name
    assert _read(after / "p") == _read(os.path.join(tree_dir, "snp_distance_pairwise.tsv"))
    assert _read(after / "nj") == want

    # beside the minimum spanning tree without a table: one more computation of the matrix, the same bytes
    beside, plain = tmp_path / "beside", tmp_path / "plain"
    beside.mkdir()
    plain.mkdir()
    _run("distance %s --amdMst %s/t" % (fasta, plain))
    _run("distance %s --amdMst %s/t --amdNj %s/nj" % (fasta, beside, beside))
    assert sorted(os.listdir(str(plain))) == ["t"] and sorted(os.listdir(str(beside))) == ["nj", "t"]
    assert _read(beside / "t") == _read(plain / "t") and _read(beside / "nj") == want

    # and on the path that keeps the packed matrix for the sites of the tree's edges
    _run("distance -f %s --amdNj %s/nj2 --amdMstSites %s/sites" % (fasta, beside, beside))
    assert _read(beside / "nj2") == want


def test_hot_path_batch_writes_what_distance_writes_from_its_matrices(tmp_path, monkeypatch):
    """One rank builds the tree from its device matrix (padded from 7 to 128 rows and columns that must never be read).  Without
    the option no new file appears."""
    work = tmp_path
    ref_path, dirs, dirs_file, _ = _outbreak_tree(work, n_samples=7)
    filter_extra = "--edge_length 100 --window_size 1000 125 15 --max_snp 3 2 1 --mode all"
    line = ("hot_path_batch -f %s %s %%s --filterRegionsExtraParams=%s --callConsensusExtraParams=%s --varscanExtraParams=%s"
            % (dirs_file, ref_path, filter_extra.replace(" ", "\x00"), CONSENSUS_EXTRA.replace(" ", "\x00"), VARSCAN_EXTRA.replace(" ", "\x00")))
    monkeypatch.chdir(work)
    _run(line % "")
    work = pathlib.Path(str(work))
    assert not [name for name in os.listdir(str(work)) if "nj" in name]
    tables = {name: _read(work / name) for name in ("snp_distance_matrix.tsv", "snp_distance_matrix_preserved.tsv", "snpma.fasta", "snpma_preserved.fasta")}
    _run(line % "--nj")
    assert sorted(name for name in os.listdir(str(work)) if "nj" in name) == ["snp_nj.nwk", "snp_nj_preserved.nwk"]
    assert tables == {name: _read(work / name) for name in tables}
    for suffix in ("", "_preserved"):
        got = _read(work / ("snp_nj%s.nwk" % suffix))
        want_file = work / ("want%s.nwk" % suffix)
        _run("distance -f %s --amdNj %s" % (work / ("snpma%s.fasta" % suffix), want_file))
        assert got == _read(want_file)
        want, n = _want(work / ("snp_distance_matrix%s.tsv" % suffix))                   # ... and the statement on the table the job wrote
        assert n == 7 and got == want
