"""The bootstrap of the neighbour-joining tree through the command: ``distance --amdNj --amdNjBootstrap --amdNjSeed --amdNjSupport``
against the statement of tests/nj_bootstrap_cases.py, byte for byte."""
import os

import numpy as np
import pytest

from tests import nj_bootstrap_cases as bc
from tests import nj_cases as nc
from tests.test_gpu_distance_clusters_cli import _read, _run
from tests.test_gpu_linkage_cli import _old_fasta

pytestmark = pytest.mark.gpu


def _fasta(tmp_path, n, columns=300):
    """A small SNP matrix whose records come in no sorted order and one of whose ids needs quoting.  Returns (path, the sorted ids,
    their rows)."""
    sym = nc.planted_symbols(n, columns, 4, seed=n)
    ids = ["sample%03d" % i for i in range(n)]
    ids[n // 2] = "odd name's"
    order = np.random.default_rng(n).permutation(n)
    path = tmp_path / "snpma.fasta"
    path.write_text("".join(">%s\n%s\n" % (ids[i], sym[i].tobytes().decode()) for i in order))
    old = os.path.getmtime(str(path)) - 1000
    os.utime(str(path), (old, old))
    by_id = sorted(range(n), key=lambda i: ids[i])
    return str(path), [ids[i] for i in by_id], np.ascontiguousarray(sym[by_id])


def _want(ids, sym, replicates, seed):
    tree, counts = bc.bootstrap(sym, replicates, seed)
    return nc.newick_text(ids, tree), bc.newick_support_text(ids, tree, counts, replicates), bc.support_table_text(ids, tree[0], counts, replicates)


@pytest.mark.parametrize("n", [9, 97])
def test_both_files_are_the_statement_alone_and_next_to_the_tables(tmp_path, n):
    """(Before the options existed argparse left with status 2 here.)"""
    fasta, ids, sym = _fasta(tmp_path, n)
    plain, nwk, tsv = _want(ids, sym, 6, 1)
    assert "'odd name''s'" in nwk and "odd name's\t" in tsv and nwk != plain

    alone = tmp_path / "alone"
    alone.mkdir()
    _run("distance %s --amdNj %s/nj --amdNjBootstrap 6 --amdNjSupport %s/sup" % (fasta, alone, alone))
    assert sorted(os.listdir(str(alone))) == ["nj", "sup"]
    assert _read(alone / "nj") == nwk and _read(alone / "sup") == tsv
    _run("distance -f %s --amdNjBootstrap 6 --amdNjSupport %s/only" % (fasta, alone))          # the table without the tree
    assert sorted(os.listdir(str(alone))) == ["nj", "only", "sup"] and _read(alone / "only") == tsv
    _run("distance -f %s --amdNj %s/seeded --amdNjBootstrap 6 --amdNjSeed 18446744073709551615" % (fasta, alone))
    assert _read(alone / "seeded") == _want(ids, sym, 6, 2 ** 64 - 1)[1]

    # next to the tables: their bytes are those of a run without the new options, and the tree is the same line
    before, after = tmp_path / "before", tmp_path / "after"
    before.mkdir()
    after.mkdir()
    _run("distance %s -p %s/p -m %s/m" % (fasta, before, before))
    _run("distance %s -p %s/p -m %s/m --amdNj %s/nj --amdNjBootstrap 6 --amdNjSupport %s/sup" % (fasta, after, after, after, after))
    assert sorted(os.listdir(str(after))) == ["m", "nj", "p", "sup"]
    for name in "pm":
        assert _read(after / name) == _read(before / name), name
    assert _read(after / "nj") == nwk and _read(after / "sup") == tsv

    # without --amdNjBootstrap the tree is the line it was
    _run("distance %s --amdNj %s/plain" % (fasta, before))
    assert _read(before / "plain") == plain
    _run("distance -f %s -m %s/m2 --amdNj %s/plain2" % (fasta, before, before))
    assert _read(before / "plain2") == plain and _read(before / "m2") == _read(before / "m")


def test_every_misuse_is_a_global_error_that_leaves_no_file(tmp_path):
    fasta, _, _ = _fasta(tmp_path, 9)
    out = tmp_path / "out"
    out.mkdir()
    for line in ("--amdNjSupport %s/s" % out, "--amdNjSupport %s/s --amdNj %s/t" % (out, out), "--amdNjBootstrap 4", "--amdNjBootstrap 4 -m %s/m" % out,
                 "--amdNj %s/t --amdNjSeed 3" % out, "--amdNj %s/t --amdNjBootstrap 0" % out, "--amdNj %s/t --amdNjBootstrap -1" % out,
                 "--amdNj %s/t --amdNjBootstrap 4 --amdNjSeed -1" % out, "--amdNj %s/t --amdNjBootstrap 4 --amdNjSeed 18446744073709551616" % out):
        with pytest.raises(SystemExit) as ei:
            _run("distance -f %s %s" % (fasta, line))
        assert ei.value.code == 100 and os.listdir(str(out)) == [], line


def test_the_listeria_fixture(tmp_path, fixture_trees):
    from snp_pipeline_amd import distance, snp_matrix
    tree_dir = fixture_trees["listeria"][0]
    fasta = _old_fasta(tmp_path, tree_dir)
    ids, sym = distance._sorted_rows(*snp_matrix.load_matrix(fasta))
    assert sym.shape == (48, 10102)
    plain, nwk, tsv = _want(ids, sym, 4, 1)
    out = tmp_path / "out"
    out.mkdir()
    _run("distance %s --amdNj %s/nj --amdNjBootstrap 4 --amdNjSupport %s/sup" % (fasta, out, out))
    assert _read(out / "nj") == nwk and _read(out / "sup") == tsv
    assert tsv.count("\n") == 1 + 45
    _run("distance %s --amdNj %s/plain" % (fasta, out))
    assert _read(out / "plain") == plain
    # topology and lengths are those of the tree alone: the line without what stands between ")" and ":"
    import re
    assert re.sub(r"\)\d+:", "):", nwk) == plain
