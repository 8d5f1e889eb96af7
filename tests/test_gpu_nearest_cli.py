"""The nearest-neighbour output through the command: ``distance --amdQuery / --amdNearest / --amdNearestCount`` on the bundled
listeria SNP matrix, against the statement of tests/nearest_cases.py applied to the reference's own distance table."""
import os
import shutil
import time

import numpy as np
import pytest

from tests import clusters_cases as cc
from tests import nearest_cases as nc
from tests.test_gpu_distance_clusters_cli import _read, _run

pytestmark = pytest.mark.gpu


def _write_fasta(path, records):
    with open(str(path), "w") as f:
        for name, row in records:
            f.write(">%s\n%s\n" % (name, bytes(bytearray(row)).decode("latin-1")))


def test_distance_writes_the_nearest_samples_alone_and_next_to_the_other_outputs(tmp_path, fixture_trees):
    """(Before the options existed argparse left with status 2 here.)"""
    tree_dir = fixture_trees["listeria"][0]
    fasta = str(tmp_path / "snpma.fasta")
    shutil.copyfile(os.path.join(tree_dir, "snpma.fasta"), fasta)
    ids, mat = cc.read_matrix_tsv(os.path.join(tree_dir, "snp_distance_matrix.tsv"))
    fasta_ids, rows = nc.read_fasta_rows(fasta)
    assert fasta_ids == ids

    # the queries: every third sample under a new name, out of order; one id twice (the last record counts); one id of the database
    picked = list(range(0, 48, 3))
    records = [("new_%s" % ids[i], rows[i]) for i in reversed(picked)]
    records += [("twice", rows[1]), (ids[4], rows[7]), ("twice", rows[2])]
    query = str(tmp_path / "query.fasta")
    _write_fasta(query, records)
    q_of = dict(("new_%s" % ids[i], i) for i in picked)
    q_of.update({"twice": 2, ids[4]: 7})
    q_ids = sorted(q_of)
    q_mat = mat[[q_of[name] for name in q_ids]]
    old = time.time() - 1000
    for path in (fasta, query):
        os.utime(path, (old, old))

    def want(k, t):
        return nc.nearest_text(q_ids, ids, nc.nearest_of_matrix(q_mat, k, t))

    assert want(3, None).count("\n") == 1 + 3 * len(q_ids) and "%s\t%s\t" % (ids[4], ids[7]) in want(1, None)

    # alone: nothing else is written
    alone = tmp_path / "alone"
    alone.mkdir()
    _run("distance %s --amdQuery %s --amdNearest %s --amdNearestCount 3" % (fasta, query, alone / "n3.tsv"))
    assert os.listdir(str(alone)) == ["n3.tsv"] and _read(alone / "n3.tsv") == want(3, None)
    _run("distance %s --amdQuery %s --amdNearest %s --amdNearestCount 5 --amdMaxPairDistance 20" % (fasta, query, alone / "n5.tsv"))
    assert _read(alone / "n5.tsv") == want(5, 20)
    _run("distance %s --amdQuery %s --amdNearest %s --amdMaxPairDistance 20" % (fasta, query, alone / "t20.tsv"))
    assert _read(alone / "t20.tsv") == want(0, 20)
    _run("distance %s --amdQuery %s --amdNearest %s" % (fasta, query, alone / "all.tsv"))
    assert _read(alone / "all.tsv") == want(0, None) and want(0, None).count("\n") == 1 + 48 * len(q_ids)

    # next to the tables and the tree: they are byte for byte what they are without the new options
    out, plain = tmp_path / "out", tmp_path / "plain"
    out.mkdir()
    plain.mkdir()
    p, m, t, n = (str(out / name) for name in ("pairwise.tsv", "matrix.tsv", "mst.tsv", "nearest.tsv"))
    line = "distance %s -p %s -m %s --amdMst %s --amdQuery %s --amdNearest %s --amdNearestCount 1" % (fasta, p, m, t, query, n)
    _run(line)
    _run("distance %s -p %s -m %s --amdMst %s" % (fasta, plain / "pairwise.tsv", plain / "matrix.tsv", plain / "mst.tsv"))
    for name in ("pairwise.tsv", "matrix.tsv", "mst.tsv"):
        assert _read(out / name) == _read(plain / name)
    assert _read(p) == _read(os.path.join(tree_dir, "snp_distance_pairwise.tsv")) and _read(n) == want(1, None)

    # freshness: nothing is rewritten while the inputs are older; a missing file counts; the query file is a source; -f rewrites
    for path in (p, m, t, n):
        with open(path, "w") as f:
            f.write("kept\n")
    _run(line)
    assert all(_read(path) == "kept\n" for path in (p, m, t, n))
    os.remove(n)
    _run(line)
    assert _read(n) == want(1, None)
    with open(n, "w") as f:
        f.write("kept\n")
    only = "distance %s --amdQuery %s --amdNearest %s --amdNearestCount 1" % (fasta, query, n)
    _run(only)
    assert _read(n) == "kept\n"
    _run("distance -f %s --amdQuery %s --amdNearest %s --amdNearestCount 1" % (fasta, query, n))
    assert _read(n) == want(1, None)
    with open(n, "w") as f:
        f.write("kept\n")
    now = time.time() + 10
    os.utime(query, (now, now))
    _run(only)
    assert _read(n) == want(1, None)


def test_empty_inputs_give_the_header(tmp_path, fixture_trees):
    tree_dir = fixture_trees["listeria"][0]
    fasta = str(tmp_path / "snpma.fasta")
    shutil.copyfile(os.path.join(tree_dir, "snpma.fasta"), fasta)
    empty = str(tmp_path / "empty.fasta")
    open(empty, "w").close()
    out = str(tmp_path / "n.tsv")
    _run("distance %s --amdQuery %s --amdNearest %s --amdNearestCount 2" % (fasta, empty, out))
    assert _read(out) == nc.HEADER
    os.remove(out)
    _run("distance %s --amdQuery %s --amdNearest %s" % (empty, fasta, out))
    assert _read(out) == nc.HEADER
    # a database without columns: every distance is 0, the first samples win
    _write_fasta(tmp_path / "db0.fasta", [("b", b""), ("a", b""), ("c", b"")])
    _write_fasta(tmp_path / "q0.fasta", [("x", b"")])
    _run("distance %s --amdQuery %s --amdNearest %s --amdNearestCount 2" % (tmp_path / "db0.fasta", tmp_path / "q0.fasta", out))
    assert _read(out) == nc.HEADER + "x\ta\t0\nx\tb\t0\n"
    assert np.array_equal(nc.nearest_of_matrix(np.zeros((1, 3), dtype=np.int32), 2)[1], [0, 1])
