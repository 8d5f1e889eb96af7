"""The compared-site counts through the command: ``distance --amdComparedMatrix`` and ``--amdCompared`` on the bundled listeria
SNP matrix and on a small matrix with unequal lengths and an id twice, against the statement of tests/compared_cases.py."""
import os
import time

import numpy as np
import pytest

from tests import compared_cases as pc
from tests import nearest_cases as nc
from tests.test_gpu_distance_clusters_cli import _read, _run

pytestmark = pytest.mark.gpu


def _write_fasta(path, records):
    with open(str(path), "w") as f:
        for name, row in records:
            f.write(">%s\n%s\n" % (name, bytes(bytearray(row)).decode("latin-1")))


def _records(which, fixture_trees):
    """(records of the matrix, records of the queries), in file order."""
    if which == "listeria":
        ids, rows = nc.read_fasta_rows(os.path.join(fixture_trees["listeria"][0], "snpma.fasta"))
        assert rows.shape == (48, 10102)
        matrix = [(i, bytes(r)) for i, r in zip(ids, rows)]
        queries = [("new_%s" % ids[k], bytes(rows[k])) for k in reversed(range(0, 48, 5))] + [(ids[4], bytes(rows[7]))]
        return matrix, queries
    sym = pc.random_symbols(9, 700, 111)
    sym[3, 100:300] = 0x4E                                           # N
    names = ["s5", "s1", "s9", "s3", "s1", "s7", "s2", "s8", "s4"]   # s1 twice: the last record counts
    lens = {"s1": 640, "s2": 655, "s3": 655, "s4": 690, "s5": 700, "s7": 700, "s8": 700, "s9": 700}      # non-decreasing in sorted order
    matrix = [(name, bytes(sym[r, :lens[name]])) for r, name in enumerate(names)]
    q_sym = pc.random_symbols(4, 700, 112)
    q_sym[2] = sym[0]
    queries = [("q2", bytes(q_sym[0])), ("q1", bytes(q_sym[1])), ("s5", bytes(q_sym[2])), ("q1", bytes(q_sym[3]))]
    return matrix, queries


def _rows_with_compared(text, a_ids, b_ids, compared):
    """The statement's text of a three-column file with its fourth column: row (a, b) carries compared[a][b]."""
    a_of, b_of = {n: k for k, n in enumerate(a_ids)}, {n: k for k, n in enumerate(b_ids)}
    rows = [line.split("\t") for line in text.split("\n")[1:-1]]
    return pc.with_fourth_column(text, [compared[a_of[r[0]], b_of[r[1]]] for r in rows])


@pytest.mark.parametrize("which", ["listeria", "synthetic"])
def test_distance_writes_the_compared_counts(tmp_path, fixture_trees, which):
    """(Before the options existed argparse left with status 2 here.)"""
    matrix, queries = _records(which, fixture_trees)
    fasta, query = str(tmp_path / "snpma.fasta"), str(tmp_path / "query.fasta")
    _write_fasta(fasta, matrix)
    _write_fasta(query, queries)
    old = time.time() - 1000
    for path in (fasta, query):
        os.utime(path, (old, old))
    ids, sym = pc.sorted_rows_of_records(matrix)
    q_ids, q_sym = pc.sorted_rows_of_records(queries)
    compared, q_compared = pc.compared_rect(sym, sym), pc.compared_rect(q_sym, sym)
    dist = nc.rect_distance(sym, sym)
    assert (dist <= compared).all() and compared.min() < compared.max() and (compared != dist).all()
    if which == "synthetic":
        assert ids == ["s%d" % k for k in (1, 2, 3, 4, 5, 7, 8, 9)] and compared[0].max() <= 640 and compared[2, 2] <= 455

    # the matrix alone: nothing else is written
    alone = tmp_path / "alone"
    alone.mkdir()
    _run("distance %s --amdComparedMatrix %s" % (fasta, alone / "compared.tsv"))
    assert os.listdir(str(alone)) == ["compared.tsv"] and _read(alone / "compared.tsv") == pc.matrix_text(ids, compared)

    # next to the two tables: they are byte for byte what they are without the new option
    out, plain = tmp_path / "out", tmp_path / "plain"
    out.mkdir()
    plain.mkdir()
    _run("distance %s -p %s -m %s --amdComparedMatrix %s" % (fasta, out / "pairwise.tsv", out / "matrix.tsv", out / "compared.tsv"))
    _run("distance %s -p %s -m %s" % (fasta, plain / "pairwise.tsv", plain / "matrix.tsv"))
    for name in ("pairwise.tsv", "matrix.tsv"):
        assert _read(out / name) == _read(plain / name)
    assert _read(out / "compared.tsv") == pc.matrix_text(ids, compared) and _read(out / "matrix.tsv") == pc.matrix_text(ids, dist)

    # the three pair files with and without the fourth column
    t = 20 if which == "listeria" else 470
    files = "--amdClosePairs %s --amdMaxPairDistance %d --amdMst %s --amdQuery %s --amdNearest %s --amdNearestCount 3"
    c, m, n = (str(out / name) for name in ("close.tsv", "mst.tsv", "nearest.tsv"))
    line = "distance %s --amdCompared " % fasta + files % (c, t, m, query, n)
    _run(line)
    _run("distance %s " % fasta + files % (plain / "close.tsv", t, plain / "mst.tsv", query, plain / "nearest.tsv"))
    for name, a_ids, counts in (("close.tsv", ids, compared), ("mst.tsv", ids, compared), ("nearest.tsv", q_ids, q_compared)):
        without = _read(plain / name)
        assert without.count("\n") >= len(a_ids) and _read(out / name) == _rows_with_compared(without, a_ids, ids, counts), name
    close = _read(c).split("\n")
    assert all("%s\t%s\t0\t%d" % (i, i, compared[k, k]) in close for k, i in enumerate(ids))       # the diagonal rows: the own counts

    # the path that answers site files from a kept packed matrix carries the column as well
    _run("distance %s --amdCompared --amdMst %s --amdMstSites %s --amdClosePairs %s --amdMaxPairDistance %d" % (fasta, out / "mst2.tsv", out / "sites.tsv", out / "close2.tsv", t))
    assert _read(out / "mst2.tsv") == _read(m) and _read(out / "close2.tsv") == _read(c)

    # freshness: nothing is rewritten while the inputs are older; a missing file counts; -f rewrites
    k = str(out / "compared.tsv")
    both = line + " --amdComparedMatrix %s" % k
    wanted = {path: _read(path) for path in (c, m, n, k)}
    for path in wanted:
        with open(path, "w") as f:
            f.write("kept\n")
    _run(both)
    assert all(_read(path) == "kept\n" for path in wanted)
    os.remove(k)
    _run(both)
    assert all(_read(path) == text for path, text in wanted.items())
    with open(k, "w") as f:
        f.write("kept\n")
    _run("distance %s --amdComparedMatrix %s" % (fasta, k))
    assert _read(k) == "kept\n"
    _run("distance -f %s --amdComparedMatrix %s" % (fasta, k))
    assert _read(k) == wanted[k]


def test_the_error_cases_exit_100(tmp_path, monkeypatch, capsys):
    from snp_pipeline_amd import cfsan_snp_pipeline as cli
    log = tmp_path / "error.log"
    monkeypatch.setenv("errorOutputFile", str(log))
    fasta = tmp_path / "snpma.fasta"
    _write_fasta(fasta, [("a", b"ACGT"), ("b", b"ACG-")])
    out = str(tmp_path / "out.tsv")
    for line, msg in (("distance %s --amdCompared -m %s" % (fasta, out), "--amdCompared needs at least one of"),
                      ("distance %s --amdCompared --amdComparedMatrix %s" % (fasta, out), "--amdCompared needs at least one of"),
                      ("distance %s --amdCompared --amdNearest %s" % (fasta, out), "--amdQuery and --amdNearest go together"),
                      ("distance %s --amdComparedMatrix %s" % (tmp_path / "absent.fasta", out), "without the snp matrix file")):
        if log.exists():
            log.unlink()
        args = cli.parse_command_line(line)
        with pytest.raises(SystemExit) as ei:
            args.func(args)
        assert ei.value.code == 100, line
        assert msg in log.read_text(), line
        assert not os.path.exists(out)
    capsys.readouterr()
    _run("distance %s --amdComparedMatrix %s" % (fasta, out))
    assert _read(out) == "\ta\tb\na\t4\t3\nb\t3\t3\n"
