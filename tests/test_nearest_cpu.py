"""The statement of the nearest-neighbour output (tests/nearest_cases.py) pinned against the reference's own table and the
site-by-site oracle, the host writer of the file, and the global errors of ``distance --amdQuery / --amdNearest``, which must
reach the user before a device is needed.  No GPU."""
import itertools
import os

import numpy as np
import pytest

from oracle import distance_ref as dr
from tests import clusters_cases as cc
from tests import nearest_cases as nc


@pytest.fixture(scope="module")
def listeria(fixture_trees):
    tree = fixture_trees["listeria"][0]
    ids, mat = cc.read_matrix_tsv(os.path.join(tree, "snp_distance_matrix.tsv"))
    fasta_ids, rows = nc.read_fasta_rows(os.path.join(tree, "snpma.fasta"))
    assert fasta_ids == ids and len(ids) == 48
    mat.setflags(write=False)
    return ids, rows, mat


def test_rect_distance_gives_the_rows_of_the_reference_table(listeria):
    ids, rows, mat = listeria
    assert np.array_equal(nc.rect_distance(rows[::3], rows), mat[::3])
    assert np.array_equal(nc.rect_distance(rows, rows[5:9]), mat[:, 5:9])


@pytest.mark.parametrize("every_byte", [False, True])
def test_rect_distance_is_the_off_diagonal_block_of_the_square_statement(every_byte):
    q_sym, db_sym = nc.random_symbols(7, 301, 11, every_byte), nc.random_symbols(19, 301, 12, every_byte)
    if not every_byte:
        assert all((np.concatenate((q_sym, db_sym)) == b).any() for b in b"acgt-N")
    square = dr.row_loop(np.concatenate((q_sym, db_sym)))
    got = nc.rect_distance(q_sym, db_sym)
    assert got.shape == (7, 19) and np.array_equal(got, square[:7, 7:]) and got.max() > 0
    assert nc.rect_distance(q_sym[:0], db_sym).shape == (0, 19) and nc.rect_distance(q_sym, db_sym[:0]).shape == (7, 0)


def _brute(mat, k, t):
    rows = []
    for i in range(mat.shape[0]):
        order = sorted(range(mat.shape[1]), key=lambda j: (int(mat[i, j]), j))
        order = [j for j in order if t is None or mat[i, j] <= t]
        rows.append(order[:k] if k else order)
    return rows


@pytest.mark.parametrize("kind", ["two", "equal"])
def test_nearest_of_matrix_is_the_sorted_brute_force(kind):
    rng = np.random.default_rng(3)
    mat = rng.integers(0, 2, size=(5, 37)).astype(np.int32) * 9 - 4 if kind == "two" else np.full((5, 37), 6, dtype=np.int32)
    for k in (0, 1, 2, 36, 37, 42):
        for t in (None, -5, -4, 5, 6, nc.INT_MAX):
            row_off, col, dist = nc.nearest_of_matrix(mat, k, t)
            want = _brute(mat, k, t)
            assert [int(x) for x in row_off] == [0] + list(np.cumsum([len(r) for r in want]))
            assert [int(c) for c in col] == [j for r in want for j in r]
            assert [int(x) for x in dist] == [int(mat[i, j]) for i, r in enumerate(want) for j in r]
    row_off, col, dist = nc.nearest_of_matrix(np.full((2, 9), 6, dtype=np.int32), 4, None)
    assert list(col) == [0, 1, 2, 3, 0, 1, 2, 3]                     # an all-equal row keeps its first columns


def test_the_listeria_table_pins_the_tie_rule(listeria):
    ids, rows, mat = listeria
    assert [nc.ties_across_the_cut(mat, k) for k in (1, 3, 5)] == [30, 43, 36]
    for k in (1, 3, 5):
        row_off, col, dist = nc.nearest_of_matrix(mat, k)
        assert list(np.diff(row_off.astype(np.int64))) == [k] * 48
        for i in range(48):
            c, d = col[i * k:(i + 1) * k], dist[i * k:(i + 1) * k]
            assert list(d) == sorted(d) and all(mat[i, j] == x for j, x in zip(c, d))
            rest = np.delete(np.arange(48), c)
            # whatever was left out is farther, or as far and behind every kept sample of that distance
            assert all(mat[i, j] > d[-1] or (mat[i, j] == d[-1] and j > c[-1]) for j in rest)
    text = nc.nearest_text(ids[::3], ids, nc.nearest_of_matrix(mat[::3], 3, 20))
    assert text.startswith(nc.HEADER + "%s\t%s\t0\n" % (ids[0], ids[0])) and text.count("\n") <= 1 + 16 * 3


def test_the_writer_gives_the_text_of_the_statement(tmp_path):
    from snp_pipeline_amd import distance
    rng = np.random.default_rng(5)
    mat = rng.integers(-3, 40, size=(6, 11)).astype(np.int32)
    q_ids, db_ids = ["q%d" % i for i in range(6)], ["sé%d" % j for j in range(11)]
    path = str(tmp_path / "n.tsv")
    for k, t in ((0, None), (3, None), (0, 7), (2, -4)):
        csr = nc.nearest_of_matrix(mat, k, t)
        distance.write_nearest(path, q_ids, db_ids, *csr)
        with open(path, "rb") as f:
            assert f.read().decode("utf-8") == nc.nearest_text(q_ids, db_ids, csr)
    distance.write_nearest(path, [], db_ids, [0], [], [])
    with open(path) as f:
        assert f.read() == nc.HEADER
    # enough entries for the writer's threads (over 2^22): the block offsets must add up.  Rows of 0 ... all database samples, ids
    # of unequal byte lengths, distances from negative to 10 digits
    n_db = 2100
    db_ids = ["d" * (j % 7) + "%d" % j for j in range(n_db)]
    db_ids[5] = "dé5"
    lens = np.arange(2 * (n_db + 1)) % (n_db + 1)
    q_ids = ["query%d" % i if i % 3 else "q%d" % i for i in range(len(lens))]
    row_off = np.concatenate(([0], np.cumsum(lens))).astype(np.uint64)
    total = int(row_off[-1])
    assert total > 1 << 22 and lens[0] == 0 and lens[-1] == n_db
    col = rng.integers(0, n_db, size=total).astype(np.uint32)
    dist = np.minimum(rng.integers(1, 10, size=total) * 10 ** rng.integers(0, 10, size=total), 2 ** 31 - 1) * rng.choice([-1, 1], size=total)
    dist[:2] = 0, -(2 ** 31)
    distance.write_nearest(path, q_ids, db_ids, row_off, col, dist)
    db_field = np.asarray(["\t%s\t" % name for name in db_ids], dtype=object)
    rows = zip(np.repeat(np.asarray(q_ids, dtype=object), lens).tolist(), db_field[col].tolist(), map(str, dist.tolist()), itertools.repeat("\n"))
    with open(path, "rb") as f:
        assert f.read().decode("utf-8") == nc.HEADER + "".join(map("".join, rows))
    with pytest.raises(ValueError):
        distance.write_nearest(path, ["a"], ["b"], [0, 1], [1], [0])          # a column outside the database
    with pytest.raises(IOError):
        distance.write_nearest(str(tmp_path / "no_such_dir" / "n.tsv"), ["a"], ["b"], [0, 1], [0], [0])


def test_query_rows_keep_the_last_record_in_sorted_order():
    from snp_pipeline_amd import distance
    sym = np.frombuffer(b"ACGTAAAACCCCGGGG", dtype=np.uint8).reshape(4, 4)
    ids, rows = distance.query_rows(["b", "a", "b", "c"], sym, np.full(4, 4, dtype=np.uint64), 4)
    assert ids == ["a", "b", "c"] and rows.tobytes() == b"AAAACCCCGGGG"
    ids, rows = distance.query_rows([], np.zeros((0, 0), dtype=np.uint8), np.zeros(0, dtype=np.uint64), 4)
    assert ids == [] and rows.shape == (0, 4)


def test_new_options_keep_the_reference_namespace():
    from snp_pipeline_amd import cfsan_snp_pipeline as cli
    plain = vars(cli.parse_command_line("distance -p p.tsv x.fasta"))
    full = vars(cli.parse_command_line("distance -p p.tsv x.fasta --amdQuery q.fasta --amdNearest n.tsv --amdNearestCount 5 --amdMaxPairDistance 9"))
    added = {"amdQueryFile", "amdNearestFile", "amdNearestCount"}
    assert added <= set(full) and set(full) == set(plain) and all(plain[k] is None for k in added)
    assert (full["amdQueryFile"], full["amdNearestFile"], full["amdNearestCount"]) == ("q.fasta", "n.tsv", 5)
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
    query = tmp_path / "query.fasta"
    query.write_text(">x\nACGT\n>y\nACG\n>y\nACGTA\n")
    out = str(tmp_path / "out.tsv")
    for line, msg in (("distance %s --amdQuery %s" % (fasta, query), "--amdQuery and --amdNearest go together"),
                      ("distance %s --amdNearest %s" % (fasta, out), "--amdQuery and --amdNearest go together"),
                      ("distance %s -p %s --amdNearestCount 3" % (fasta, out), "--amdNearestCount needs --amdQuery and --amdNearest"),
                      ("distance %s --amdQuery %s --amdNearest %s --amdNearestCount -1" % (fasta, query, out), "--amdNearestCount cannot be negative"),
                      ("distance %s --amdQuery %s --amdNearest %s --amdMaxPairDistance -1" % (fasta, query, out), "a distance threshold cannot be negative"),
                      ("distance %s --amdQuery %s --amdNearest %s" % (fasta, tmp_path / "absent.fasta", out), "without the query file"),
                      ("distance %s --amdQuery %s --amdNearest %s" % (fasta, query, out), "the query y has 5 columns, the snp matrix has 4 columns"),
                      ("distance %s --amdNearestCount 3" % fasta, "--amdNearestCount needs --amdQuery and --amdNearest")):
        if log.exists():
            log.unlink()
        args = cli.parse_command_line(line)
        with pytest.raises(SystemExit) as ei:
            args.func(args)
        assert ei.value.code == 100, line
        assert msg in log.read_text(), line
        assert not os.path.exists(out)
    # no pair at all: the header, and still no device
    empty = tmp_path / "empty.fasta"
    empty.write_text("")
    for db, qf in ((fasta, empty), (empty, query)):
        args = cli.parse_command_line("distance -f %s --amdQuery %s --amdNearest %s" % (db, qf, out))
        args.verbose = 0
        args.func(args)
        with open(out) as f:
            assert f.read() == nc.HEADER
        os.remove(out)
    capsys.readouterr()
