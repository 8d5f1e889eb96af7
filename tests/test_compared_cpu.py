"""The statement of the compared-site counts (tests/compared_cases.py) pinned against a brute-force loop and the bundled listeria
matrix, the host writer of the four-column pair files, and the options of ``distance --amdComparedMatrix / --amdCompared``, whose
errors must reach the user before a device is needed.  No GPU."""
import itertools
import os

import numpy as np
import pytest

from tests import clusters_cases as cc
from tests import compared_cases as pc
from tests import nearest_cases as nc


@pytest.fixture(scope="module")
def listeria(fixture_trees):
    tree = fixture_trees["listeria"][0]
    ids, mat = cc.read_matrix_tsv(os.path.join(tree, "snp_distance_matrix.tsv"))
    fasta_ids, rows = nc.read_fasta_rows(os.path.join(tree, "snpma.fasta"))
    assert fasta_ids == ids and len(ids) == 48
    return ids, rows, mat


def test_the_statement_is_the_brute_force_double_loop():
    sym = pc.random_symbols(7, 50, 3)
    sym[1, :8] = np.frombuffer(b"acgtnN-.", dtype=np.uint8)
    sym[2, 5:12] = (0x80, 0xC1, 0xE1, 0xFF, 0x41 + 0x80, 0x00, 0x7B)       # bytes that are letters only after losing a bit, '{'
    sym[3] = 0x2D
    assert all((sym == b).any() for b in b"ACGTacgt-N") and (sym >= 0x80).any()

    def valid(c):
        c = int(c)
        if 97 <= c <= 122:
            c -= 32
        return chr(c) in "ACGT"

    want = [[sum(1 for k in range(50) if valid(sym[i, k]) and valid(sym[j, k])) for j in range(7)] for i in range(7)]
    got = pc.compared_rect(sym, sym)
    assert got.dtype == np.int32 and got.tolist() == want and (got[3] == 0).all() and got.max() > 0
    assert np.array_equal(got, got.T) and np.array_equal(pc.compared_rect(sym[:3], sym[2:]), got[:3, 2:])
    assert np.array_equal(nc.rect_distance(sym, sym) <= got, np.ones((7, 7), dtype=bool))
    a, b = [0, 6, 3, 2, 2], [5, 6, 1, 4, 4]
    assert pc.compared_pairs(sym, a, b).tolist() == [want[i][j] for i, j in zip(a, b)]
    assert pc.compared_pairs(sym[:4], [3, 0], [0, 2], sym[4:]).tolist() == [want[3][4], want[0][6]]
    assert pc.compared_pairs(sym, [], []).shape == (0,) and pc.compared_rect(sym[:0], sym).shape == (0, 7)
    # the plane: bit i of word w is column 32 w + i, rows padded with zero words to whole slabs
    plane = pc.valid_plane(sym)
    assert plane.shape == (7, 16) and plane.dtype == np.dtype("<u4") and (plane[:, 2:] == 0).all()
    assert [[(int(plane[r, k // 32]) >> (k % 32)) & 1 for k in range(50)] for r in range(7)] == [[int(valid(c)) for c in row] for row in sym]
    assert [pc.plane_words(s) for s in (0, 1, 512, 513, 1024, 1025)] == [0, 16, 16, 32, 32, 48]


def test_the_listeria_matrix_holds_between_9974_and_10102_comparable_columns(listeria):
    ids, rows, mat = listeria
    assert rows.shape == (48, 10102)
    compared = pc.compared_rect(rows, rows)
    own = np.asarray([sum(1 for c in bytes(row).upper() if c in b"ACGT") for row in rows])
    assert np.array_equal(np.diag(compared), own) and own.min() == 9974 and own.max() == 10102
    assert (mat <= compared).all() and (compared <= np.minimum.outer(own, own)).all() and np.array_equal(compared, compared.T)
    assert np.array_equal(nc.rect_distance(rows, rows), mat)


def _written(tmp_path, *args):
    from snp_pipeline_amd import distance
    path = str(tmp_path / "rows.tsv")
    distance.write_pair_rows(path, *args)
    with open(path, "rb") as f:
        return f.read().decode("utf-8")


def test_the_writer_gives_the_text_of_the_statement(tmp_path):
    from snp_pipeline_amd import distance
    rng = np.random.default_rng(6)
    a_ids = ["q%d" % i for i in range(6)] + ["long_" + "x" * 3000, "séü"]
    b_ids = ["sé%d" % j for j in range(11)] + ["y" * 70000]
    for m in (0, 1, 5000):
        a, b = rng.integers(0, len(a_ids), size=m), rng.integers(0, len(b_ids), size=m)
        dist, compared = rng.integers(-3, 40, size=m), rng.integers(0, 2 ** 31 - 1, size=m)
        if m:
            a[0], b[0], dist[0], compared[0] = 6, 11, -(2 ** 31), 2 ** 31 - 1
        assert _written(tmp_path, a_ids, b_ids, a, b, dist, compared) == pc.pair_rows_text(a_ids, b_ids, a, b, dist, compared), m
        if m:                                                   # one table for both columns
            a %= len(b_ids)
            assert _written(tmp_path, b_ids, b_ids, a, b, dist, compared) == pc.pair_rows_text(b_ids, b_ids, a, b, dist, compared), m
    assert _written(tmp_path, [], [], [], [], [], []) == pc.HEADER == "Seq1\tSeq2\tDistance\tCompared\n"
    # enough rows for the writer's threads (over 2^22): the block offsets must add up.  Two id tables, both numbers of 1 ... 10 digits
    m = (1 << 22) + 1001
    a_tab, b_tab = ["q%d" % i for i in range(300)] + ["séü"], ["sample_%d" % (j * j) for j in range(77)]
    a, b = rng.integers(0, len(a_tab), size=m), rng.integers(0, len(b_tab), size=m)
    dist, compared = (np.minimum(rng.integers(1, 10, size=m) * 10 ** rng.integers(0, 10, size=m), 2 ** 31 - 1) for _ in range(2))
    fields = [(np.asarray(t, dtype=object) + "\t")[x].tolist() for t, x in ((a_tab, a), (b_tab, b))] + [map(str, dist.tolist()), map(str, compared.tolist())]
    rows = zip(fields[0], fields[1], fields[2], itertools.repeat("\t"), fields[3], itertools.repeat("\n"))
    assert _written(tmp_path, a_tab, b_tab, a, b, dist, compared) == pc.HEADER + "".join(map("".join, rows))
    # the three writers with the fourth column: the rows of the three-column file and one more field
    mat = rng.integers(0, 40, size=(6, 11)).astype(np.int32)
    csr = nc.nearest_of_matrix(mat, 3, 30)
    counts = rng.integers(0, 999, size=len(csr[1]))
    path = str(tmp_path / "n.tsv")
    distance.write_nearest(path, a_ids[:6], b_ids[:11], *csr, compared=counts)
    with open(path, "rb") as f:
        assert f.read().decode("utf-8") == pc.with_fourth_column(nc.nearest_text(a_ids[:6], b_ids[:11], csr), counts)
    square = cc.filter_rows(mat[:, :6], 20)
    counts = rng.integers(0, 999, size=len(square[1]))
    distance.write_close_pairs(path, a_ids[:6], *square, compared=counts)
    with open(path, "rb") as f:
        assert f.read().decode("utf-8") == pc.with_fourth_column(cc.close_pairs_text(a_ids[:6], mat[:, :6], 20), counts)
    distance.write_mst(path, a_ids[:6], [0, 2, 1], [5, 3, 4], [1, 2, 7], compared=[9, 8, 0])
    with open(path, "rb") as f:
        assert f.read().decode("utf-8") == pc.pair_rows_text(a_ids, a_ids, [0, 2, 1], [5, 3, 4], [1, 2, 7], [9, 8, 0])


def test_the_writer_refuses_an_index_outside_its_table(tmp_path):
    from snp_pipeline_amd import distance
    path = str(tmp_path / "bad.tsv")
    for a, b in (([2], [0]), ([0], [3]), ([0, 1, 0], [0, 2, 7])):
        with pytest.raises(ValueError):
            distance.write_pair_rows(path, ["a", "b"], ["x", "y", "z"], a, b, [0] * len(a), [0] * len(a))
        assert not os.path.exists(path)
    with pytest.raises(ValueError):
        distance.write_pair_rows(path, ["a"], ["x"], [0], [0], [1, 2], [1])
    with pytest.raises(IOError):
        distance.write_pair_rows(str(tmp_path / "no_such_dir" / "n.tsv"), ["a"], ["b"], [0], [0], [0], [4])


def test_new_options_keep_the_reference_namespace():
    from snp_pipeline_amd import cfsan_snp_pipeline as cli
    plain = vars(cli.parse_command_line("distance -p p.tsv x.fasta"))
    full = vars(cli.parse_command_line("distance -p p.tsv x.fasta --amdComparedMatrix c.tsv --amdCompared --amdClosePairs k.tsv --amdMaxPairDistance 9"))
    added = {"amdComparedMatrixFile", "amdCompared"}
    assert added <= set(full) and set(full) == set(plain)
    assert plain["amdComparedMatrixFile"] is None and plain["amdCompared"] is False
    assert (full["amdComparedMatrixFile"], full["amdCompared"]) == ("c.tsv", True)
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
    out = str(tmp_path / "out.tsv")
    needs = "--amdCompared needs at least one of --amdClosePairs, --amdMst and --amdNearest"
    for line, msg in (("distance %s --amdCompared -p %s" % (fasta, out), needs),
                      ("distance %s --amdCompared --amdComparedMatrix %s" % (fasta, out), needs),
                      ("distance %s --amdCompared --amdDendrogram %s" % (fasta, out), needs),
                      ("distance %s --amdCompared" % fasta, needs),
                      ("distance %s --amdCompared --amdClosePairs %s" % (fasta, out), "--amdClosePairs needs --amdMaxPairDistance"),
                      ("distance %s --amdComparedMatrix %s" % (tmp_path / "absent.fasta", out), "without the snp matrix file")):
        if log.exists():
            log.unlink()
        args = cli.parse_command_line(line)
        with pytest.raises(SystemExit) as ei:
            args.func(args)
        assert ei.value.code == 100, line
        assert msg in log.read_text(), line
        assert not os.path.exists(out)
    # nothing to count: the matrix of a file without records or without columns, and still no device
    empty = tmp_path / "empty.fasta"
    empty.write_text("")
    bare = tmp_path / "bare.fasta"
    bare.write_text(">b\n>a\n")
    for source, text in ((empty, "\t\n"), (bare, "\ta\tb\na\t0\t0\nb\t0\t0\n")):
        args = cli.parse_command_line("distance -f %s --amdComparedMatrix %s" % (source, out))
        args.verbose = 0
        args.func(args)
        with open(out) as f:
            assert f.read() == text == pc.matrix_text(*((["a", "b"], np.zeros((2, 2), dtype=int)) if source is bare else ([], [])))
        os.remove(out)
    capsys.readouterr()
