"""Pins the statement of tests/nj_bootstrap_cases.py — the draws, the bipartitions, the counts and the percentages of the bootstrap
of the neighbour-joining tree — and checks the host text writers of the library (snpgpu_write_nj_newick_support,
snpgpu_write_nj_support) against its text.  Nothing here needs a GPU."""
import collections

import numpy as np
import pytest

from tests import nj_bootstrap_cases as bc
from tests import nj_cases as nc


def test_the_draws_are_the_pinned_numbers():
    s = 200000
    for (seed, b, k), value, col in (((1, 0, 0), 0x5e41ab087439611e, 73637), ((1, 0, 1), 0xf18d6ce93d6cf1ee, 188712), ((1, 1, 0), 0x778b1aa9c29bc868, 93393),
                                     ((0, 0, 0), 0xa706dd2f4d197e6f, 130489), ((2 ** 64 - 1, 7, 199999), 0xf9bb05c1acdd3844, 195101)):
        assert bc.draw(seed, b, k) == value and bc.column(seed, b, k, s) == col, (seed, b, k)
        assert int(bc.columns(seed, b, s)[k]) == col
    assert bc.columns(1, 0, 10).tolist() == [3, 9, 0, 7, 2, 7, 6, 2, 1, 2]
    assert bc.columns(1, 1, 10).tolist() == [4, 0, 0, 5, 3, 7, 4, 1, 7, 2]
    drawn = np.bincount(bc.columns(1, 0, 1000), minlength=1000)
    assert int((drawn == 0).sum()) == 360 and int(drawn.max()) == 5


def test_a_column_is_below_the_column_count_at_both_ends():
    top = 2 ** 32 - 1
    for seed in (0, 1, 2 ** 64 - 1):
        for b in (0, 7):
            assert all(bc.column(seed, b, k, 1) == 0 for k in range(50))
            assert all(0 <= bc.column(seed, b, k, top) < top for k in list(range(50)) + [top - 1])
            assert bc.columns(seed, b, 1).tolist() == [0] and bc.columns(seed, b, 0).size == 0
    assert (bc.MASK * top) >> 64 == top - 1                         # the largest draw there is
    assert [int(x) for x in bc.columns(5, 3, 70001)[::997]] == [bc.column(5, 3, k, 70001) for k in range(0, 70001, 997)]    # the array form is the definition


@pytest.mark.parametrize("n", [4, 5, 64, 65])
def test_every_tree_has_its_distinct_canonical_bipartitions(n):
    for name, make in nc.MATRICES.items():
        merges = nc.nj_numpy(make(n))[0]
        sets = bc.splits(n, merges)
        assert len(sets) == n - 3 == len(set(sets)), name
        for x in sets:
            assert not x & 1 and x >> n == 0 and 2 <= bin(x).count("1") <= n - 2, name
        rows = bc.split_words(n, sets)
        assert rows.shape == (n - 3, bc.words(n)) and [sum(int(v) << (64 * k) for k, v in enumerate(r)) for r in rows] == sets


def test_the_percent_table():
    want = {1: [0, 100, 0, 100], 3: [0, 33, 33, 100], 8: [0, 13, 50, 100], 1000: [0, 0, 50, 100]}
    for replicates, row in want.items():
        assert [bc.percent(c, replicates) for c in (0, 1, replicates // 2, replicates)] == row
    assert [bc.percent(c, 8) for c in range(9)] == [0, 13, 25, 38, 50, 63, 75, 88, 100]      # .5 goes up


def test_the_statement_separates_strong_from_weak_data():
    tree, counts = bc.planted_bootstrap()
    assert len(counts) == 94 and sorted(set(counts)) == list(range(9))
    assert tree == nc.nj_numpy(bc.distance_matrix(bc.planted()))
    sym = bc.additive_symbols()
    assert sym.shape == (65, 7400)
    assert bc.additive_bootstrap()[1] == [8] * 62
    other = bc.differing_seed()
    assert other != 1 and bc.planted_bootstrap(other)[0] == tree and bc.planted_bootstrap(other)[1] != counts


def test_a_replicate_does_not_depend_on_the_order_of_its_columns():
    sym = bc.planted()
    cols = bc.columns(1, 0, sym.shape[1])
    assert np.array_equal(bc.distance_matrix(sym[:, cols]), bc.distance_matrix(sym[:, np.sort(cols)]))
    weight = np.bincount(cols, minlength=sym.shape[1])
    differ = (sym[0] != sym[1]).astype(np.int64)
    assert int(bc.distance_matrix(sym[:2][:, cols])[0, 1]) == int((differ * weight).sum())


# ---- the host writers ------------------------------------------------------------------------------------------------------------
def _read(path):
    with open(path, "rb") as f:
        return f.read().decode("utf-8")


def _counts(k, replicates, seed):
    rng = np.random.default_rng(seed)
    counts = [int(x) for x in rng.integers(0, replicates + 1, size=k)]
    if k >= 2:
        counts[0], counts[-1] = 0, replicates                          # both ends of the range
    return counts


def _write_both(tmp_path, ids, tree, counts, replicates):
    from snp_pipeline_amd import distance
    nwk, tsv = str(tmp_path / "t.nwk"), str(tmp_path / "t.tsv")
    arrays = nc.arrays(tree)
    support = np.asarray(counts, dtype=np.uint32)
    distance.write_nj(nwk, ids, *arrays, support=support, replicates=replicates)
    distance.write_nj_support(tsv, ids, arrays[0], arrays[1], support, replicates)
    return _read(nwk), _read(tsv)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, 97])
def test_the_writers_give_the_text_of_the_statement(tmp_path, n):
    from snp_pipeline_amd import distance
    ids = ["s%02d" % i for i in range(n)]
    for high, replicates in ((40, 8), (3, 1), (9, 1000)):
        tree = nc.nj_numpy(nc.random_matrix(n, n + high, high=high))
        counts = _counts(max(n - 3, 0), replicates, n + high)
        nwk, tsv = _write_both(tmp_path, ids, tree, counts, replicates)
        assert nwk == bc.newick_support_text(ids, tree, counts, replicates), (n, high)
        assert tsv == bc.support_table_text(ids, tree[0], counts, replicates), (n, high)
        assert tsv.count("\n") == 1 + max(n - 3, 0) and tsv.startswith("Seq1\tSeq2\tSize\tSupport\tReplicates\n")
        plain = str(tmp_path / "plain.nwk")
        distance.write_nj(plain, ids, *nc.arrays(tree))
        if n <= 3:
            assert nwk == _read(plain)                                # nothing carries a value
        else:
            assert nwk != _read(plain) and nwk.count(")") == _read(plain).count(")") == n - 2
    if n == 97:
        assert nc.negative_lengths(tree) >= 1                         # negative lengths stand behind a value as they stand behind ')'


def test_quoted_ids_negative_lengths_and_both_ends_of_the_range(tmp_path):
    tree = ([(1, 3, nc.ONE, 2 * nc.ONE), (0, 1, 0, 5 * nc.ONE)], (0, 2, 4), (-(nc.ONE >> 4), nc.ONE, 15 * nc.ONE >> 1))
    ids = ["a", "b c", "it's", "d", "e"]
    nwk, tsv = _write_both(tmp_path, ids, tree, [0, 3], 3)
    assert nwk == "((a:0,('b c':1,d:2)0:5)100:-0.0625,'it''s':1,e:7.5);\n" == bc.newick_support_text(ids, tree, [0, 3], 3)
    assert tsv == "Seq1\tSeq2\tSize\tSupport\tReplicates\nb c\td\t2\t0\t3\na\tb c\t3\t3\t3\n" == bc.support_table_text(ids, tree[0], [0, 3], 3)
    nwk, _ = _write_both(tmp_path, ids, tree, [1, 2], 3)
    assert nwk == "((a:0,('b c':1,d:2)33:5)67:-0.0625,'it''s':1,e:7.5);\n"
    # the statement's own example of the grammar
    tree = ([(0, 1, nc.ONE, 2 * nc.ONE)], (0, 2, 3), (nc.ONE >> 1, nc.ONE, nc.ONE))
    assert _write_both(tmp_path, ["s1", "s2", "s3", "s4"], tree, [7], 8)[0] == "((s1:1,s2:2)88:0.5,s3:1,s4:1);\n"


def test_what_is_no_tree_or_no_count_is_refused_and_an_unwritable_path_is_an_io_error(tmp_path):
    from snp_pipeline_amd import _lib as L
    from snp_pipeline_amd import distance
    ids = ["a", "b", "c", "d", "e"]
    good = ([(1, 3, 1, 2), (0, 1, 0, 5)], (0, 2, 4), (1, 1, 7))
    path = str(tmp_path / "x")
    a, b = nc.arrays(good)[:2]
    for counts, replicates in (([0, 4], 3), ([0, 1], 0), ([0], 3), ([0, 1, 2], 3), ([0, 1], None)):
        with pytest.raises(ValueError):
            distance.write_nj(path, ids, *nc.arrays(good), support=np.asarray(counts, dtype=np.uint32), replicates=replicates)
        with pytest.raises(ValueError):
            distance.write_nj_support(path, ids, a, b, np.asarray(counts, dtype=np.uint32), replicates)
    for merges, star in (([(1, 3, 1, 2), (0, 3, 0, 5)], (0, 2, 4)), ([(3, 1, 1, 2), (0, 1, 0, 5)], (0, 2, 4)), ([(1, 5, 1, 2), (0, 1, 0, 5)], (0, 2, 4))):
        bad = nc.arrays((merges, star, (1, 1, 7)))
        with pytest.raises(ValueError):
            distance.write_nj(path, ids, *bad, support=[1, 1], replicates=2)
        with pytest.raises(ValueError):
            distance.write_nj_support(path, ids, bad[0], bad[1], [1, 1], 2)
    with pytest.raises(ValueError):
        distance.write_nj_support(path, ids[:4], a, b, [1, 1], 2)       # four samples have one join
    for call in (lambda p: distance.write_nj(p, ids, *nc.arrays(good), support=[1, 2], replicates=2), lambda p: distance.write_nj_support(p, ids, a, b, [1, 2], 2)):
        with pytest.raises(IOError):
            call(str(tmp_path / "no_such_dir" / "x"))
    # ... and the codes of the library itself
    lib = L.load()
    blob, off = distance._id_table(ids)
    la, lb = nc.arrays(good)[2:4]
    star, star_len = np.asarray([0, 2, 4], dtype=np.uint32), np.asarray([1, 1, 7], dtype=np.int64)
    support = np.asarray([1, 2], dtype=np.uint32)
    unwritable = str(tmp_path / "no_such_dir" / "x").encode()
    assert lib.snpgpu_write_nj_newick_support(unwritable, blob, off.ctypes.data, 5, a.ctypes.data, b.ctypes.data, la.ctypes.data, lb.ctypes.data, 2, star.ctypes.data,
                                              star_len.ctypes.data, support.ctypes.data, 2) == L.E_IO
    assert lib.snpgpu_write_nj_support(unwritable, blob, off.ctypes.data, 5, a.ctypes.data, b.ctypes.data, 2, support.ctypes.data, 2) == L.E_IO
    assert lib.snpgpu_write_nj_support(path.encode(), blob, off.ctypes.data, 5, a.ctypes.data, b.ctypes.data, 2, None, 2) == L.E_ARG
    assert lib.snpgpu_write_nj_support(path.encode(), blob, off.ctypes.data, 5, a.ctypes.data, b.ctypes.data, 2, support.ctypes.data, 1) == L.E_ARG


def test_the_new_symbols_are_declared_and_the_abi_stays():
    import os
    from snp_pipeline_amd import _lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "snpgpu.h")).read()
    lib = L.load()
    for name in ("snpgpu_bootstrap_columns_dev", "snpgpu_bootstrap_columns_sorted_dev", "snpgpu_resample_packed_dev", "snpgpu_nj_splits_dev", "snpgpu_split_support_dev", "snpgpu_nj_bootstrap",
                 "snpgpu_write_nj_newick_support", "snpgpu_write_nj_support"):
        assert name in L.SIGNATURES and ("  %s(" % name) in header and hasattr(lib, name), name
    assert lib.snpgpu_abi_version() == 7


def test_the_new_options_keep_the_reference_namespace_and_fail_before_a_device(tmp_path):
    """Every misuse of the three options is a global error raised before a device is asked for, and leaves no output file."""
    from snp_pipeline_amd import cfsan_snp_pipeline as cli
    from snp_pipeline_amd import distance
    plain = vars(cli.parse_command_line("distance -p p.tsv -m m.tsv x.fasta"))
    full = vars(cli.parse_command_line("distance -p p.tsv x.fasta --amdNj t.nwk --amdNjBootstrap 100 --amdNjSeed 18446744073709551615 --amdNjSupport s.tsv"))
    assert set(full) == set(plain) and (plain["amdNjBootstrap"], plain["amdNjSeed"], plain["amdNjSupportFile"]) == (None, None, None)
    assert (full["amdNjBootstrap"], full["amdNjSeed"], full["amdNjSupportFile"]) == (100, 2 ** 64 - 1, "s.tsv")
    fasta = tmp_path / "snpma.fasta"
    fasta.write_text("".join(">s%d\n%s\n" % (i, "ACGT"[i % 4] * 8) for i in range(5)))
    out = tmp_path / "out"
    out.mkdir()
    nj, sup, m = out / "nj", out / "sup", out / "m"
    for line in ("--amdNjSupport %s" % sup, "--amdNjSupport %s --amdNj %s" % (sup, nj), "--amdNjBootstrap 4", "--amdNjBootstrap 4 -m %s" % m,
                 "--amdNj %s --amdNjSeed 3" % nj, "--amdNj %s --amdNjBootstrap 0" % nj, "--amdNj %s --amdNjBootstrap -2" % nj,
                 "--amdNj %s --amdNjBootstrap 4 --amdNjSeed -1" % nj, "--amdNjSupport %s --amdNjBootstrap 4 --amdNjSeed 18446744073709551616" % sup):
        with pytest.raises(SystemExit) as ei:
            distance.calculate_snp_distances(cli.parse_command_line("distance -f %s %s" % (fasta, line)))
        assert ei.value.code == 100 and collections.Counter(p.name for p in out.iterdir()) == {}, line
