"""The statement of tests/nj_cases.py pinned on itself (additive trees come back exactly, the closed form of the all-2 matrix, the
Python-integer form against the NumPy form, the range bound on every matrix the GPU tests use, the text of a length), and the host
code of the tree (snpgpu_write_nj_newick: the writer and the check of the records) against it — nothing here needs a GPU."""
import numpy as np
import pytest

from tests import nj_cases as nc

ONE = nc.ONE


@pytest.mark.parametrize("n", [3, 4, 5, 17, 64, 65, 130, 257])
def test_an_additive_tree_comes_back_exactly_and_without_a_negative_length(n):
    """Positive integer edge lengths: the fixed-point rounds recover every leaf-to-leaf distance, entry for entry."""
    for seed in ((1, 2, 3) if n <= 65 else (1,)):
        mat = nc.additive_tree(n, seed)
        tree = nc.nj_numpy(mat)
        assert len(tree[0]) == n - 3 and None not in tree[1]
        want = mat.astype(object) * ONE
        assert np.array_equal(nc.path_sums(n, tree), want), (n, seed)
        assert nc.negative_lengths(tree) == 0 and all(x % ONE == 0 for x in nc.all_lengths(tree)), (n, seed)
        if n <= 65:
            assert nc.nj(mat) == tree


def test_the_all_2_matrix_is_a_star_with_unit_leaves():
    for n in (4, 5, 8, 64, 130):
        want = nc.star_of_equal(n)
        assert nc.nj_numpy(nc.equal_matrix(n)) == want, n
        if n <= 64:
            assert nc.nj(nc.equal_matrix(n)) == want, n
        assert len(want[0]) == n - 3
    merges, star, star_len = nc.star_of_equal(6)
    assert merges == [(0, 1, ONE, ONE), (0, 2, 0, ONE), (0, 3, 0, ONE)] and star == (0, 4, 5) and star_len == (0, ONE, ONE)
    assert np.array_equal(nc.path_sums(6, (merges, star, star_len)), nc.equal_matrix(6).astype(object) * ONE)


def test_the_end_cases():
    assert nc.nj(np.zeros((0, 0), dtype=np.int32)) == nc.nj_numpy(np.zeros((0, 0), dtype=np.int32)) == ([], (None, None, None), (0, 0, 0))
    assert nc.nj(np.zeros((1, 1), dtype=np.int32)) == nc.nj_numpy(np.zeros((1, 1), dtype=np.int32)) == ([], (None, None, None), (0, 0, 0))
    two = np.array([[0, 7], [7, 0]], dtype=np.int32)
    assert nc.nj(two) == nc.nj_numpy(two) == ([], (0, 1, None), (7 * ONE // 2, 7 * ONE - 7 * ONE // 2, 0))
    three = np.array([[0, 3, 4], [3, 0, 5], [4, 5, 0]], dtype=np.int32)
    assert nc.nj(three) == nc.nj_numpy(three) == ([], (0, 1, 2), (ONE, 2 * ONE, 3 * ONE))
    # the floor goes towards minus infinity: (0 + 0 - 1) / 2 is -1/2
    odd = np.array([[0, 0, 0], [0, 0, 1], [0, 1, 0]], dtype=np.int32)
    assert nc.nj(odd)[2] == (-ONE // 2, ONE // 2, ONE // 2)
    # the diagonal is never read
    assert nc.nj(three + 9 * np.eye(3, dtype=np.int32)) == nc.nj(three)
    assert nc.refused(np.array([[0, -1], [-1, 0]])) and not nc.refused(np.array([[-5, 1], [1, -5]]))


def _cases():
    for seed in range(40):
        n = 4 + (seed * 7) % 23
        yield "random", nc.random_matrix(n, seed, high=40)
        yield "tied", nc.random_matrix(n, seed, high=3)
        yield "wide", nc.random_matrix(n, seed, high=1000)
    yield "planted", nc.planted_matrix(40, 300, 5)
    yield "planted", nc.planted_matrix(61, 200, 7, seed=3)
    yield "line", nc.line_matrix(33)
    yield "xor", nc.xor_matrix(32)
    yield "zero", nc.zero_matrix(9)
    yield "largest", nc.equal_matrix(4, nc.INT_MAX)


def test_the_python_integer_and_numpy_forms_agree():
    negative = 0
    for name, mat in _cases():
        n = mat.shape[0]
        slow, fast = nc.nj(mat), nc.nj_numpy(mat)
        assert slow == fast, (name, n)
        merges, star, star_len = slow
        assert len(merges) == n - 3 and all(a < b < n for a, b, _, _ in merges) and star == tuple(sorted(star))
        retired = [b for _, b, _, _ in merges]
        assert sorted(retired + list(star)) == list(range(n))       # every sample retires once or is in the star
        a, b, la, lb = merges[0]
        assert la + lb == int(mat[a][b]) * ONE                      # the two branches of the first join span its distance
        negative += nc.negative_lengths(slow)
    assert negative > 0                                             # lengths do go negative on matrices that are no trees


def test_no_working_value_grows_beyond_the_largest_entry():
    """What makes the sticky range flag of csrc/nj.hip a guard no test reaches: the update is half of a sum of two entries less a
    third."""
    for name, mat in _cases():
        *_, highest, lowest = nc.nj_numpy(mat, want_lowest=True)
        top = int(mat.max()) * ONE
        assert highest == top and lowest >= -top, name


# every matrix tests/test_gpu_nj.py gives to the device (nj_cases.MATRICES, by name and size)
GPU_CASES = [("random", n) for n in (0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257)] + [("ties3", n) for n in (3, 65, 130, 257)] + \
    [("line", 130), ("xor", 64), ("wide", 257), ("planted", 90), ("zero", 65), ("additive", 65), ("additive", 257), ("largest", 4), ("equal2", 130)]


@pytest.mark.parametrize("name,n", GPU_CASES)
def test_the_range_bound_holds_on_every_matrix_of_the_gpu_tests(name, n):
    """nj_numpy asserts |w| <= floor(2^61 / n) for every value it holds."""
    mat = np.asarray(nc.MATRICES[name](n))
    assert not nc.refused(mat)
    tree = nc.nj_numpy(mat)
    assert len(tree[0]) == max(n - 3, 0)


def test_the_range_bound_of_the_matrices_past_the_grid():
    """The all-2 matrix at 2 100 samples is checked against its closed form, in which no working value exceeds 2 << F; the
    all-INT32_MAX matrix is refused there and accepted at 4."""
    assert (2 << nc.F) <= nc.limit(2100) and not nc.refused(nc.equal_matrix(2100))
    assert nc.nj_numpy(nc.equal_matrix(130), want_lowest=True)[3:] == (2 * ONE, 0)
    assert nc.refused(nc.equal_matrix(2100, nc.INT_MAX)) and not nc.refused(nc.equal_matrix(4, nc.INT_MAX))
    assert (nc.INT_MAX << nc.F) <= nc.limit(1024) and (nc.INT_MAX << nc.F) > nc.limit(1025)


def test_the_text_of_a_length():
    assert nc.length(0) == "0" and nc.length(7 * ONE) == "7" and nc.length(7 * ONE + ONE // 2) == "7.5"
    assert nc.length(-ONE // 16) == "-0.0625" and nc.length(-3 * ONE) == "-3" and nc.length(-ONE // 2) == "-0.5"
    assert nc.length(1) == "0.000001"                                # 0.95 millionths: half up
    assert nc.length(-1) == "-0.000001" and nc.millionths(-1) == -1  # -0.95 millionths: floor(-0.95 + 0.5)
    assert nc.millionths(ONE // 2) == 500000 and nc.millionths(-ONE // 2) == -500000
    assert nc.length(nc.INT_MAX * ONE) == "2147483647" and nc.length(-nc.INT_MAX * ONE - 1) == "-2147483647.000001"
    assert nc.length(ONE // 3) == "0.333333" and nc.length(2 * ONE // 3) == "0.666666" and nc.length(2 * ONE // 3 + 1) == "0.666667"


def test_the_text_by_hand():
    ids = ["a", "b c", "it's", "d", "e"]
    assert nc.newick_text([], ([], (None,) * 3, (0,) * 3)) == ";\n"
    assert nc.newick_text(ids[1:2], ([], (None,) * 3, (0,) * 3)) == "'b c';\n"
    assert nc.newick_text(ids[:2], ([], (0, 1, None), (3 * ONE + ONE // 2, 3 * ONE + ONE // 2, 0))) == "(a:3.5,'b c':3.5);\n"
    assert nc.newick_text(ids[:3], ([], (0, 1, 2), (ONE, 2 * ONE, -ONE // 4))) == "(a:1,'b c':2,'it''s':-0.25);\n"
    tree = ([(1, 3, ONE, 2 * ONE), (0, 1, 0, 5 * ONE)], (0, 2, 4), (ONE // 2, ONE, 7 * ONE))
    assert nc.newick_text(ids, tree) == "((a:0,('b c':1,d:2):5):0.5,'it''s':1,e:7);\n"


def _read(path):
    with open(path, "rb") as f:
        return f.read().decode("utf-8")


def test_the_host_writer_against_the_statement(tmp_path):
    from snp_pipeline_amd import distance
    path = str(tmp_path / "out.nwk")
    odd = ["S_é", "two words", "it's", "par(en)", "under_score", "plain-1.2|x"]
    for n in (0, 1, 2, 3, 4, 5, 14, 40):
        ids = [odd[i % 7] + str(i) if i % 7 < 6 else "sample%d" % i for i in range(n)]
        for high in (1, 3, 1000):
            tree = nc.nj_numpy(nc.random_matrix(n, 100 + n + high, high=high))
            distance.write_nj(path, ids, *nc.arrays(tree))
            text = _read(path)
            assert text == nc.newick_text(ids, tree), (n, high)
            assert text.endswith(";\n") and text.count("\n") == 1
    tree = ([(1, 3, ONE, 2 * ONE), (0, 1, 0, 5 * ONE)], (0, 2, 4), (-ONE // 16, ONE, 7 * ONE + ONE // 2))
    distance.write_nj(path, ["a", "b c", "it's", "d", "e"], *nc.arrays(tree))
    assert _read(path) == "((a:0,('b c':1,d:2):5):-0.0625,'it''s':1,e:7.5);\n"
    for x in (0, 1, -1, ONE // 3, -ONE // 3, nc.INT_MAX * ONE, -nc.INT_MAX * ONE - 1, 2 ** 63 - 1, -2 ** 63):
        distance.write_nj(path, ["a", "b"], *nc.arrays(([], (0, 1, None), (x, 0, 0))))
        assert _read(path) == "(a:%s,b:0);\n" % nc.length(x), x


def test_a_chain_of_ten_thousand_joins_is_written_without_recursion(tmp_path):
    from snp_pipeline_amd import distance
    n = 10000
    ids = ["s%05d" % i for i in range(n)]
    tree = nc.star_of_equal(n)
    path = str(tmp_path / "chain.nwk")
    distance.write_nj(path, ids, *nc.arrays(tree))
    text = _read(path)
    assert text == nc.newick_text(ids, tree)
    assert text.startswith("(" * (n - 2) + "s00000:1,s00001:1):0,s00002:1):0,") and text.endswith(",s09997:1):0,s09998:1,s09999:1);\n")


def test_the_writer_refuses_what_is_not_a_tree_and_what_cannot_be_written(tmp_path):
    from snp_pipeline_amd import distance
    path = str(tmp_path / "out.nwk")
    ids = ["a", "b", "c", "d", "e"]
    good = ([(1, 3, 1, 2), (0, 1, 0, 5)], (0, 2, 4), (1, 1, 7))
    distance.write_nj(path, ids, *nc.arrays(good))
    for merges, star in (([(1, 3, 1, 2)], (0, 2, 4)),                               # too few merges
                         ([(1, 3, 1, 2), (0, 1, 0, 5), (0, 2, 1, 1)], (0, 4, None)),  # too many
                         ([(1, 3, 1, 2), (0, 3, 0, 5)], (0, 2, 4)),                 # slot 3 has retired
                         ([(1, 3, 1, 2), (3, 4, 0, 5)], (0, 1, 2)),                 # ... as the first of a pair
                         ([(3, 1, 1, 2), (0, 1, 0, 5)], (0, 2, 4)),                 # a > b
                         ([(1, 1, 1, 2), (0, 1, 0, 5)], (0, 2, 4)),                 # a = b
                         ([(1, 5, 1, 2), (0, 1, 0, 5)], (0, 2, 4)),                 # an index past n
                         ([(1, 3, 1, 2), (0, 1, 0, 5)], (0, 2, 3)),                 # a star slot that has retired
                         ([(1, 3, 1, 2), (0, 1, 0, 5)], (2, 0, 4)),                 # a star out of order
                         ([(1, 3, 1, 2), (0, 1, 0, 5)], (0, 2, None)),              # a star with a slot missing
                         ([(1, 3, 1, 2), (0, 1, 0, 5)], (0, 2, 7))):                # a star slot past n
        with pytest.raises(ValueError):
            distance.write_nj(path, ids, *nc.arrays((merges, star, (1, 1, 7))))
    for n, star in ((0, (0, None, None)), (1, (0, None, None)), (2, (0, None, None)), (2, (1, 0, None)), (2, (0, 1, 1)), (3, (0, 1, None))):
        with pytest.raises(ValueError):
            distance.write_nj(path, ids[:n], *nc.arrays(([], star, (1, 1, 1))))
    with pytest.raises(ValueError):
        distance.write_nj(path, ids, np.zeros(2, dtype=np.uint32), np.zeros(1, dtype=np.uint32), np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int64), (0, 2, 4), (1, 1, 7))
    with pytest.raises(IOError):
        distance.write_nj(str(tmp_path / "no_such_dir" / "x"), ids, *nc.arrays(good))


def test_the_new_option_keeps_the_reference_namespace():
    from snp_pipeline_amd import cfsan_snp_pipeline as cli
    plain = vars(cli.parse_command_line("distance -p p.tsv -m m.tsv x.fasta"))
    full = vars(cli.parse_command_line("distance -p p.tsv -m m.tsv x.fasta --amdNj tree.nwk"))
    assert "amdNjFile" in full and set(full) == set(plain) and plain["amdNjFile"] is None and full["amdNjFile"] == "tree.nwk"
    batch = vars(cli.parse_command_line("hot_path_batch dirs.txt ref.fasta --nj"))
    assert batch["nj"] is True and vars(cli.parse_command_line("hot_path_batch dirs.txt ref.fasta"))["nj"] is False
