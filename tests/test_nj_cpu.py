"""The statement of tests/nj_cases.py pinned on itself (additive trees come back exactly, the closed form of the all-2 matrix, the
Python-integer form against the NumPy form, the range bound on every matrix the GPU tests use, the text of a length), and the host
code of the tree (snpgpu_write_nj_newick: the writer and the check of the records) against it — nothing here needs a GPU."""
import numpy as np
import pytest

from tests import nj_cases as nc
from tests import nj_geometry as ng

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


# ---- the checker of tests/nj_cases.py: check_tree, nj_prefix, far_cherries, compaction_rounds -------------------------------------
CHECKED = [(name, n) for name in sorted(nc.MATRICES) for n in (4, 5, 64, 65, 130)]      # ("largest" stays within 2^61 / n up to 1 024 samples)


def _matrix(name, n):
    return np.asarray(nc.MATRICES[name](n))


@pytest.mark.parametrize("name,n", CHECKED)
def test_check_tree_accepts_the_trees_of_both_forms_with_every_round_checked(name, n):
    """... and the incremental R of the replay is the statement's sum over the live slots in every round (summed_R)."""
    mat = _matrix(name, n)
    tree = nc.nj_numpy(mat)
    nc.check_tree(mat, tree, range(n - 3), summed_R=True)
    nc.check_tree(mat, tree)
    nc.check_tree(mat, nc.nj(mat), range(n - 3), summed_R=True)


def test_check_tree_accepts_the_smallest_trees_and_rejects_their_wrong_stars():
    for n in (0, 1, 2, 3):
        mat = nc.random_matrix(n, 5, high=40)
        tree = nc.nj(mat)
        nc.check_tree(mat, tree)
        if n >= 2:
            for s in range(n):
                lengths = list(tree[2])
                lengths[s] += 1
                with pytest.raises(AssertionError, match="the star"):
                    nc.check_tree(mat, (tree[0], tree[1], tuple(lengths)))
    with pytest.raises(AssertionError, match="joins"):
        nc.check_tree(nc.random_matrix(5, 5, high=40), ([], (0, 1, 2), (0, 0, 0)))


def _state_at(mat, merges, t):
    state = nc.Replay(mat)
    for a, b, _, _ in merges[:t]:
        state.join(a, b)
    return state


def _raises_in_round(mat, tree, rounds, t, what):
    with pytest.raises(AssertionError) as ei:
        nc.check_tree(mat, tree, rounds)
    assert str(ei.value).startswith("round %d: " % t) and what in str(ei.value), str(ei.value)


@pytest.mark.parametrize("name,n", [("random", 64), ("ties3", 65), ("wide", 130), ("additive", 65)])
def test_check_tree_rejects_every_single_change_and_names_the_round(name, n):
    mat = _matrix(name, n)
    merges, star, star_len = nc.nj_numpy(mat)
    every = range(n - 3)
    for t in (0, 1, n // 2, n - 5, n - 4):
        a, b, la, lb = merges[t]
        state = _state_at(mat, merges, t)
        # the second-best pair with the lengths that are right for it: only the choice is wrong
        best, second = state.ranked(2)
        assert best == (a, b)
        wrong = merges[:t] + [second + state.lengths(*second)] + merges[t + 1:]
        _raises_in_round(mat, (wrong, star, star_len), every, t, "the least (Q, i, j)")
        # a and b swapped
        _raises_in_round(mat, (merges[:t] + [(b, a, la, lb)] + merges[t + 1:], star, star_len), every, t, "not two live slots")
        # a length moved by one unit from one branch to the other
        _raises_in_round(mat, (merges[:t] + [(a, b, la + 1, lb - 1)] + merges[t + 1:], star, star_len), every, t, "the lengths")
        _raises_in_round(mat, (merges[:t] + [(a, b, la + 1, lb - 1)] + merges[t + 1:], star, star_len), (), t, "the lengths")
        # two consecutive joins exchanged: the later one is not the least of the earlier round (or names a slot that has retired)
        if t + 1 < n - 3:
            swapped = merges[:t] + [merges[t + 1], merges[t]] + merges[t + 2:]
            with pytest.raises(AssertionError) as ei:
                nc.check_tree(mat, (swapped, star, star_len), every)
            assert str(ei.value).startswith("round %d: " % t), str(ei.value)     # (on an additive matrix only the choice tells: the lengths of two cherries are right in either order)
    for s in range(3):
        lengths = list(star_len)
        lengths[s] -= 1
        with pytest.raises(AssertionError, match="the star"):
            nc.check_tree(mat, (merges, star, tuple(lengths)))
        retired = merges[-1][1]
        slots = list(star)
        slots[s] = retired
        with pytest.raises(AssertionError, match="the star"):
            nc.check_tree(mat, (merges, tuple(slots), star_len))


def test_a_record_changed_in_a_round_that_is_not_sampled_fails_a_later_length_check():
    """What makes sampling the argmin rounds sound against a corrupted state: every later round's lengths come from w(a,b), R(a) and
    R(b) of the replayed state, and a wrong join moves R of every live slot.  Here round t takes the second-best pair with the lengths
    that are right for it, so round t itself passes when it is no argmin round; the records behind it are the true tree's."""
    n = 96
    mat = nc.random_matrix(n, 21, high=40)
    merges, star, star_len = nc.nj_numpy(mat)
    for t in (0, 7, 40, 80):
        state = _state_at(mat, merges, t)
        best, second = state.ranked(2)
        assert best == merges[t][:2]
        wrong = merges[:t] + [second + state.lengths(*second)] + merges[t + 1:]
        sampled = set(range(0, n - 3, 32)) - {t} | {n - 4}
        with pytest.raises(AssertionError) as ei:
            nc.check_tree(mat, (wrong, star, star_len), sampled - {t})
        later = int(str(ei.value).split(":")[0].split()[1])
        assert str(ei.value).startswith("round ") and t < later <= t + 2, str(ei.value)


@pytest.mark.parametrize("name,n", [("random", 65), ("ties3", 130), ("equal2", 64), ("zero", 9)])
def test_the_prefix_is_the_head_of_the_tree(name, n):
    mat = _matrix(name, n)
    merges = nc.nj_numpy(mat)[0]
    for rounds in (0, 1, 8, n - 4, n - 3, n):
        assert nc.nj_prefix(mat, rounds) == merges[:rounds]


def test_the_planted_pairs_of_far_cherries_are_the_first_joins():
    small = [(0, 39), (1, 20), (5, 6), (37, 38)]
    for n, pairs in [(40, small)] + sorted(ng.CHERRIES.items()):
        mat = nc.far_cherries(n, ng.CHERRY_SEED, pairs)
        assert np.array_equal(mat, mat.T) and not mat.diagonal().any() and not nc.refused(mat)
        off = mat[~np.eye(n, dtype=bool)]
        assert sorted(np.unique(off).tolist()) == [1] + list(range(40, 61)) and int((off == 1).sum()) == 2 * len(pairs)
        head = nc.nj_prefix(mat, len(pairs) + 1)
        assert sorted(m[:2] for m in head[:len(pairs)]) == sorted(pairs), n
        assert head[len(pairs)][:2] not in pairs and all(m[2] + m[3] == nc.ONE for m in head[:len(pairs)])
    assert np.array_equal(nc.far_cherries(40, 7, small), nc.far_cherries(40, 7, small))
    assert not np.array_equal(nc.far_cherries(40, 7, small), nc.far_cherries(40, 8, small))


def test_the_planted_pairs_fall_where_the_loops_of_the_kernels_turn():
    """Written over the constants of csrc/nj.hip, so the conditions move with them."""
    c = ng.kernel_constants()
    turn = 2 * c["THREADS"] * c["UNROLL"]                            # the columns of one turn of k_nj_rows' outer loop
    assert turn == 2048 and c["PICK_THREADS"] == 1024 and c["ROW_GRID_CAP"] == 2048 and 0 < c["COMPACT_NUM"] < c["COMPACT_DEN"]
    for n, pairs in ng.CHERRIES.items():
        steps = {ng.row_step(i, k, c) for i, k in pairs}
        reachable = min(c["UNROLL"], (n - 1) // (2 * c["THREADS"]) + 1)       # the sub-steps a row of n columns has at all
        assert {u for turn_, u in steps if turn_ == 0} == set(range(reachable)), n
        assert {2, reachable - 1} <= {u for _, u in steps}
        assert any(i >= c["PICK_THREADS"] for i, _ in pairs)                  # a second row of a thread of k_nj_pick wins
        assert any(i >= n - 4 and k >= n - 2 for i, k in pairs)               # the last rows
        assert any(i <= 1 and k == n - 1 for i, k in pairs)                   # the first row against the last column
    pairs = ng.CHERRIES[2100]
    assert any(i <= 1 and k >= turn + 2 and ng.row_step(i, k, c)[0] == 1 for i, k in pairs)      # the second turn of the outer loop
    assert {ng.row_step(i, k, c)[1] for i, k in pairs if ng.row_step(i, k, c)[0] == 0} == {0, 1, 2, 3}
    assert any(i >= c["ROW_GRID_CAP"] for i, _ in pairs)                      # a row of the grid-stride turn
    assert any(3 in ng.row_step(i, k, c) for i, k in ng.CHERRIES[1600]) and any(i >= 1024 for i, _ in ng.CHERRIES[1600])


def test_the_compaction_rounds_are_those_of_the_host_loop():
    assert nc.compaction_rounds(16, 7, 8) == [(2, 16, 14), (4, 14, 12), (6, 12, 10), (8, 10, 8), (9, 8, 7), (10, 7, 6), (11, 6, 5), (12, 5, 4)]
    assert nc.compaction_rounds(3, 7, 8) == [] and nc.compaction_rounds(100, 0, 8) == []
    c = ng.kernel_constants()
    for n in (1100, 1600, 2100):
        rounds = nc.compaction_rounds(n, c["COMPACT_NUM"], c["COMPACT_DEN"])
        assert rounds[0][1] == n and all(x[2] == y[1] for x, y in zip(rounds, rounds[1:])) and all(0 < t < n - 3 for t, _, _ in rounds)
        assert all(after * c["COMPACT_DEN"] <= before * c["COMPACT_NUM"] < (after + 1) * c["COMPACT_DEN"] for _, before, after in rounds)
        assert all(before - after == t - s for (s, _, _), (t, before, after) in zip([(0, 0, 0)] + rounds, rounds))   # a round retires one slot
        assert rounds == ng.compactions(n)
        wanted = ng.argmin_schedule(n, 16, rounds)
        ng.assert_schedule(n, 16, rounds, wanted)
        assert len(wanted) >= 64 and all({t - 1, t, t + 1} <= wanted for t, _, _ in rounds if t + 1 < n - 3)
    with pytest.raises(AssertionError):                              # a schedule that dropped one round of a compaction is refused
        ng.assert_schedule(n, 16, rounds, wanted - {rounds[1][0] + 1})
    with pytest.raises(AssertionError):
        ng.assert_schedule(n, 16, rounds, wanted - {64})


def test_the_additive_matrix_by_rows_is_the_additive_matrix():
    for n in (3, 4, 5, 17, 65, 130):
        for seed in (1, 2, 7):
            assert np.array_equal(nc.additive_tree_by_rows(n, seed), nc.additive_tree(n, seed)), (n, seed)
    assert np.array_equal(nc.additive_tree_by_rows(40, 3, longest=3), nc.additive_tree(40, 3, longest=3))
    big = nc.additive_tree_by_rows(2100, 7)
    assert big.shape == (2100, 2100) and np.array_equal(big, big.T) and not big.diagonal().any() and not nc.refused(big)
    assert int(big[~np.eye(2100, dtype=bool)].min()) >= 2           # two leaves are at least two edges apart
