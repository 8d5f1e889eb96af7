"""The kernels of csrc/nj.hip past one turn of every loop, with values that tell positions apart: the later sub-steps and the second
turn of k_nj_rows' column loop, a thread's second row in k_nj_pick, several workgroups adding into R[a] in k_nj_update, the later column
turns and the grid-stride rows of k_nj_compact — where tests/test_gpu_nj.py only ever sends the all-2 matrix.  (Not here: the
compaction's exclusive scan past its first block of 8 192 positions; tests/test_gpu_analysis_edges.py takes the scan of prims.h there.)
Up to 769 samples the tree is compared with the statement whole.  Above, the statement is too slow (nj_numpy takes a minute at 2 100),
so its first rounds are compared exactly (nj_cases.nj_prefix) and the rest is replayed (nj_cases.check_tree): every record's slots and
lengths against the replayed state, the star, and the choice itself in the rounds of nj_geometry.argmin_schedule.  A state that goes
wrong in any round shows in the lengths behind it (tests/test_nj_cpu.py)."""
import functools

import numpy as np
import pytest

from tests import nj_cases as nc
from tests import nj_geometry as ng
from tests.gpu_util import get_device
from tests.test_gpu_nj import _tree

pytestmark = pytest.mark.gpu

KINDS = {
    "random": lambda n: nc.MATRICES["random"](n),
    "ties3": lambda n: nc.MATRICES["ties3"](n),
    "ties10": lambda n: nc.random_matrix(n, 3, high=10),             # entries below 10: ties abound
    "cherries": lambda n: nc.far_cherries(n, ng.CHERRY_SEED, ng.CHERRIES[n]),
    "additive": lambda n: nc.additive_tree_by_rows(n, 7),            # every length's division is exact: one unit too many in R(b) shows
}
LARGE = [(n, kind) for n in (1100, 1600) for kind in ("random", "ties3", "cherries")] + [(2100, "cherries"), (2100, "ties10"), (2100, "additive")]


@functools.lru_cache(maxsize=None)
def _matrix(kind, n):
    mat = np.ascontiguousarray(KINDS[kind](n), dtype=np.int32)
    mat.setflags(write=False)
    return mat


@functools.lru_cache(maxsize=None)
def _whole(kind, n):
    return nc.nj_numpy(_matrix(kind, n))


@pytest.mark.parametrize("kind", ["random", "ties3"])
@pytest.mark.parametrize("n", [513, 600, 769])
def test_mid_sizes_against_the_whole_statement(n, kind):
    """Past 512 columns the sub-step u = 1 of a row decides joins, three or four workgroups add into R[a], and the first compactions
    run at m > 512.  No column of these sizes reaches u = 2 (row 0 meets column 768 in u = 1): that is left to the cases from 1 100 on."""
    c = ng.kernel_constants()
    assert n > 2 * c["THREADS"] and (n + c["THREADS"] - 1) // c["THREADS"] >= 3
    assert ng.compactions(n, c)[0][1] > 512
    mat, want = _matrix(kind, n), _whole(kind, n)
    if n >= 600:                                                     # (at 513 row 0 alone has a column in u = 1)
        assert _reached(n, want[0])["step"] >= {(0, 0), (0, 1)}
    assert _tree(get_device(), mat) == want


def _reached(n, merges):
    """Which (turn, sub-step) of k_nj_rows' column loop met a joined pair, and the largest position of a joined row."""
    c = ng.kernel_constants()
    where = ng.join_positions(n, merges, ng.compactions(n, c))
    return {"step": {ng.row_step(a, b, c) for _, a, b in where}, "row": max(a for _, a, _ in where)}


def _schedule(n, kind):
    c = ng.kernel_constants()
    prefix = (len(ng.CHERRIES[n]) if kind == "cherries" else 0) + 8
    compactions = ng.compactions(n, c)
    return prefix, compactions, ng.argmin_schedule(n, prefix, compactions)


@functools.lru_cache(maxsize=None)
def checked_tree(kind, n):
    """(matrix, the device's tree) of a large case once check_tree has accepted it; tests/test_gpu_nj_bootstrap_edges.py feeds these
    join records to the bipartition kernel."""
    mat = _matrix(kind, n)
    prefix, compactions, rounds = _schedule(n, kind)
    ng.assert_schedule(n, prefix, compactions, rounds)                # the condition on the sampling, before the device is called
    got = _tree(get_device(), mat)
    assert got[0][:prefix] == nc.nj_prefix(mat, prefix)
    nc.check_tree(mat, got, rounds)
    return mat, got


@pytest.mark.parametrize("n,kind", LARGE)
def test_large_sizes_by_prefix_and_replay(n, kind):
    """1 100 and 1 600: sub-steps u = 2 and (at 1 600) u = 3 and a row from 1 024 on decide joins, the compaction's second column turn
    moves values that differ.  2 100: the second turn of k_nj_rows' column loop, the grid-stride rows of k_nj_init, k_nj_rows and
    k_nj_compact, the second row of a thread of k_nj_pick, all three column turns of the first compaction, nine workgroups into R[a]."""
    c = ng.kernel_constants()
    compactions = ng.compactions(n, c)
    if n == 2100:
        assert n > c["ROW_GRID_CAP"] and any(m > 2 * c["PICK_THREADS"] for _, m, _ in compactions)
        assert any(c["PICK_THREADS"] < m <= 2 * c["PICK_THREADS"] for _, m, _ in compactions)
        assert any(m > 2 * c["UNROLL"] * c["THREADS"] for _, m, _ in compactions)      # three column turns of k_nj_compact
    mat, got = checked_tree(kind, n)
    if kind == "additive":
        # La = floor(((r-2) w(a,b) + R(a) - R(b)) / (2 (r-2))) divides exactly on an additive matrix, so a length tells when R(b) is one
        # unit too large — anywhere else that shows once in 2 (r-2) joins.  The rows of the first compaction's grid-stride turn are
        # joined later, as b, to rows of its first turn: what the compaction wrote to to_R[] for them is read there.
        first = compactions[0][0]
        assert any(t >= first and a < c["ROW_GRID_CAP"] <= b for t, (a, b, _, _) in enumerate(got[0]))
        assert nc.negative_lengths(got) == 0 and all(x % nc.ONE == 0 for x in nc.all_lengths(got))
    if kind != "cherries":                                           # (the other kinds decide where their joins fall themselves)
        return
    assert sorted(m[:2] for m in got[0][:len(ng.CHERRIES[n])]) == sorted(ng.CHERRIES[n])
    reached = _reached(n, got[0])                                    # where the accepted tree's joins were met
    assert reached["step"] >= {(0, u) for u in range(min(c["UNROLL"], (n - 1) // (2 * c["THREADS"]) + 1))} and reached["row"] >= c["PICK_THREADS"]
    if n == 2100:
        assert (1, 0) in reached["step"] and reached["row"] >= c["ROW_GRID_CAP"]


def test_a_row_pitch_beyond_n_and_garbage_past_one_pick_stride():
    """1 101 samples, an odd n (the working pitch is n + 1) past one stride of k_nj_pick, at a row pitch of 1 111 with INT32_MIN /
    INT32_MAX in the padding and on the diagonal."""
    n = 1101
    c = ng.kernel_constants()
    assert n % 2 == 1 and n > c["PICK_THREADS"]
    mat = _matrix("ties3", n)
    compactions = ng.compactions(n, c)
    rounds = ng.argmin_schedule(n, 8, compactions)
    ng.assert_schedule(n, 8, compactions, rounds)
    d = get_device()
    got = _tree(d, mat, stride=n + 10, garbage=True)
    assert got[0][:8] == nc.nj_prefix(mat, 8)
    nc.check_tree(mat, got, rounds)
    assert _tree(d, mat, garbage=True) == got


def test_two_runs_give_the_same_tree():
    mat, got = checked_tree("cherries", 2100)
    assert _tree(get_device(), mat) == got
