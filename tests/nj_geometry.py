"""Where the kernels of csrc/nj.hip meet a join: the loop geometry read from the source, the positions of the joined pairs between
the compactions, the planted pairs of the far_cherries matrices, and the rounds in which the GPU tests of the large sizes check the
choice itself.  The statement and its checker are tests/nj_cases.py; this module is about the device code alone."""
import bisect
import os
import re

from tests import nj_cases as nc


def kernel_constants():
    """The loop geometry of csrc/nj.hip, read from its source: THREADS, PICK_THREADS, ROW_GRID_CAP, UNROLL, COMPACT_NUM, COMPACT_DEN."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "snp_pipeline_amd", "csrc", "nj.hip")) as f:
        src = f.read()
    return {name: int(re.search(r"#define NJ_%s (\d+)" % name, src).group(1)) for name in ("THREADS", "PICK_THREADS", "ROW_GRID_CAP", "UNROLL", "COMPACT_NUM", "COMPACT_DEN")}


def compactions(n, c=None):
    """nj_cases.compaction_rounds with the schedule of the source."""
    c = c or kernel_constants()
    return nc.compaction_rounds(n, c["COMPACT_NUM"], c["COMPACT_DEN"])


def row_step(i, k, c):
    """(turn of k_nj_rows' column loop, sub-step u within it) in which row i meets column k > i: a turn is UNROLL sub-steps of
    2 THREADS columns, from the even column at or below i + 1 on."""
    d = k - ((i + 1) & ~1)
    span = 2 * c["THREADS"]
    return d // (span * c["UNROLL"]), (d // span) % c["UNROLL"]


def join_positions(n, merges, compactions):
    """[(m, position of a, position of b)] per round: where the device's kernels meet the joined pair.  A position is the rank of a
    slot among the slots stored since the last compaction; m is the stored extent."""
    stored, retired, at = list(range(n)), set(), {t for t, _, _ in compactions}
    out = []
    for t, m in enumerate(merges):
        if t in at:
            stored = [s for s in stored if s not in retired]
            retired = set()
        out.append((len(stored), bisect.bisect_left(stored, m[0]), bisect.bisect_left(stored, m[1])))
        retired.add(m[1])
    return out


def argmin_schedule(n, prefix, compactions):
    """The rounds in which the GPU tests of the large sizes check the choice itself: the first `prefix` rounds, the round before and
    the two rounds after every compaction, every 32nd round, the last 64."""
    rounds = max(n - 3, 0)
    want = set(range(min(prefix, rounds))) | set(range(0, rounds, 32)) | set(range(max(rounds - 64, 0), rounds))
    for t, _, _ in compactions:
        want |= {t - 1, t, t + 1}
    return {t for t in want if 0 <= t < rounds}


def assert_schedule(n, prefix, compactions, rounds):
    """The condition on the sampling, asserted before the device is called: at least 64 argmin rounds, among them the prefix, the
    round before and the two after every compaction, every 32nd round and the last 64.  No case may drop rounds."""
    assert len(rounds) >= 64
    assert set(range(prefix)) <= rounds and set(range(0, n - 3, 32)) <= rounds and set(range(n - 3 - 64, n - 3)) <= rounds
    assert all({t - 1, t, t + 1} <= rounds for t, _, _ in compactions if t + 1 < n - 3)


# the planted pairs of the far_cherries matrices the GPU tests use, by n; tests/test_nj_cpu.py asserts where they fall
CHERRIES = {
    1100: [(0, 1099), (1, 600), (3, 1030), (2, 400), (1026, 1027), (1096, 1098), (700, 1090)],
    1600: [(0, 1599), (1, 1100), (3, 600), (5, 100), (1026, 1500), (1596, 1598), (40, 1590)],
    2100: [(0, 2099), (1, 2049), (3, 515), (5, 1029), (7, 1543), (1026, 1027), (2050, 2051), (2096, 2098), (300, 2000)],
}
CHERRY_SEED = 7
