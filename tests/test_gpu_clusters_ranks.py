"""The rank glue of ``hot_path_batch --closePairs / --clusters`` (hot_path.close_rows_over_ranks) with bands that hold rows on
every rank: 300 ids give three tile rows, so three ranks own 128, 128 and 44 rows of a matrix padded to 384 — the second and
third band begin past row 0 (the kernel is given where row 0 would lie in front of the band), and three CSR pieces that are not
empty are joined into one."""
import os

import numpy as np
import pytest

from tests import clusters_cases as cc
from tests.clusters_ranks_worker import seeded_matrix
from tests.ranks_util import ROOT, run_ranks

pytestmark = pytest.mark.gpu

N, SEED = 300, 17


# (two ranks at a threshold that lets everything through: 256 x 300 entries do not fit the first call's room, so the second call runs)
@pytest.mark.parametrize("world, threshold", [(3, 6), (2, 59)])
def test_bands_of_several_ranks_thresholded_and_joined(tmp_path, world, threshold):
    out = str(tmp_path / "csr.npz")
    run_ranks(world, [os.path.join(ROOT, "tests", "clusters_ranks_worker.py"), str(N), str(SEED), str(threshold), out], tmp_path)
    got = np.load(out)
    rows = [int(hi - lo) for lo, hi in got["band_rows"]]
    assert rows == ([128, 128, 44] if world == 3 else [256, 44]) and [int(lo) for lo, _ in got["band_rows"]][1] > 0
    mat = seeded_matrix(N, SEED)
    want = cc.filter_rows(mat, threshold)
    assert threshold != 59 or len(want[1]) == N * N
    assert all(int(want[0][hi] - want[0][lo]) > 2 * (hi - lo) for lo, hi in got["band_rows"])            # every band's piece holds more than its diagonal
    assert np.array_equal(got["row_off"], want[0])
    assert np.array_equal(got["col"], want[1]) and got["col"].dtype == np.uint32
    assert np.array_equal(got["dist"], want[2])
