"""The rank glue of ``hot_path_batch --mst`` (hot_path.mst_over_ranks) with bands that hold rows on every rank: 300 ids give
three tile rows, so three ranks own 128, 128 and 44 rows of a matrix padded to 384.  Every rank builds the forest of its own band
on the device (the second and third band begin past row 0), and rank 0 merges the forests with Kruskal in the same edge order:
the result must be THE tree of the whole matrix."""
import os

import numpy as np
import pytest

from tests import mst_cases as mc
from tests.mst_ranks_worker import matrix
from tests.ranks_util import ROOT, run_ranks

pytestmark = pytest.mark.gpu

N = 300


@pytest.mark.parametrize("world, kind", [(3, "xor"), (2, "tie"), (3, "tie"), (2, "xor")])
def test_forests_of_several_ranks_merge_into_the_tree(tmp_path, world, kind):
    out = str(tmp_path / "tree.npz")
    run_ranks(world, [os.path.join(ROOT, "tests", "mst_ranks_worker.py"), str(N), kind, out], tmp_path)
    got = np.load(out)
    rows = [int(hi - lo) for lo, hi in got["band_rows"]]
    assert rows == ([128, 128, 44] if world == 3 else [256, 44])
    want = mc.mst_of_matrix(matrix(N, kind))
    assert len(want) == N - 1 and mc.weight(want) == (593 if kind == "xor" else 299)
    assert got["u"].dtype == np.uint32 and got["dist"].dtype == np.int32
    assert mc.edges_of_arrays(got["u"], got["v"], got["dist"]) == want
