"""One rank of tests/test_gpu_mst_ranks.py (started by tests/ranks_util.run_ranks; not a test module): the rank glue of
hot_path_batch --mst on a seeded matrix, without a job around it.

    mst_ranks_worker.py N KIND OUT.npz

Every rank builds the same symmetric N x N int32 matrix (KIND: xor or tie), keeps of it only the 128 x 128 tiles (and mirror
images) that sharding.RowBands deals to it — what snpgpu_distance_packed_dev would have computed on this rank, zeros everywhere
else and in the padding —, exchanges the row bands, and calls hot_path.mst_over_ranks.  Rank 0 saves the tree it gets."""
import sys

import numpy as np


def matrix(n, kind):
    from tests import mst_cases as mc
    return mc.xor_matrix(n) if kind == "xor" else mc.seeded_matrix(n, 17)


def main():
    n, kind, out = int(sys.argv[1]), sys.argv[2], sys.argv[3]
    import torch
    from snp_pipeline_amd import device as devmod
    from snp_pipeline_amd import hot_path, sharding
    comm = hot_path._Comm()
    dev = devmod.Device(comm.local_rank)
    dev.use_torch_stream()
    try:
        bands = sharding.RowBands(n, comm.world)
        T = sharding.DIST_TILE
        full = np.zeros((bands.n_padded, bands.n_padded), dtype=np.int32)
        full[:n, :n] = matrix(n, kind)
        mine = np.zeros_like(full)
        for t, (bi, bj) in enumerate(sharding.upper_tiles(n)):
            if t % comm.world == comm.rank:
                mine[bi * T:(bi + 1) * T, bj * T:(bj + 1) * T] = full[bi * T:(bi + 1) * T, bj * T:(bj + 1) * T]
                mine[bj * T:(bj + 1) * T, bi * T:(bi + 1) * T] = full[bj * T:(bj + 1) * T, bi * T:(bi + 1) * T]
        dmat = torch.from_numpy(mine).cuda()
        band = bands.exchange(dmat, comm.rank) if comm.dist else None
        tree = hot_path.mst_over_ranks(torch, dev, comm, bands, dmat, band, n)
        assert (tree is None) == (comm.rank != 0)
        if tree is not None:
            np.savez(out, u=tree[0], v=tree[1], dist=tree[2], band_rows=np.asarray([bands.band_rows(r) for r in range(comm.world)]))
        comm.barrier()
    finally:
        dev.close()
        comm.close()


if __name__ == "__main__":
    main()
