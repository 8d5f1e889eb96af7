"""One rank of tests/test_gpu_clusters_ranks.py (started by tests/ranks_util.run_ranks; not a test module): the rank glue of
hot_path_batch --closePairs / --clusters on a seeded matrix, without a job around it.

    clusters_ranks_worker.py N SEED THRESHOLD OUT.npz

Every rank builds the same symmetric N x N int32 matrix, keeps of it only the 128 x 128 tiles (and mirror images) that
sharding.RowBands deals to it — what snpgpu_distance_packed_dev would have computed on this rank, zeros everywhere else and in
the padding —, exchanges the row bands, and calls hot_path.close_rows_over_ranks.  Rank 0 saves the CSR it gets."""
import sys

import numpy as np


def seeded_matrix(n, seed):
    rng = np.random.default_rng(seed)
    m = rng.integers(1, 60, size=(n, n)).astype(np.int32)
    m = np.minimum(m, m.T)
    np.fill_diagonal(m, 0)
    return m


def main():
    n, seed, threshold, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
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
        full[:n, :n] = seeded_matrix(n, seed)
        mine = np.zeros_like(full)
        for t, (bi, bj) in enumerate(sharding.upper_tiles(n)):
            if t % comm.world == comm.rank:
                mine[bi * T:(bi + 1) * T, bj * T:(bj + 1) * T] = full[bi * T:(bi + 1) * T, bj * T:(bj + 1) * T]
                mine[bj * T:(bj + 1) * T, bi * T:(bi + 1) * T] = full[bj * T:(bj + 1) * T, bi * T:(bi + 1) * T]
        dmat = torch.from_numpy(mine).cuda()
        band = bands.exchange(dmat, comm.rank) if comm.dist else None
        csr = hot_path.close_rows_over_ranks(torch, dev, comm, bands, dmat, band, n, threshold)
        assert (csr is None) == (comm.rank != 0)
        if csr is not None:
            np.savez(out, row_off=csr[0], col=csr[1], dist=csr[2], band_rows=np.asarray([bands.band_rows(r) for r in range(comm.world)]))
        comm.barrier()
    finally:
        dev.close()
        comm.close()


if __name__ == "__main__":
    main()
