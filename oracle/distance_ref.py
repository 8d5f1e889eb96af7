"""All-pairs SNP distance as matrix products — a second, independent statement of the distance arithmetic.
TEST INFRASTRUCTURE ONLY — see ``oracle/pileup_oracle.py`` for the rules.

``snppipeline/utils.py:1135-1165`` counts, for a pair of sequences, the sites where both bytes are in ACGT after
upper-casing and differ.  With V = "is ACGT after upper-casing a-z" (n x s, 0/1) and O_c = one-hot of base c:

    D = V . V^T  -  sum_c  O_c . O_c^T          (both valid)  -  (both valid and equal)

Every entry of every product is an integer count of sites, so in float32 the sums are exact in any order as long as they
stay below 2^24 (asserted).  ``steps_oracle.sequence_distance`` and the row loop of the GPU tests walk the sites of a pair;
this form never does, which is what makes it fast enough for whole matrices of 10^4 rows (numpy, 23 100 x 96: 19 s on 16
threads) and independent enough to be worth comparing with them (tests/test_distance_ref.py).
"""
import numpy as np

BASES = b"ACGT"
MAX_SITES = 1 << 24


def row_loop(sym):
    """The plain statement: one row against all others, site by site.  (n, s) uint8 -> (n, n) int32."""
    sym = np.asarray(sym, dtype=np.uint8)
    up = np.where((sym >= 97) & (sym <= 122), sym - 32, sym)
    valid = np.isin(up, np.frombuffer(BASES, dtype=np.uint8))
    n = len(sym)
    out = np.zeros((n, n), dtype=np.int32)
    for i in range(n):
        out[i] = ((up != up[i]) & valid & valid[i]).sum(axis=1)
    return out


def distance_numpy(sym, k_chunk=1 << 16):
    """(n, s) uint8 -> (n, n) int32 with float32 matrix products, K chunks accumulated in int32."""
    sym = np.asarray(sym, dtype=np.uint8)
    n, s = sym.shape
    assert s < MAX_SITES
    out = np.zeros((n, n), dtype=np.int32)
    for k0 in range(0, s, k_chunk):
        c = sym[:, k0:k0 + k_chunk]
        up = np.where((c >= 97) & (c <= 122), c - 32, c)
        hot = [(up == b).astype(np.float32) for b in BASES]
        v = hot[0] + hot[1] + hot[2] + hot[3]
        acc = v @ v.T
        for o in hot:
            acc -= o @ o.T
        out += acc.astype(np.int32)
    return out


def distance_torch(sym, device=None, row_block=2048, k_chunk=1 << 14):
    """The same formula with torch on ``device`` (default: where ``sym`` lives).  ``sym``: (n, s) uint8 tensor or array.
    The one-hot matrices exist for one K chunk at a time, the float32 products for one block of rows at a time; chunks
    are accumulated in int32, so a chunk below 2^11 sites keeps every float32 sum below 2^11 if a matmul back end should
    ever not be exact up to 2^24.  Returns an (n, n) int32 tensor on the device."""
    import torch
    if not isinstance(sym, torch.Tensor):
        sym = torch.from_numpy(np.ascontiguousarray(sym, dtype=np.uint8))
    if device is not None:
        sym = sym.to(device)
    n, s = sym.shape
    assert s < MAX_SITES and sym.dtype == torch.uint8
    out = torch.zeros((n, n), dtype=torch.int32, device=sym.device)
    for k0 in range(0, s, k_chunk):
        c = sym[:, k0:k0 + k_chunk]
        up = torch.where((c >= 97) & (c <= 122), c - 32, c)
        hot = [(up == b).to(torch.float32) for b in BASES]
        v = hot[0] + hot[1] + hot[2] + hot[3]
        for r0 in range(0, n, row_block):
            r1 = min(n, r0 + row_block)
            acc = v[r0:r1] @ v.T
            for o in hot:
                acc -= o[r0:r1] @ o.T
            out[r0:r1] += acc.to(torch.int32)
        del hot, v, up
    return out
