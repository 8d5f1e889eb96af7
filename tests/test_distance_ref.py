"""oracle/distance_ref.py (the matrix-product statement of the SNP distance, which checks whole matrices in the GPU tests) is
itself checked: both of its forms against the site-by-site row loop and against steps_oracle.sequence_distance."""
import numpy as np
import pytest

from oracle import distance_ref as dr
from oracle import steps_oracle as so


def _all_bytes(n, s, seed):
    rng = np.random.default_rng(seed)
    sym = rng.integers(0, 256, size=(n, s), dtype=np.uint8)
    letters = np.frombuffer(b"ACGTacgt", dtype=np.uint8)
    pick = rng.random((n, s)) < 0.6                         # enough valid sites for the distances not to be all tiny
    return np.where(pick, rng.choice(letters, size=(n, s)), sym).astype(np.uint8)


@pytest.mark.parametrize("s", [0, 1, 31, 32, 33, 127, 128, 129])
def test_both_forms_equal_the_row_loop_and_the_pairwise_oracle(s):
    import torch
    n = 19
    sym = _all_bytes(n, s, seed=s)
    if s >= 32:
        sym[:, :256 if s >= 256 else s] = np.resize(np.arange(256, dtype=np.uint8), (n, min(s, 256)))   # every value s allows ...
        sym[1::2, :] = np.roll(sym[1::2, :], 1, axis=1)                                                    # ... against a different one
    want = dr.row_loop(sym)
    # latin-1 maps byte b to code point b; only a-z have an upper case inside ACGT, as in the kernel's to_upper (str.upper()
    # turns 0xB5 / 0xFF into code points above 255, not in ACGT either).  0xDF is the one latin-1 character whose upper case
    # is two characters long, which would shift the rest of the string: the pairwise oracle sees 0xDE in its place.
    seqs = [row.tobytes().decode("latin-1").replace("\xdf", "\xde") for row in sym]
    for i in range(n):
        for j in range(n):
            assert want[i, j] == so.sequence_distance(seqs[i], seqs[j]), (i, j)
    assert np.array_equal(dr.distance_numpy(sym), want)
    assert np.array_equal(dr.distance_numpy(sym, k_chunk=7), want)
    assert np.array_equal(dr.distance_torch(sym, device="cpu").numpy(), want)
    assert np.array_equal(dr.distance_torch(torch.from_numpy(sym), row_block=5, k_chunk=13).numpy(), want)


def test_forms_on_300_rows_of_all_256_values():
    sym = _all_bytes(300, 777, seed=3)
    sym[:, :256] = np.arange(256, dtype=np.uint8)
    sym[150:, :256] = np.arange(256, dtype=np.uint8)[::-1]
    want = dr.row_loop(sym)
    assert want.max() > 100 and np.array_equal(want, want.T) and not want.diagonal().any()
    assert np.array_equal(dr.distance_numpy(sym), want)
    assert np.array_equal(dr.distance_numpy(sym, k_chunk=100), want)
    assert np.array_equal(dr.distance_torch(sym, device="cpu", row_block=128, k_chunk=256).numpy(), want)
