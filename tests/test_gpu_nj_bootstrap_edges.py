"""The kernels of csrc/nj_bootstrap.hip past one turn of every loop: k_nj_splits on real trees of 2 100 samples, with 256 threads
(more than 64 words) and with a thread's second word (more than 256 words); k_split_count and the sort's SplitLess over 66 words, and
k_split_count past its grid; k_boot_resample with a second turn over the row groups.  Every expected value comes from the statement of
tests/nj_bootstrap_cases.py at test time."""
import collections
import time

import numpy as np
import pytest

from tests import nj_bootstrap_cases as bc
from tests import nj_cases as nc
from tests.gpu_util import get_device
from tests.test_gpu_nj_bootstrap import _dev, _filled, _host, _pack, _sharing_the_cherries, _splits_on_device, _support_on_device, _symbols, _tree
from tests.test_gpu_nj_edges import checked_tree

pytestmark = pytest.mark.gpu


def _cu_count():
    import torch
    return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)


def _rows_of(n, sets):
    """bc.split_words by way of int.to_bytes: the same array, fast enough for 16 500 rows of 258 words."""
    w = bc.words(n)
    out = np.frombuffer(b"".join(x.to_bytes(8 * w, "little") for x in sets), dtype="<u8").reshape(len(sets), w)
    assert np.array_equal(out[:40], bc.split_words(n, sets[:40])) and np.array_equal(out[-3:], bc.split_words(n, sets[-3:]))
    return out


# ---- the bipartitions ------------------------------------------------------------------------------------------------------------
def test_the_bipartitions_of_real_trees_of_2100_samples():
    """The join records the device built for the two matrices of tests/test_gpu_nj_edges.py (accepted by check_tree there): joins all
    over the 33 words, rows that are complements and rows that are not — where the all-2 tree is one chain into slot 0."""
    d = get_device()
    n = 2100
    trees = [checked_tree("cherries", n)[1][0], checked_tree("ties10", n)[1][0], nc.star_of_equal(n)[0]]
    want = [_rows_of(n, bc.splits(n, merges)) for merges in trees]
    for merges in trees[:2]:
        into_0 = sum(1 for m in merges if m[0] == 0)
        assert 0 < into_0 < len(merges) // 2                         # both kinds of rows
    for chosen in ([0], [1], [0, 1, 2]):
        got = _splits_on_device(d, n, [trees[t] for t in chosen])
        for at, t in enumerate(chosen):
            assert np.array_equal(got[at], want[t]), (chosen, t)
        assert not (got[:, :, -1] >> np.uint64(n % 64)).any() and not (got[:, :, 0] & np.uint64(1)).any()


def _random_joins(n, seed, spare_0):
    """A valid join sequence without any matrix: two live slots at random, the smaller keeps its slot.  With spare_0 slot 0 is never
    drawn (it stays for the star), so no leaf set holds sample 0 and no row is a complement."""
    rng = np.random.default_rng(seed)
    live = list(range(1 if spare_0 else 0, n))
    merges = []
    draws = rng.random((n - 3, 2))
    for t in range(n - 3):
        i = int(draws[t, 0] * len(live))
        j = int(draws[t, 1] * (len(live) - 1))
        j += j >= i
        a, b = min(live[i], live[j]), max(live[i], live[j])
        merges.append((a, b))
        at = i if live[i] == b else j
        live[at] = live[-1]
        live.pop()
    return merges


@pytest.mark.parametrize("n", [4200, 16500])
def test_the_bipartitions_with_256_threads_and_with_a_second_word_per_thread(n):
    """4 200 samples are 66 words: k_nj_splits launches 256 threads instead of 64.  16 500 are 258 words: threads 0 and 1 own a second
    word (256 and 257), the last of them with the tail.  The statement's bitsets are Python integers: 0.3 s at 16 500, and int.to_bytes lays them out (_rows_of)."""
    d = get_device()
    w = bc.words(n)
    assert w > 64 and n % 64 and (n < 16000 or w > 256)
    anywhere, beside_0 = _random_joins(n, 5, False), _random_joins(n, 6, True)
    assert any(m[0] == 0 for m in anywhere) and not any(m[0] == 0 for m in beside_0)
    began = time.time()
    want = [_rows_of(n, bc.splits(n, merges)) for merges in (anywhere, beside_0)]
    print("the statement's bipartitions at n = %d: %.2f s" % (n, time.time() - began))
    got = _splits_on_device(d, n, [anywhere, beside_0])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert not (got[:, :, -1] >> np.uint64(n % 64)).any()           # the tail of the last word is zero
    assert not (got[:, :, 0] & np.uint64(1)).any()                  # no row holds sample 0
    assert (want[0][:, 64:] != 0).any(axis=0).all() and (want[1][:, 64:] != 0).any(axis=0).all()      # every later word is set in some row


# ---- the support counts ----------------------------------------------------------------------------------------------------------
def test_the_counts_over_66_words_told_apart_in_the_last_two():
    """Main rows equal in words 0 ... 63 and different in word 64 or 65 alone: a probe of k_split_count needs its second turn over 64
    words, and SplitLess of the sort runs over all 66.  Replicate rows hit them, or miss by one bit in word 64, 65, 63 or 0, set or
    cleared: on either side of their neighbour in the sorted order."""
    d = get_device()
    n = 4200
    assert bc.words(n) == 66
    rng = np.random.default_rng(3)
    base = 0
    for bit in np.flatnonzero(rng.random(64 * 64) < 0.5):
        base |= 1 << int(bit)
    base &= ~1
    base |= (1 << 2) | (1 << (63 * 64 + 5))
    base &= ~((1 << 3) | (1 << (63 * 64 + 6)))
    main = [base | (1 << (64 * 64 + i)) for i in range(0, 64, 2)] + [base | (1 << (65 * 64 + i)) for i in range(1, 40, 3)]
    assert len(set(main)) == len(main) and all(x < (1 << n) for x in main)
    hits = [main[i] for i in (0, 0, 5, 31, 32, 32, 32, 44, len(main) - 1)]
    misses = []
    for x in main[::3]:
        misses += [x | (1 << (64 * 64 + 1)), x | (1 << (65 * 64 + 0)), x ^ (1 << (63 * 64 + 6)), x ^ (1 << (63 * 64 + 5)), x ^ (1 << 3), x ^ (1 << 2)]
    misses += [base, base | (1 << (64 * 64)) | (1 << (65 * 64 + 1))]
    assert not set(misses) & set(main)
    by_words = lambda x: tuple((x >> (64 * k)) & bc.MASK for k in range(66))      # noqa: E731  (the device's order: from word 0)
    order = sorted(main, key=by_words)
    keys = [by_words(x) for x in misses]
    assert any(k < by_words(order[0]) for k in keys) and any(k > by_words(order[-1]) for k in keys) and any(by_words(order[3]) < k < by_words(order[-3]) for k in keys)
    for rows in (hits, misses, hits + misses + main, main[::-1]):
        have = collections.Counter(rows)
        assert _support_on_device(d, n, main, rows) == [have[x] for x in main], len(rows)


def test_more_replicate_rows_than_the_grid_of_the_count_has_waves():
    """k_split_count runs a wave per row on at most 32 workgroups per CU, four waves each: rows past 128 per CU go round its loop."""
    d = get_device()
    n = 257
    assert bc.words(n) == 5
    main = bc.splits(n, _tree("random", n))
    other = bc.splits(n, _tree("ties3", n))
    once = main + other + _sharing_the_cherries(n, main)
    waves = 32 * _cu_count() * 4
    rows = once * (waves // len(once) + 1) + main[:100]
    assert len(rows) > waves and len(rows) - waves >= 100
    have = collections.Counter(rows)
    assert len({have[x] for x in main}) >= 3                         # absent from the other rows, once or twice in them, and among the last hundred
    assert _support_on_device(d, n, main, rows) == [have[x] for x in main]


# ---- the resampled pack ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [129, 130, 131])
def test_the_resampled_pack_with_a_second_turn_over_the_row_groups(n):
    """70 001 output columns are 274 workgroups across, so the grid is ceil(8 CUs / 274) row groups deep and 33 groups of four rows go
    round k_boot_resample's loop; the last group holds one, two or three rows."""
    import torch
    d = get_device()
    s, n_cols = 1000, 70001
    dst_words = d.packed_row_bytes(n_cols) // 16
    gx = (dst_words // 2 + 3) // 4                                   # as resample_run computes it: four waves a workgroup
    steps, fill = (n + 3) // 4, (8 * _cu_count() + gx - 1) // gx
    assert steps > fill and n % 4 in (1, 2, 3)
    sym = _symbols(n, s, 7000 + n)
    cols = np.sort(bc.columns(9, 2, n_cols) % s).astype(np.uint32)
    want = _pack(sym[:, cols])
    assert want.shape[1] == dst_words and want[fill * 4:].any()
    src, d_cols = _dev(_pack(sym)), _dev(cols)
    out = _filled(want.size + 16, -1, torch.int32)
    d.resample_packed_dev(src.data_ptr(), n, s, d_cols.data_ptr(), n_cols, out.data_ptr())
    torch.cuda.synchronize()
    got = _host(out, np.uint32)
    assert np.array_equal(got[:want.size].reshape(want.shape), want)
    assert (got[want.size:] == 0xFFFFFFFF).all()
