"""The preserved-flow rule of csrc/flows.hip (its header comment) stated in NumPy, and the cases the CPU and the GPU tests of it share.

    out_filters = filters.copy();  out_base = base[:, cols]
    for each sample s, each slot of its exclude list:
        slot >= n_sites                              -> err |= 1, nothing else
        line_off[s, slot] == 0 or filters & 0x80     -> nothing
        else out_filters[s, slot] |= F_REGION;  if col_of[slot] >= 0: out_base[s, col_of[slot]] = '-'

tests/test_flows_cpu.py pins this statement to the oracle's two calls (full list without an exclude set, preserved list with one);
tests/test_gpu_flows.py holds snpgpu_region_flow_dev against it."""
import random

import numpy as np

from oracle import fuzz
from oracle import pileup_oracle as po

F_REGION = po.F_REGION           # bit 5 of a filter mask
F_MALFORMED = 0x80               # bit 7: the position's line is malformed, no record
DASH = 0x2D


def flow_rule(base, filters, line_off, cols, col_of, excl_off, excl_slots):
    """(out_base [n_samples][n_cols], out_filters [n_samples][n_sites], err) of base / filters / line_off [n_samples][n_sites],
    cols [n_cols], col_of [n_sites] (-1: not a column) and the exclude lists as a CSR pair (excl_slots may be None or empty)."""
    base, filters, line_off = np.asarray(base, dtype=np.uint8), np.asarray(filters, dtype=np.uint8), np.asarray(line_off)
    n_samples, n_sites = filters.shape
    cols = np.asarray(cols, dtype=np.int64)
    out_filters = filters.copy()
    out_base = base[:, cols].copy() if len(cols) else np.zeros((n_samples, 0), dtype=np.uint8)
    err = 0
    if excl_slots is None:
        return out_base, out_filters, err
    for s in range(n_samples):
        for k in range(int(excl_off[s]), int(excl_off[s + 1])):
            slot = int(excl_slots[k])
            if slot >= n_sites:
                err |= 1
                continue
            if line_off[s, slot] == 0 or filters[s, slot] & F_MALFORMED:
                continue
            out_filters[s, slot] |= F_REGION
            if col_of[slot] >= 0:
                out_base[s, col_of[slot]] = DASH
    return out_base, out_filters, err


def col_of_cols(cols, n_sites):
    """The inverse of a column list: col_of[slot] = j where cols[j] == slot, -1 for a slot that is no column."""
    col_of = np.full(n_sites, -1, dtype=np.int32)
    col_of[np.asarray(cols, dtype=np.int64)] = np.arange(len(cols), dtype=np.int32)
    return col_of


def csr(lists):
    """Per-sample slot lists as (excl_off int32 [n + 1], excl_slots uint32 — one zero entry when every list is empty)."""
    off = np.zeros(len(lists) + 1, dtype=np.int32)
    np.cumsum([len(e) for e in lists], out=off[1:])
    flat = np.concatenate([np.asarray(e, dtype=np.uint32) for e in lists]) if off[-1] else np.zeros(1, dtype=np.uint32)
    return off, flat.astype(np.uint32)


# ---- the samples of the oracle comparison ---------------------------------------------------------------------------------------
ORACLE_SEEDS = (101, 102, 103, 104, 105, 106, 107, 108)
ORACLE_PARAMS = [po.CallerParams(q, 0.6, dp, sd, sb) for q, dp, sd, sb in
                 ((0, 1, 0, 0.0), (13, 3, 2, 0.1), (0, 25, 0, 0.0), (13, 1, 2, 0.0), (0, 3, 0, 0.1))]
assert {p.min_base_quality for p in ORACLE_PARAMS} == {0, 13} and {p.min_cons_depth for p in ORACLE_PARAMS} == {1, 3, 25}
assert {p.min_cons_strand_depth for p in ORACLE_PARAMS} == {0, 2} and {p.min_cons_strand_bias for p in ORACLE_PARAMS} == {0.0, 0.1}


def oracle_samples(seeds=ORACLE_SEEDS):
    """[(pileup bytes, exclude set)] of fuzz.synth_pileup samples on one genome of 3000 positions, the full site list (sorted: the
    order of a site set's slots) and a shuffled preserved list.  The full list is the union of the samples' sites and five
    positions past the genome's end, which have no pileup line; every sample's exclude set is 30 % of the full list."""
    datas, full = [], set()
    for seed in seeds:
        data, _, sites = fuzz.synth_pileup(seed, genome_len=3000, n_sites=120)
        datas.append(data)
        full.update(sites)
    full.update((b"synth_chr1", 3000 + k) for k in range(1, 6))
    full = sorted(full)
    rng = random.Random(7)
    preserved = rng.sample(full, len(full) * 6 // 10)                      # (a shuffled subset: sample() returns selection order)
    preserved += [k for k in full[-5:] if k not in preserved][:3]          # some of the positions without a line are columns
    samples = [(data, set(rng.sample(full, len(full) * 3 // 10))) for data in datas]
    return samples, full, preserved


def oracle_full_call(data, full, p):
    """(base, filters, line_off) rows of one sample in full-list order from the oracle's full-list call: what the device's call of
    the whole set leaves (a position without a line: '-', no filter, offset 0)."""
    cons, detail = po.call_consensus_sites(data, full, set(), p)
    base = np.frombuffer(cons, dtype=np.uint8).copy()
    filters = np.array([detail[k][2] if k in detail else 0 for k in full], dtype=np.uint8)
    line_off = np.array([1 if k in detail else 0 for k in full], dtype=np.uint64)
    return base, filters, line_off


def flow_inputs(full, preserved, excludes):
    """(cols, col_of, excl_off, excl_slots) of a preserved list and per-sample exclude sets over the (sorted) full list."""
    slot = {k: i for i, k in enumerate(full)}
    cols = np.array([slot[k] for k in preserved], dtype=np.uint32)
    excl_off, excl_slots = csr([sorted(slot[k] for k in e) for e in excludes])
    return cols, col_of_cols(cols, len(full)), excl_off, excl_slots


def check_against_oracle_preserved(data, full, preserved, excluded, p, out_base_row, out_filters_row):
    """The derived preserved flow of one sample against the oracle's own preserved call: the bases in preserved order, the masks at
    every position that call parsed.  Returns how many masks were compared."""
    want, detail = po.call_consensus_sites(data, preserved, excluded, p)
    assert bytes(out_base_row) == want
    slot = {k: i for i, k in enumerate(full)}
    for key, (_, _, mask) in detail.items():
        assert int(out_filters_row[slot[key]]) == mask, key
    return len(detail)


# ---- the small exhaustive case ------------------------------------------------------------------------------------------------
SMALL_SAMPLES, SMALL_SITES = 3, 37


def small_case(cols_shape, excl_shape, seed=5, bad_slots=False):
    """Arrays of the 3 x 37 case.  cols_shape: "empty", "identity" or "subset" (shuffled); excl_shape: "mixed" (the lists described
    below), "none" (every list empty: the caller passes a null excl_slots) or "long" (lists of 257 and 513 entries).
    bad_slots: one slot equal to n_sites and one of 0xFFFFFFFF among the others.

    The mixed lists — sample 0: a slot that is a column, one that is not, a slot without a line, one whose line is the file's first
    (line_off exactly 1), a malformed one (bit 7), one that has Region already, one slot twice; sample 1: empty; sample 2: two
    ordinary slots.  (With cols "identity" every slot is a column, with "empty" none is.)"""
    rng = np.random.default_rng(seed)
    n, S = SMALL_SAMPLES, SMALL_SITES
    base = rng.choice(np.frombuffer(b"ACGTacgt-N", dtype=np.uint8), size=(n, S)).astype(np.uint8)
    filters = rng.integers(0, 32, size=(n, S), dtype=np.uint8)
    filters[rng.random((n, S)) < 0.5] = 0
    line_off = rng.integers(2, 1 << 40, size=(n, S)).astype(np.uint64)
    if cols_shape == "empty":
        cols = np.zeros(0, dtype=np.uint32)
    elif cols_shape == "identity":
        cols = np.arange(S, dtype=np.uint32)
    else:
        cols = rng.permutation(S)[:19].astype(np.uint32)
    col_of = col_of_cols(cols, S)
    is_col = col_of >= 0
    a_col = int(np.nonzero(is_col)[0][0]) if is_col.any() else 0
    not_col = next((i for i in range(S) if not is_col[i] and i != a_col), a_col + 1)
    free = [i for i in range(S) if i not in (a_col, not_col)]
    no_line, first_line, malformed, has_region, twice, o1, o2 = free[:7]
    line_off[0, no_line] = 0
    line_off[0, first_line] = 1
    filters[0, malformed] |= F_MALFORMED
    filters[0, has_region] |= F_REGION
    if excl_shape == "none":
        lists = [[], [], []]
    elif excl_shape == "mixed":
        lists = [[a_col, not_col, no_line, first_line, malformed, has_region, twice, twice], [], [o1, o2]]
    else:                                                                  # the 256-thread stride of a list: second and third turns
        lists = [list(rng.integers(0, S, size=257)), list(rng.integers(0, S, size=513)), [o1]]
        line_off[1, no_line] = 0
        filters[1, malformed] |= F_MALFORMED
    if bad_slots:
        lists[0] = lists[0][:2] + [S] + lists[0][2:]
        lists[2] = lists[2] + [0xFFFFFFFF]
    excl_off, excl_slots = csr(lists)
    return dict(base=base, filters=filters, line_off=line_off, cols=cols, col_of=col_of, excl_off=excl_off, excl_slots=excl_slots,
                n_samples=n, n_sites=S)
