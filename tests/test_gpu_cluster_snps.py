"""The kernels of csrc/cluster_snps.hip — the allele counts of every column of a packed matrix and the cluster-defining SNPs of a
labelling of its rows — and the library's host forms, against the plain statements of tests/cluster_snps_cases.py.  Everything is
compared exactly, and what lies behind an output must keep the mark it was filled with."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import cluster_snps_cases as sc
from tests.gpu_util import get_device

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARK = 0xA5
TILE = 64 * 32                                                      # sites of a word tile: CS_TILE_WORDS words
CHUNK = 256                                                         # rows a wave walks: CS_ROW_CHUNK
SITES = (0, 1, 31, 32, 33, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
ROWS = (1, 2, CHUNK - 1, CHUNK, CHUNK + 1)


def test_the_constants_restated_here_are_the_kernels():
    src = open(os.path.join(ROOT, "snp_pipeline_amd", "csrc", "cluster_snps.hip")).read()
    assert int(re.search(r"#define CS_TILE_WORDS (\d+)", src).group(1)) * 32 == TILE
    assert int(re.search(r"#define CS_ROW_CHUNK (\d+)", src).group(1)) == CHUNK
    assert 2 ** (int(re.search(r"#define CS_PLANES (\d+)", src).group(1)) - 1) == CHUNK      # 256 equal bases carry through eight planes into the ninth
    assert int(re.search(r"#define CS_CLUSTER_CHUNK (\d+)", src).group(1)) == 64


def _pack(d, sym):
    import torch
    sym_t = torch.from_numpy(np.array(sym, dtype=np.uint8, order="C")).cuda()
    n, s = sym.shape
    pk = torch.full((max(n, 1), max(d.packed_row_bytes(s), 16)), MARK, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    if n and s:
        d.pack_matrix_dev(sym_t.data_ptr(), n, s, s, pk.data_ptr())
    d.sync()
    return pk


def _counts_dev(d, pk, n, s):
    import torch
    out = torch.full((s * 16 + 64,), MARK, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    d.site_counts_dev(pk.data_ptr(), n, s, out.data_ptr())
    d.sync()
    host = out.cpu().numpy()
    assert (host[s * 16:] == MARK).all()
    return host[:s * 16].copy().view("<i4").reshape(s, 4)


class _Out(object):
    """The four outputs with `room` entries and 8 more, everything filled with the mark."""
    def __init__(self, n_clusters, room):
        import torch
        self.room, self.n_clusters = room, n_clusters
        self.off = torch.full(((n_clusters + 1) * 8 + 64,), MARK, dtype=torch.uint8, device="cuda")
        self.site = torch.full(((room + 8) * 4,), MARK, dtype=torch.uint8, device="cuda")
        self.base = torch.full((room + 8,), MARK, dtype=torch.uint8, device="cuda")
        self.members = torch.full(((room + 8) * 4,), MARK, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def args(self):
        return self.off.data_ptr(), self.site.data_ptr(), self.base.data_ptr(), self.members.data_ptr()

    def host(self):
        return self.off.cpu().numpy(), self.site.cpu().numpy(), self.base.cpu().numpy(), self.members.cpu().numpy()

    def untouched(self):
        return all((x == MARK).all() for x in self.host())

    def written(self, total):
        """(cluster_off, site, base, members) of the first `total` entries; everything behind them keeps the mark."""
        off, site, base, members = self.host()
        c = self.n_clusters + 1
        assert (off[c * 8:] == MARK).all() and (site[total * 4:] == MARK).all() and (base[total:] == MARK).all() and (members[total * 4:] == MARK).all()
        return off[:c * 8].copy().view("<u8"), site[:total * 4].copy().view("<u4"), base[:total].copy(), members[:total * 4].copy().view("<u4")


def _snps_dev(d, pk, n, s, labels, n_clusters, protocol=False):
    """Count, then emit into exactly enough room; protocol: the count-only and the one-too-small call must write nothing."""
    import torch
    lab = torch.from_numpy(np.asarray(labels, dtype=np.int64).astype(np.int32)).cuda() if n else torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    probe = _Out(n_clusters, 4)
    total = d.cluster_snps_dev(pk.data_ptr(), n, s, lab.data_ptr(), n_clusters, 0, *probe.args())
    d.sync()
    assert probe.untouched()
    if protocol and total > 1:
        small = _Out(n_clusters, total - 1)
        assert d.cluster_snps_dev(pk.data_ptr(), n, s, lab.data_ptr(), n_clusters, total - 1, *small.args()) == total
        d.sync()
        assert small.untouched()
    out = _Out(n_clusters, total)
    assert d.cluster_snps_dev(pk.data_ptr(), n, s, lab.data_ptr(), n_clusters, max(total, 1), *out.args()) == total
    d.sync()
    return out.written(total)


def _same(got, want, where):
    for g, w, name in zip(got, want, ("cluster_off", "site", "base", "members")):
        assert g.shape == w.shape and np.array_equal(g, w), (where, name)


def _check(sym, labellings, where, protocol=False, host_form=True):
    d = get_device()
    n, s = sym.shape
    pk = _pack(d, sym)
    counts = sc.site_counts(sym)
    assert np.array_equal(_counts_dev(d, pk, n, s), counts), where
    assert np.array_equal(d.site_counts(sym), counts), where
    wants = []
    for name, (labels, n_clusters) in labellings.items():
        want = sc.cluster_snps(sym, labels, n_clusters)
        assert np.array_equal(want[3], counts[want[1], want[2]])
        _same(_snps_dev(d, pk, n, s, labels, n_clusters, protocol), want, (where, name))
        wants.append(want)
    if host_form and labellings:                                    # all labellings on one upload and pack: each as in a call of its own
        offs, site, base, members = d.cluster_snps(sym, np.stack([lab for lab, _ in labellings.values()]), n_clusters=[c for _, c in labellings.values()])
        first = 0
        for (name, _), off, want in zip(labellings.items(), offs, wants):
            k = len(want[1])
            _same((off - np.uint64(first), site[first:first + k], base[first:first + k], members[first:first + k]), want, (where, name, "host form"))
            first += k
        assert first == len(site) == len(base) == len(members)
    return wants


def _with_counts(labs):
    return {k: (v, int(v.max()) if len(v) else 0) for k, v in labs.items()}


@pytest.mark.parametrize("s", SITES)
def test_every_word_and_tile_edge_of_the_sites(s):
    n = 37
    labs = sc.labellings(n, s + 1)
    sym = sc.planted_symbols(n, s, labs["planted"], 100 + s)
    wants = _check(sym, _with_counts(labs), s)
    assert s <= 1 or sum(len(w[1]) for w in wants) > 0       # (one column of 37 planted rows defines no cluster)


@pytest.mark.parametrize("n", ROWS)
def test_every_chunk_edge_of_the_rows_with_a_cluster_across_it(n):
    s = 100
    sizes = [n] if n <= 2 else [CHUNK - 6, n - (CHUNK - 6)]          # the second cluster's rows lie on both sides of row CHUNK when n > CHUNK
    labels = np.repeat(np.arange(1, len(sizes) + 1), sizes)
    rng = np.random.default_rng(n)
    shuffled = labels[rng.permutation(n)]                            # the same sizes, no cluster contiguous in the matrix
    sym = sc.planted_symbols(n, s, labels, 7 + n, missing=0.05)
    labs = _with_counts({"sorted": labels.astype(np.uint32), "shuffled": shuffled.astype(np.uint32)})
    labs["one more number"] = (labels.astype(np.uint32), len(sizes) + 1)      # a cluster number without rows
    wants = _check(sym, labs, n)
    assert len(wants[0][1]) > 0 and wants[2][0][-1] == wants[2][0][-2]


@pytest.mark.parametrize("sizes", [(1, 2, 3, 4, 255), (256, 257), (257, 256, 1)])
def test_cluster_sizes_through_the_carry_of_eight_planes(sizes):
    n, s = sum(sizes), 70
    labels = np.repeat(np.arange(1, len(sizes) + 1), sizes).astype(np.uint32)
    sym = sc.planted_symbols(n, s, labels, 31 + n, missing=0.02)
    sym[:, 3] = np.frombuffer(b"Gg", dtype=np.uint8)[np.arange(n) % 2]       # every row one base: the counters run to n
    sym[labels == len(sizes), 5] = 0x54                                       # T in the last cluster alone, everywhere in it
    sym[labels != len(sizes), 5] = 0x41
    rng = np.random.default_rng(n)
    order = rng.permutation(n)
    wants = _check(sym, _with_counts({"sorted": labels}), sizes)
    _check(sym[order], _with_counts({"shuffled": labels[order]}), sizes, host_form=False)
    off, site, base, members = wants[0]
    last = slice(int(off[-2]), int(off[-1]))
    at = int(np.flatnonzero(site[last] == 5)[0])
    assert base[last][at] == 3 and members[last][at] == sizes[-1] and 3 not in site.tolist()
    assert sc.site_counts(sym)[3].tolist() == [0, 0, n, 0]


@pytest.mark.parametrize("s", [130, 2 * TILE + 1])
def test_one_cluster_singletons_and_interleaved_labels_over_more_than_a_chunk(s):
    n = 300
    labs = sc.labellings(n, 5)
    sym = sc.planted_symbols(n, s, labs["planted"], 77, missing=0.1)
    sym[:, 1] = 0x63                                                 # monomorphic, lower case: the all-samples cluster's, nobody else's
    wants = _check(sym, _with_counts(labs), s, host_form=(s == 130))
    by_name = dict(zip(labs, wants))
    assert 1 in by_name["one"][1].tolist() and all(1 not in by_name[k][1].tolist() for k in ("singletons", "interleaved", "planted"))
    assert (by_name["singletons"][3] == 1).all() and len(by_name["singletons"][1]) > 0


def test_every_byte_value():
    sym = sc.random_symbols(70, 300, 9, every_byte=True)
    sym[:, ::3] = sc.random_symbols(70, 100, 10)                      # enough bases among them for entries to exist
    wants = _check(sym, _with_counts(sc.labellings(70, 11)), "every byte")
    assert sum(len(w[1]) for w in wants) > 0


def test_constructed_columns():
    rows = [b"aCAAG-TTA",     # 1
            b"ACACGNTAA",     # 1
            b"AGA-G-TAC",     # 2
            b"AGATG-TAC",     # 2
            b"tGA-GNC-C",     # 2
            b"ATGAC-TAc"]     # 3
    sym = np.asarray([np.frombuffer(r, dtype=np.uint8) for r in rows], dtype=np.uint8)
    labels = np.asarray([1, 1, 2, 2, 2, 3], dtype=np.uint32)
    want = _check(sym, {"hand": (labels, 3)}, "constructed", protocol=True)[0]
    rows_of = {c + 1: [(int(want[1][e]), "ACGT"[want[2][e]], int(want[3][e])) for e in range(int(want[0][c]), int(want[0][c + 1]))] for c in range(3)}
    # column 1: a lower- and an upper-case member of one allele (cluster 1: C); cluster 2 holds G, cluster 3 T
    # column 2: cluster 3's G is private; column 3: cluster 1 holds two alleles; cluster 2 has T in one member, the others miss
    # column 4: cluster 3's C; column 5: all members missing everywhere; column 6: cluster 2 holds T and C
    # column 7: cluster 1 holds T and A; the A of clusters 2 and 3 is also held by an outsider (row 1 of cluster 1)
    # column 8: C of cluster 2 is held by the last row too, in lower case; the A of cluster 1 is its own
    assert rows_of == {1: [(1, "C", 2), (8, "A", 2)], 2: [(1, "G", 3), (3, "T", 1)], 3: [(1, "T", 1), (2, "G", 1), (4, "C", 1)]}
    # the cluster's base also held by one outsider: in the first, a middle and the last row
    n = 41
    labels = np.ones(n, dtype=np.uint32)
    labels[10:30] = 2
    base = np.full((n, 40), 0x2D, dtype=np.uint8)
    base[10:30, :] = 0x47                                            # G throughout cluster 2, nobody else holds a base
    for outsider in (None, 0, 5, n - 1):
        sym = base.copy()
        if outsider is not None:
            sym[outsider, 7] = 0x67                                  # g
        want = _check(sym, {"outsider": (labels, 2)}, outsider, host_form=False)[0]
        assert want[0].tolist() == [0, 0, 40 if outsider is None else 39] and (7 in want[1].tolist()) == (outsider is None)
        assert (want[3] == 20).all()
    sym = base.copy()
    sym[12:17, 7] = 0x4E                                             # some members missing: Members < Size
    sym[10:30, 8] = 0x2E                                             # all members missing
    want = _check(sym, {"missing": (labels, 2)}, "missing", host_form=False)[0]
    assert dict(zip(want[1].tolist(), want[3].tolist()))[7] == 15 and 8 not in want[1].tolist() and len(want[1]) == 39


def test_the_capacity_protocol_and_the_labels_that_are_refused():
    import torch
    from snp_pipeline_amd.device import SnpGpuError
    d = get_device()
    n, s = 60, 200
    labs = sc.labellings(n, 3)
    sym = sc.planted_symbols(n, s, labs["planted"], 4)
    _check(sym, _with_counts(labs), "protocol", protocol=True)
    pk = _pack(d, sym)
    c = int(labs["planted"].max())
    for at, bad in ((0, 0), (n - 1, c + 1), (17, 2 ** 32 - 1)):
        labels = labs["planted"].astype(np.int64)
        labels[at] = bad
        lab = torch.from_numpy(labels.astype(np.uint32).view(np.int32)).cuda()
        out = _Out(c, 4 * s)
        with pytest.raises(SnpGpuError):
            d.cluster_snps_dev(pk.data_ptr(), n, s, lab.data_ptr(), c, 4 * s, *out.args())
        d.sync()
        assert out.untouched(), at
        host = [np.full(c + 1, MARK, dtype=np.uint64), np.full(4 * s, MARK, dtype=np.uint32), np.full(4 * s, MARK, dtype=np.uint8), np.full(4 * s, MARK, dtype=np.uint32)]
        lab32, ncl, total = labels.astype(np.uint32), np.asarray([c], dtype=np.uint32), ctypes.c_uint64(7)
        rc = d.lib.snpgpu_cluster_snps(d.ctx, sym.ctypes.data, n, s, lab32.ctypes.data, ncl.ctypes.data, 1, 4 * s, *[h.ctypes.data for h in host], ctypes.byref(total))
        assert rc != 0 and all((h == MARK).all() for h in host) and total.value == 0, at
        with pytest.raises(ValueError):
            d.cluster_snps(sym, labels.astype(np.uint32), n_clusters=c)
    # nothing to do: no row, no site, no cluster
    lab = torch.ones(n, dtype=torch.int32, device="cuda")
    for rows, sites, clusters in ((0, s, 3), (n, 0, 1), (0, 0, 0), (0, s, 0)):
        out = _Out(clusters, 4)
        assert d.cluster_snps_dev(pk.data_ptr(), rows, sites, lab.data_ptr(), clusters, 4, *out.args()) == 0
        d.sync()
        assert out.written(0)[0].tolist() == [0] * (clusters + 1)
    assert _counts_dev(d, pk, 0, 9).tolist() == [[0, 0, 0, 0]] * 9
    assert d.site_counts(sym[:0]).shape == (s, 4) and d.site_counts(sym[:, :0]).shape == (0, 4)
    got = d.cluster_snps(sym[:, :0], labs["one"])
    assert [o.tolist() for o in got[0]] == [[0, 0]] and len(got[1]) == 0
