"""distance subcommand: all-pairs SNP distances from snpma.fasta.

Host mirror of snppipeline/distance.py:14-118.  The pair counting (utils.calculate_sequence_distance for every pair)
runs in the HIP distance kernel (csrc/distance.hip) behind ``Device.distance``; this file parses the multi-FASTA,
orders the ids and writes the two TSV layouts.
"""
from __future__ import print_function

import os

import numpy as np

from . import snp_matrix
from . import utils


def distance_matrix(dev, seqs):
    """seqs: {id: sequence}.  Returns (sorted ids, (n, n) int32 matrix).

    Unequal lengths behave as in the reference: utils.calculate_sequence_distance (utils.py:1156-1158) walks
    range(len(seq1)) for every pair of itertools.combinations(sorted ids) — a longer second sequence is simply cut, a shorter
    one raises IndexError at seq2[pos].  So the lengths must be non-decreasing in sorted-id order, and a pair is compared over
    the length of its first sequence: the shorter rows are padded with '-' (never counted) and the kernel does the rest."""
    ids = sorted(seqs.keys())
    n = len(ids)
    if n == 0:
        return ids, np.zeros((0, 0), dtype=np.int32)
    lens = [len(seqs[i]) for i in ids]
    for a, b in zip(lens, lens[1:]):
        if b < a:
            raise IndexError("string index out of range")                     # what seq2[pos] raises in utils.py:1158
    s = lens[-1]
    if s == 0:
        return ids, np.zeros((n, n), dtype=np.int32)
    sym = np.full((n, s), 0x2D, dtype=np.uint8)
    for r, i in enumerate(ids):
        sym[r, :lens[r]] = np.frombuffer(seqs[i].encode("latin-1"), dtype=np.uint8)
    return ids, dev.distance(sym)


def _sorted_rows(file_ids, sym, lens):
    """The arrays of snp_matrix.load_matrix in the order the distance step works in: equal ids keep their last record (the
    reference's dict, distance.py:80-84), rows go into sorted-id order, lengths follow the rule of distance_matrix.  Returns
    (ids, rows): rows is None without records, else the (n, s) byte matrix (s may be 0)."""
    last = {}
    for r, i in enumerate(file_ids):
        last[i] = r
    ids = sorted(last)
    rows = np.asarray([last[i] for i in ids], dtype=np.int64)
    n = len(ids)
    if n == 0:
        return ids, None
    ordered = lens[rows]
    if (ordered[1:] < ordered[:-1]).any():
        raise IndexError("string index out of range")                         # what seq2[pos] raises in utils.py:1158
    if sym.shape[1] == 0:
        return ids, np.zeros((n, 0), dtype=np.uint8)
    if not np.array_equal(rows, np.arange(len(file_ids))):
        sym = sym[rows]                                                         # (snp_matrix writes sorted sample order: usually a no-op)
    return ids, np.ascontiguousarray(sym)


def distance_of_matrix(dev, file_ids, sym, lens):
    """distance_matrix for the arrays of snp_matrix.load_matrix (no Python strings in between)."""
    ids, rows = _sorted_rows(file_ids, sym, lens)
    n = len(ids)
    if rows is None:
        return ids, np.zeros((0, 0), dtype=np.int32)
    if rows.shape[1] == 0:
        return ids, np.zeros((n, n), dtype=np.int32)
    return ids, dev.distance(rows)


def close_pairs_of_matrix(dev, file_ids, sym, lens, threshold, want_matrix=False):
    """As distance_of_matrix, but only what lies within `threshold` SNPs comes back: (ids, row_off, col, dist), per id the
    entries d <= threshold of its row of the matrix in ascending column order, the diagonal included — the rows of the pairwise
    file (distance.py:100-106) under the threshold.  The matrix is computed and thresholded on the device and stays there;
    want_matrix (the two tables are wanted as well) adds it as a fifth value, from the same computation."""
    ids, rows = _sorted_rows(file_ids, sym, lens)
    if rows is None:
        empty = (ids, np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.int32))
        return empty + (np.zeros((0, 0), dtype=np.int32),) if want_matrix else empty
    return (ids,) + tuple(dev.close_pairs(rows, threshold, want_matrix=want_matrix))


def filter_pairs(row_off, col, dist, threshold):
    """The entries d <= threshold of a CSR, in place and order."""
    keep = np.asarray(dist) <= threshold
    kept_before = np.concatenate((np.zeros(1, dtype=np.uint64), np.cumsum(keep, dtype=np.uint64)))
    return kept_before[np.asarray(row_off, dtype=np.int64)], np.asarray(col)[keep], np.asarray(dist)[keep]


def cluster_thresholds(values):
    """Thresholds as the clusters file lists them: ascending, each once."""
    return sorted(set(int(v) for v in values))


def _id_table(ids):
    names = [i.encode("utf-8") for i in ids]
    off = np.zeros(len(names) + 1, dtype=np.uint64)
    np.cumsum([len(b) for b in names], out=off[1:])
    return b"".join(names), off


class _Ids(object):
    """The ids of a table among the arguments of _write: its bytes, its offsets and its count."""
    def __init__(self, ids):
        self.ids = ids


def _as(dtype, *arrays):
    return [np.ascontiguousarray(x, dtype=dtype) for x in arrays]


def _opt(x):
    """An array the library wants to see as NULL when it is empty."""
    return x if x.size else None


def _write(entry, path, args, arg_error=None):
    """One call of a writer of csrc/tsv_out.hip.  args, behind the path: _Ids for an id table, an array for its address, anything
    else as it is.  E_IO raises IOError, E_ARG ValueError(arg_error) when the writer has one, every other failure RuntimeError."""
    from . import _lib as L
    flat, keep = [], []
    for x in args:
        if isinstance(x, _Ids):
            blob, off = _id_table(x.ids)
            keep.append(off)
            flat += [blob, off.ctypes.data, len(x.ids)]
        else:
            flat.append(x.ctypes.data if isinstance(x, np.ndarray) else x)
    rc = getattr(L.load(), entry)(path.encode(), *flat)
    if rc == L.E_IO:
        raise IOError("cannot write %s" % path)
    if rc == L.E_ARG and arg_error is not None:
        raise ValueError(arg_error)
    if rc != 0:
        raise RuntimeError("%s failed (%d)" % (entry, rc))


def write_pair_rows(path, a_ids, b_ids, a, b, dist, compared):
    """Header and "id\tid\tdistance\tcompared" rows of pair lists in the order given (csrc/tsv_out.hip): a names ids of a_ids, b of
    b_ids — the rows of a close-pairs, tree or nearest file with the fourth column of --amdCompared."""
    a, b = _as(np.uint32, a, b)
    d, c = _as(np.int32, dist, compared)
    if not len(a) == len(b) == len(d) == len(c):
        raise ValueError("a, b, dist and compared hold one entry per row")
    _write("snpgpu_write_pair_rows_tsv", path, [_Ids(a_ids), _Ids(b_ids), _opt(a), _opt(b), _opt(d), _opt(c), len(a)],
           "a row names a sample outside the %d and %d ids" % (len(a_ids), len(b_ids)))


def rows_of_csr(row_off):
    """The row of every entry of a CSR."""
    row_off = np.asarray(row_off, dtype=np.int64)
    return np.repeat(np.arange(len(row_off) - 1, dtype=np.uint32), np.diff(row_off))


def write_close_pairs(path, ids, row_off, col, dist, compared=None):
    """Header and "id\tid\tdistance" rows of a CSR over ids, row by row, through the library's host formatter (csrc/tsv_out.hip);
    compared (one count per entry): a fourth column."""
    if compared is not None:
        return write_pair_rows(path, ids, ids, rows_of_csr(row_off), col, dist, compared)
    _write("snpgpu_write_close_pairs_tsv", path, [_Ids(ids)] + _as(np.uint64, row_off) + _as(np.uint32, col) + _as(np.int32, dist))


def write_clusters(path, ids, thresholds, numbers):
    """"Id" and the thresholds, then per id its cluster number at each threshold; numbers: (len(thresholds), len(ids)) uint32."""
    thr, = _as(np.int32, thresholds)
    num = _as(np.uint32, numbers)[0].reshape(len(thr), len(ids))
    _write("snpgpu_write_clusters_tsv", path, [_Ids(ids), thr, len(thr), num])


def write_pairs_and_clusters(dev, ids, row_off, col, dist, pairs_file, max_pair_distance, clusters_file, thresholds, pairs_compared=None, want_numbers=False):
    """The two additive outputs from one CSR that holds at least every entry within the largest threshold asked for;
    pairs_compared: the fourth column of the pairs file, one count per entry within max_pair_distance.  Returns the cluster
    numbers (len(cluster_thresholds(thresholds)), n) when a clusters file or want_numbers asked for them, else None."""
    if pairs_file:
        write_close_pairs(pairs_file, ids, *filter_pairs(row_off, col, dist, max_pair_distance), compared=pairs_compared)
    numbers = None
    if clusters_file or want_numbers:
        thresholds = cluster_thresholds(thresholds)
        numbers, _ = dev.clusters(len(ids), row_off, col, dist, thresholds)
    if clusters_file:
        write_clusters(clusters_file, ids, thresholds, numbers)
    return numbers


def mst_of_matrix(dev, file_ids, sym, lens, want_matrix=False, pairs_within=None):
    """As close_pairs_of_matrix, but what comes back is the minimum spanning tree of the samples: (ids, u, v, dist), the n - 1
    edges {u, v}, u < v, of the tree Kruskal builds under the edge order (d, u, v), in that order; built on the device, where the
    matrix stays.  pairs_within = T adds the CSR (row_off, col, dist) of close_pairs_of_matrix at T, want_matrix the matrix, each
    from the same computation: (ids, u, v, dist[, csr][, matrix])."""
    ids, rows = _sorted_rows(file_ids, sym, lens)
    if rows is None:
        rows = np.zeros((0, 0), dtype=np.uint8)
    return (ids,) + tuple(dev.mst(rows, want_matrix=want_matrix, pairs_within=pairs_within))


def mst_of_edges(n, u, v, dist):
    """Kruskal under the edge order (d, min, max) over an edge list on n nodes (duplicates and both orientations allowed): the
    minimum spanning forest (u, v, dist), u < v, in that order.  Merges the forests the ranks found in their bands."""
    from . import _lib as L
    u = np.ascontiguousarray(u, dtype=np.uint32)
    v = np.ascontiguousarray(v, dtype=np.uint32)
    d = np.ascontiguousarray(dist, dtype=np.int32)
    if not len(u) == len(v) == len(d):
        raise ValueError("u, v and dist hold one entry per edge")
    room = max(min(len(u), max(int(n) - 1, 0)), 1)
    ou, ov, od = np.zeros(room, dtype=np.uint32), np.zeros(room, dtype=np.uint32), np.zeros(room, dtype=np.int32)
    out_n = L.C.c_uint32(0)
    rc = L.load().snpgpu_mst_of_edges(int(n), u.ctypes.data, v.ctypes.data, d.ctypes.data, len(u), ou.ctypes.data, ov.ctypes.data, od.ctypes.data, L.C.byref(out_n))
    if rc == L.E_ARG:
        raise ValueError("an edge names a node outside 0 ... %d or joins a node to itself" % (int(n) - 1))
    if rc != 0:
        raise RuntimeError("snpgpu_mst_of_edges failed (%d)" % rc)
    k = int(out_n.value)
    return ou[:k], ov[:k], od[:k]


def _write_tree(entry, path, ids, u, v, dist):
    u, v = _as(np.uint32, u, v)
    _write(entry, path, [_Ids(ids), u, v] + _as(np.int32, dist) + [len(u)], "the edges are not a spanning tree of the %d ids in ascending order" % len(ids))


def write_mst(path, ids, u, v, dist, compared=None):
    """Header and one "id\tid\tdistance" row per tree edge, in the order given; compared (one count per edge): a fourth column."""
    if compared is not None:
        return write_pair_rows(path, ids, ids, u, v, dist, compared)
    _write_tree("snpgpu_write_mst_tsv", path, ids, u, v, dist)


def write_dendrogram(path, ids, u, v, dist):
    """The single-linkage dendrogram of a spanning tree whose edges come in ascending order, as one Newick line: each edge joins
    the groups of its ends at height d / 2 (csrc/tsv_out.hip)."""
    _write_tree("snpgpu_write_dendrogram_newick", path, ids, u, v, dist)


def _merge_arrays(a, b, size_a, size_b, num):
    arrays = _as(np.uint32, a, b, size_a, size_b) + _as(np.uint64, num)
    if len(set(len(x) for x in arrays)) != 1:
        raise ValueError("a, b, size_a, size_b and num hold one entry per merge")
    return arrays


def linkage_cut(kind, n, a, b, size_a, size_b, num, thresholds):
    """Cluster numbers (len(thresholds), n) uint32 of a merge list at every threshold, numbered as Device.clusters numbers them:
    a merge belongs to T when num <= T (complete) or num <= T * size_a * size_b (average)."""
    from . import _lib as L
    from .device import Device
    arrays = _merge_arrays(a, b, size_a, size_b, num)
    thr = np.ascontiguousarray(thresholds, dtype=np.int32)
    numbers = np.zeros((len(thr), int(n)), dtype=np.uint32)
    counts = np.zeros(len(thr), dtype=np.uint32)
    opt = lambda x: x.ctypes.data if x.size else None          # noqa: E731
    rc = L.load().snpgpu_linkage_cut(Device._linkage_kind(kind), int(n), *([opt(x) for x in arrays] + [len(arrays[0]), opt(thr), len(thr), opt(numbers), opt(counts)]))
    if rc != 0:
        raise ValueError("the merges are not those of a tree of %d samples" % int(n))
    return numbers, counts


def _write_linkage(entry, path, ids, kind, a, b, size_a, size_b, num):
    from .device import Device
    arrays = _merge_arrays(a, b, size_a, size_b, num)
    _write(entry, path, [_Ids(ids), Device._linkage_kind(kind)] + [_opt(x) for x in arrays] + [len(arrays[0])],
           "the merges are not those of a tree of the %d ids" % len(ids))


def write_linkage_merges(path, ids, kind, a, b, size_a, size_b, num):
    """Header and one "id\tid\tsize\tsize\tdistance" row per merge, in the order given; the distance of average linkage has six
    decimals, rounded half up in integers (csrc/tsv_out.hip)."""
    _write_linkage("snpgpu_write_linkage_tsv", path, ids, kind, a, b, size_a, size_b, num)


def write_linkage_dendrogram(path, ids, kind, a, b, size_a, size_b, num):
    """The tree of the n - 1 merges as one Newick line: a join lies at half the distance of its two clusters, in millionths."""
    _write_linkage("snpgpu_write_linkage_newick", path, ids, kind, a, b, size_a, size_b, num)


def write_linkage_outputs(ids, kind, merges, merges_file, dendrogram_file, clusters_file, thresholds):
    """The three additive outputs of one tree."""
    if merges_file:
        write_linkage_merges(merges_file, ids, kind, *merges)
    if dendrogram_file:
        write_linkage_dendrogram(dendrogram_file, ids, kind, *merges)
    if clusters_file:
        thresholds = cluster_thresholds(thresholds)
        numbers, _ = linkage_cut(kind, len(ids), *(tuple(merges) + (thresholds,)))
        write_clusters(clusters_file, ids, thresholds, numbers)


def _support_counts(support, replicates, merges):
    support = np.ascontiguousarray(support, dtype=np.uint32)
    if replicates is None or not 1 <= int(replicates) < 2 ** 32:
        raise ValueError("support values need the number of replicates, 1 at least")
    if len(support) != merges:
        raise ValueError("one support count per merge")
    return support


def write_nj(path, ids, a, b, len_a, len_b, star, star_len, support=None, replicates=None):
    """The neighbour-joining tree (the values of Device.nj) as one Newick line: a trifurcation at the top, lengths in SNPs written
    from integer millionths (csrc/nj_host.h).  With support (the last value of Device.nj_bootstrap) and replicates every join node
    carries floor((200 support + replicates) / (2 replicates)) between its ")" and its ":"."""
    a, b = _as(np.uint32, a, b)
    len_a, len_b = _as(np.int64, len_a, len_b)
    if not len(a) == len(b) == len(len_a) == len(len_b) or len(star) != 3 or len(star_len) != 3:
        raise ValueError("a, b, len_a and len_b hold one entry per merge, the star three slots and three lengths")
    star = np.asarray([0xFFFFFFFF if s is None else int(s) for s in star], dtype=np.uint32)
    star_len = np.asarray([int(x) for x in star_len], dtype=np.int64)
    args = [_Ids(ids), _opt(a), _opt(b), _opt(len_a), _opt(len_b), len(a), star, star_len]
    wrong = "the merges and the star are not a neighbour-joining tree of the %d ids" % len(ids)
    if support is None:
        _write("snpgpu_write_nj_newick", path, args, wrong)
    else:
        support = _support_counts(support, replicates, len(a))
        _write("snpgpu_write_nj_newick_support", path, args + [_opt(support), int(replicates)], wrong + ", or a count exceeds the replicates")


def write_nj_support(path, ids, a, b, support, replicates):
    """The support table of the joins (a, b of Device.nj_bootstrap, its counts) in round order: Seq1, Seq2 the ids of the two slots,
    Size the leaves under the new node, Support the count, Replicates."""
    a, b = _as(np.uint32, a, b)
    if len(a) != len(b):
        raise ValueError("a and b hold one entry per merge")
    support = _support_counts(support, replicates, len(a))
    _write("snpgpu_write_nj_support", path, [_Ids(ids), _opt(a), _opt(b), len(a), _opt(support), int(replicates)],
           "the merges are not the joins of a neighbour-joining tree of the %d ids, or a count exceeds the replicates" % len(ids))


def pairs_of_csr(row_off, col, dist, threshold):
    """The entries i < j, d <= threshold of a CSR in its order: (a, b, d) — each unordered pair of the close-pairs file once."""
    row_off = np.asarray(row_off, dtype=np.int64)
    col = np.asarray(col, dtype=np.uint32)
    dist = np.asarray(dist, dtype=np.int32)
    row = np.repeat(np.arange(len(row_off) - 1, dtype=np.uint32), np.diff(row_off))
    keep = (row < col) & (dist <= threshold)
    return row[keep], col[keep], dist[keep]


def pair_sites_of_matrix(dev, file_ids, sym, lens, a, b, expect=None):
    """The columns at which the pairs (a[p], b[p]) of samples — indices into the sorted ids, as everywhere in the distance step —
    differ: (ids, pair_off, site, bases) as Device.pair_sites lays them out.  Pair p has as many entries as the matrix says at
    [a[p]][b[p]]; expect is their sum when the caller has it.  Nothing but the pair lists and the entries crosses the host link
    besides the symbols themselves."""
    ids, rows = _sorted_rows(file_ids, sym, lens)
    if rows is None:
        rows = np.zeros((0, 0), dtype=np.uint8)
    return (ids,) + tuple(dev.pair_sites(rows, a, b, expect=expect))


def site_table(snp_list):
    """[(chrom, pos)] per column (utils.read_snp_position_list) as the arrays the writer takes."""
    names, index = [], {}
    chrom_of = np.zeros(len(snp_list), dtype=np.uint32)
    pos_of = np.zeros(len(snp_list), dtype=np.uint64)
    for k, (chrom, pos) in enumerate(snp_list):
        if chrom not in index:
            index[chrom] = len(names)
            names.append(chrom.encode("utf-8"))
        if pos < 0:
            raise ValueError("negative position %d of %s" % (pos, chrom))
        chrom_of[k] = index[chrom]
        pos_of[k] = pos
    off = np.zeros(len(names) + 1, dtype=np.uint64)
    np.cumsum([len(x) for x in names], out=off[1:])
    return b"".join(names), off, chrom_of, pos_of


def write_pair_sites(path, ids, a, b, pair_off, site, bases, snp_list=None):
    """One row per differing site of every pair, in the order given (csrc/tsv_out.hip): "id\tid\tcolumn\tbase\tbase" with
    1-based columns, or — snp_list: the (chrom, pos) of every column — "id\tid\tchrom\tpos\tbase\tbase"."""
    a, b = _as(np.uint32, a, b)
    po, = _as(np.uint64, pair_off)
    st, = _as(np.uint32, site)
    bs, = _as(np.uint8, bases)
    if len(a) != len(b) or len(po) != len(a) + 1 or len(st) != len(bs) or int(po[-1]) != len(st):
        raise ValueError("pair_off holds one offset per pair and one more, site and bases one entry per offset")
    if snp_list is not None and len(st) and int(st.max()) >= len(snp_list):
        raise ValueError("a site lies beyond the %d columns of the site list" % len(snp_list))
    _write("snpgpu_write_pair_sites_tsv", path, [_Ids(ids), _opt(a), _opt(b), len(a), po, _opt(st), _opt(bs)] + _site_table_args(snp_list, len(snp_list or ())),
           "a pair names a sample outside the %d ids, or the offsets do not rise from 0" % len(ids))


def _site_table_args(snp_list, columns):
    """The last four arguments of the site writers: all None without a list, else the arrays of site_table."""
    if snp_list is None:
        return [None, None, None, None]
    if len(snp_list) != columns:
        raise ValueError("the site list names %d sites, the matrix has %d columns" % (len(snp_list), columns))
    table = list(site_table(snp_list))
    if columns == 0:                                           # a list without columns: the writer still wants to see a table
        table[2:] = [np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint64)]
    return table


def write_site_counts(path, counts, n_rows, snp_list=None):
    """"Site\tA\tC\tG\tT\tOther" and one row per column of counts ((s, 4): the rows that hold A, C, G, T), Other = n_rows minus
    the four (csrc/tsv_out.hip); 1-based columns, or — snp_list: the (chrom, pos) of every column — Chrom and Pos in their place."""
    c = _as(np.int32, counts)[0].reshape(-1, 4)
    _write("snpgpu_write_site_counts_tsv", path, [_opt(c), len(c), int(n_rows)] + _site_table_args(snp_list, len(c)),
           "the counts of a column are negative or exceed the %d rows" % int(n_rows))


def write_cluster_snps(path, thresholds, sizes, cluster_off, site, base, members, columns, snp_list=None):
    """"Threshold\tCluster\tSite\tBase\tMembers\tSize" and one row per entry of Device.cluster_snps, labelling t under
    thresholds[t]: sizes and cluster_off are lists with one array per labelling (the sizes of its clusters; their offsets and
    one more).  columns: the width of the matrix.  snp_list as for write_site_counts."""
    thr, = _as(np.int32, thresholds)
    if not len(thr) == len(sizes) == len(cluster_off) or any(len(o) != len(z) + 1 for o, z in zip(cluster_off, sizes)):
        raise ValueError("one array of sizes and one of offsets (one more) per threshold")
    ncl = np.asarray([len(z) for z in sizes], dtype=np.uint32)
    sz, = _as(np.uint32, np.concatenate([np.asarray(z, dtype=np.uint32) for z in sizes]) if len(sizes) else np.zeros(0))
    off, = _as(np.uint64, np.concatenate([np.asarray(o, dtype=np.uint64) for o in cluster_off]) if len(sizes) else np.zeros(0))
    st, mb = _as(np.uint32, site, members)
    bs, = _as(np.uint8, base)
    if not len(st) == len(bs) == len(mb) or (len(off) and int(off[-1]) != len(st)):
        raise ValueError("site, base and members hold one entry per offset")
    _write("snpgpu_write_cluster_snps_tsv", path,
           [_opt(thr), _opt(ncl), len(thr), _opt(off), _opt(sz), _opt(st), _opt(bs), _opt(mb), int(columns)] + _site_table_args(snp_list, int(columns)),
           "an entry names a site beyond the %d columns or a base above 3, or the offsets do not rise from 0" % int(columns))


def write_cluster_snps_of_numbers(device_of, path, rows, thresholds, numbers, snp_list=None):
    """--amdClusterSnps: the file for the cluster numbers (len(thresholds), n) of --amdClusters over the sorted rows (None:
    no record).  One more upload and pack of the rows; nothing but the labels and the entries crosses the host link besides."""
    numbers = np.asarray(numbers, dtype=np.uint32).reshape(len(thresholds), -1)
    n = numbers.shape[1]
    columns = 0 if rows is None else rows.shape[1]
    sizes = [np.bincount(row, minlength=1)[1:].astype(np.uint32) for row in numbers]
    if n == 0 or columns == 0:
        got = ([np.zeros(len(z) + 1, dtype=np.uint64) for z in sizes], np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint32))
    else:
        got = device_of().cluster_snps(rows, numbers, n_clusters=[len(z) for z in sizes])
    write_cluster_snps(path, thresholds, sizes, *got, columns=columns, snp_list=snp_list)


def read_pair_list(path, ids):
    """The pairs of a user's two-column TSV of ids as indices into ids: (a, b).  Further columns are ignored and so is a first
    line "Seq1\tSeq2...", so a close-pairs or tree file of this step can be handed back as it is.  An id the matrix does not
    hold is a global error that names it."""
    index = {name: k for k, name in enumerate(ids)}
    a, b = [], []
    with open(path, "r") as f:
        for number, line in enumerate(f):
            fields = line.rstrip("\r\n").split("\t")
            if not line.strip() or (number == 0 and fields[:2] == ["Seq1", "Seq2"]):
                continue
            if len(fields) < 2:
                utils.global_error("Error: line %d of %s does not hold two ids." % (number + 1, path))
            for name in fields[:2]:
                if name not in index:
                    utils.global_error("Error: the id %s of %s is not in the snp matrix." % (name, path))
            a.append(index[fields[0]])
            b.append(index[fields[1]])
    return np.asarray(a, dtype=np.uint32), np.asarray(b, dtype=np.uint32)


def query_rows(q_file_ids, q_sym, q_lens, columns):
    """The query records of a second multi-FASTA in the order the nearest-neighbour output works in: equal ids keep their last
    record, rows go into sorted-id order.  columns: the width of the database matrix, which every query must have exactly (None:
    a database without records, nothing to compare with) — else a global error that names both counts.  Returns (ids, (q, s)
    byte matrix)."""
    last = {}
    for r, i in enumerate(q_file_ids):
        last[i] = r
    ids = sorted(last)
    rows = np.asarray([last[i] for i in ids], dtype=np.int64)
    if columns is not None:
        for i, r in zip(ids, rows):
            if int(q_lens[r]) != columns:
                utils.global_error("Error: the query %s has %d columns, the snp matrix has %d columns." % (i, int(q_lens[r]), columns))
    if len(ids) == 0:
        return ids, np.zeros((0, columns or 0), dtype=np.uint8)
    return ids, np.ascontiguousarray(q_sym[rows])


def write_nearest(path, q_ids, db_ids, row_off, col, dist, compared=None):
    """Header and "query id\tdatabase id\tdistance" rows of a CSR over the queries whose columns are database samples, query by
    query, through the library's host formatter (csrc/tsv_out.hip); compared (one count per entry): a fourth column."""
    if compared is not None:
        if len(row_off) != len(q_ids) + 1:
            raise ValueError("row_off holds one offset per query and one more")
        return write_pair_rows(path, q_ids, db_ids, rows_of_csr(row_off), col, dist, compared)
    ro, = _as(np.uint64, row_off)
    c, = _as(np.uint32, col)
    d, = _as(np.int32, dist)
    if len(ro) != len(q_ids) + 1 or len(c) != len(d) or int(ro[-1]) != len(c):
        raise ValueError("row_off holds one offset per query and one more, col and dist one entry per offset")
    _write("snpgpu_write_nearest_tsv", path, [_Ids(q_ids), _Ids(db_ids), ro, _opt(c), _opt(d)],
           "a column names a sample outside the %d database ids, or the offsets do not rise from 0" % len(db_ids))


def _write_tsv(path, layout, ids, mat):
    """distance.py:100-114 through the library's host formatter (csrc/tsv_out.hip): at 10 000 samples the pairwise file has
    10^8 lines, ~35 s of Python string formatting for 38 ms of kernel."""
    m, = _as(np.int32, mat)
    _write("snpgpu_write_distance_tsv", path, [layout, _Ids(ids), m, m.shape[1] if m.ndim == 2 else 0])


def compared_of_matrix(device_of, file_ids, sym, lens):
    """As distance_of_matrix, but entry (i, j) is Compared: at how many columns both samples hold one of ACGT (either case) — the
    columns a distance counts over; the diagonal is each sample's own count (csrc/compared.hip).  device_of: asked only when there
    is something to count."""
    ids, rows = _sorted_rows(file_ids, sym, lens)
    n = len(ids)
    if rows is None or rows.shape[1] == 0:
        return ids, np.zeros((n, n), dtype=np.int32)
    return ids, device_of().compared(rows)


def compared_columns(dev, rows, pairs_csr, tree):
    """--amdCompared: the fourth column of the close-pairs file (pairs_csr: its (row_off, col, dist), or None) and of the tree
    file (tree: its (u, v, dist), or None) from one upload, pack and plane of the sorted rows: (per entry, per edge), None where
    not asked for.  The pairs are the host lists the other outputs returned; the n x n matrix is never formed."""
    lists = []
    if pairs_csr is not None:
        lists.append((rows_of_csr(pairs_csr[0]), np.asarray(pairs_csr[1], dtype=np.uint32)))
    if tree is not None:
        lists.append((np.asarray(tree[0], dtype=np.uint32), np.asarray(tree[1], dtype=np.uint32)))
    total = sum(len(a) for a, _ in lists)
    if total == 0 or rows is None:
        counts = np.zeros(total, dtype=np.int32)
    else:
        counts = dev.compared_pairs(rows, np.concatenate([a for a, _ in lists]), np.concatenate([b for _, b in lists]))
    first = len(lists[0][0]) if pairs_csr is not None else 0
    return (counts[:first] if pairs_csr is not None else None), (counts[first:] if tree is not None else None)


def write_pairwise(path, ids, mat):
    _write_tsv(path, 0, ids, mat)


def write_matrix(path, ids, mat):
    _write_tsv(path, 1, ids, mat)


def calculate_snp_distances(args):
    """Entry point of ``cfsan_snp_pipeline distance`` (cfsan_snp_pipeline.py:448-457)."""
    utils.print_log_header()
    utils.print_arguments(args)

    o = DistanceOptions()
    o.input_file = args.inputFile
    o.pairwise_file = args.pairwiseFile
    o.matrix_file = args.matrixFile
    # extensions of this build (absent when the Namespace comes from the reference's own parser)
    o.close_file = getattr(args, "amdClosePairsFile", None)
    o.max_pair_distance = getattr(args, "amdMaxPairDistance", None)
    o.clusters_file = getattr(args, "amdClustersFile", None)
    o.thresholds = list(getattr(args, "amdClusterThresholds", None) or [])
    o.mst_file = getattr(args, "amdMstFile", None)
    o.dendrogram_file = getattr(args, "amdDendrogramFile", None)
    o.close_sites_file = getattr(args, "amdClosePairSitesFile", None)
    o.mst_sites_file = getattr(args, "amdMstSitesFile", None)
    o.user_pairs_file = getattr(args, "amdPairSitesPairsFile", None)
    o.user_sites_file = getattr(args, "amdPairSitesOutFile", None)
    o.snp_list_file = getattr(args, "amdSnpListFile", None)
    o.linkage_kind = getattr(args, "amdLinkage", None)
    o.linkage_files = (getattr(args, "amdLinkageMergesFile", None), getattr(args, "amdLinkageDendrogramFile", None), getattr(args, "amdLinkageClustersFile", None))
    o.query_file = getattr(args, "amdQueryFile", None)
    o.nearest_file = getattr(args, "amdNearestFile", None)
    o.nearest_count = getattr(args, "amdNearestCount", None)
    o.compared_matrix_file = getattr(args, "amdComparedMatrixFile", None)
    o.with_compared = bool(getattr(args, "amdCompared", False))
    o.site_counts_file = getattr(args, "amdSiteCountsFile", None)
    o.cluster_snps_file = getattr(args, "amdClusterSnpsFile", None)
    o.nj_file = getattr(args, "amdNjFile", None)
    o.nj_bootstrap = getattr(args, "amdNjBootstrap", None)
    o.nj_seed = getattr(args, "amdNjSeed", None)
    o.nj_support_file = getattr(args, "amdNjSupportFile", None)
    if utils.verify_existing_input_files("SNP matrix file", [o.input_file]) > 0:
        utils.global_error("Error: cannot calculate sequence distances without the snp matrix file.")
    if o.close_file and o.max_pair_distance is None:
        utils.global_error("Error: --amdClosePairs needs --amdMaxPairDistance.")
    if o.close_sites_file and o.max_pair_distance is None:
        utils.global_error("Error: --amdClosePairSites needs --amdMaxPairDistance.")
    if bool(o.user_pairs_file) != bool(o.user_sites_file):
        utils.global_error("Error: --amdPairSitesPairs and --amdPairSitesOut go together.")
    if o.user_pairs_file and utils.verify_existing_input_files("pair list file", [o.user_pairs_file]) > 0:
        utils.global_error("Error: cannot list the differing sites without the pair list file.")
    if o.cluster_snps_file and not o.thresholds:
        utils.global_error("Error: --amdClusterSnps needs at least one threshold in --amdClusterThresholds.")
    if o.snp_list_file and (o.site_counts_file or o.cluster_snps_file) and not os.path.isfile(o.snp_list_file):
        utils.global_error("Error: --amdSnpList: cannot name the sites of --amdSiteCounts and --amdClusterSnps without the snplist file %s." % o.snp_list_file)
    if o.snp_list_file and utils.verify_existing_input_files("snplist file", [o.snp_list_file]) > 0:
        utils.global_error("Error: cannot name the differing sites without the snplist file.")
    if o.clusters_file and not o.thresholds:
        utils.global_error("Error: --amdClusters needs at least one threshold in --amdClusterThresholds.")
    if any(o.linkage_files) and not o.linkage_kind:
        utils.global_error("Error: --amdLinkageMerges, --amdLinkageDendrogram and --amdLinkageClusters need --amdLinkage.")
    if o.linkage_kind and not any(o.linkage_files):
        utils.global_error("Error: --amdLinkage needs at least one of --amdLinkageMerges, --amdLinkageDendrogram and --amdLinkageClusters.")
    if o.linkage_files[2] and not o.thresholds:
        utils.global_error("Error: --amdLinkageClusters needs at least one threshold in --amdClusterThresholds.")
    if (o.max_pair_distance is not None and o.max_pair_distance < 0) or any(t < 0 for t in o.thresholds):
        utils.global_error("Error: a distance threshold cannot be negative.")
    if bool(o.query_file) != bool(o.nearest_file):
        utils.global_error("Error: --amdQuery and --amdNearest go together.")
    if o.nearest_count is not None and not o.nearest_file:
        utils.global_error("Error: --amdNearestCount needs --amdQuery and --amdNearest.")
    if o.nearest_count is not None and o.nearest_count < 0:
        utils.global_error("Error: --amdNearestCount cannot be negative.")
    if o.query_file and utils.verify_existing_input_files("query file", [o.query_file]) > 0:
        utils.global_error("Error: cannot find the nearest samples without the query file.")
    if o.with_compared and not (o.close_file or o.mst_file or o.nearest_file):
        utils.global_error("Error: --amdCompared needs at least one of --amdClosePairs, --amdMst and --amdNearest.")
    if o.nj_support_file and o.nj_bootstrap is None:
        utils.global_error("Error: --amdNjSupport needs --amdNjBootstrap.")
    if o.nj_bootstrap is not None and not (o.nj_file or o.nj_support_file):
        utils.global_error("Error: --amdNjBootstrap needs at least one of --amdNj and --amdNjSupport.")
    if o.nj_seed is not None and o.nj_bootstrap is None:
        utils.global_error("Error: --amdNjSeed needs --amdNjBootstrap.")
    if o.nj_bootstrap is not None and not 1 <= o.nj_bootstrap < 2 ** 32:
        utils.global_error("Error: --amdNjBootstrap takes a number of replicates of 1 at least (and below 2^32).")
    if o.nj_seed is not None and not 0 <= o.nj_seed < 2 ** 64:
        utils.global_error("Error: --amdNjSeed takes a seed of 0 ... 2^64 - 1.")
    outputs = [f for f in (o.pairwise_file, o.matrix_file, o.close_file, o.clusters_file, o.mst_file, o.dendrogram_file, o.close_sites_file, o.mst_sites_file, o.user_sites_file, o.nearest_file,
                           o.compared_matrix_file, o.site_counts_file, o.cluster_snps_file, o.nj_file, o.nj_support_file) + o.linkage_files if f]
    if not outputs:
        utils.global_error("Error: no output file specified.")

    sources = [o.input_file] + [f for f in (o.user_pairs_file, o.snp_list_file) if f and (o.close_sites_file or o.mst_sites_file or o.user_sites_file)] + \
        ([o.snp_list_file] if o.snp_list_file and (o.site_counts_file or o.cluster_snps_file) and not (o.close_sites_file or o.mst_sites_file or o.user_sites_file) else []) + ([o.query_file] if o.query_file else [])
    if not (args.forceFlag or any(utils.target_needs_rebuild(sources, f) for f in outputs)):
        utils.verbose_print("Distance files have already been freshly built.  Use the -f option to force a rebuild.")
        return

    file_ids, sym, lens = snp_matrix.load_matrix(o.input_file)
    utils.verbose_print("# %s %s" % (utils.timestamp(), "Calculating all pairwise distances"))
    from .device import default_device
    named_sites = None
    if o.snp_list_file and (o.site_counts_file or o.cluster_snps_file):
        named_sites = utils.read_snp_position_list(o.snp_list_file)
        columns = _sorted_rows(file_ids, sym, lens)[1]
        columns = 0 if columns is None else columns.shape[1]
        if len(named_sites) != columns:
            utils.global_error("Error: %s lists %d sites, the snp matrix has %d columns." % (o.snp_list_file, len(named_sites), columns))
    on_their_own = 0
    if o.site_counts_file:
        # on its own, as the two below: one more upload and pack beside the other outputs; no matrix is computed for it
        ids, rows = _sorted_rows(file_ids, sym, lens)
        counts = default_device().site_counts(rows) if rows is not None and rows.size else np.zeros((0 if rows is None else rows.shape[1], 4), dtype=np.int32)
        write_site_counts(o.site_counts_file, counts, len(ids), snp_list=named_sites)
        on_their_own += 1
    if o.nearest_file:
        # the queries against the database, on their own: this first form uploads and packs the database itself, whatever else is
        # asked for, and the other outputs are computed as without it
        _write_nearest_output(default_device, file_ids, sym, lens, o.query_file, o.nearest_file, o.nearest_count or 0, o.max_pair_distance, o.with_compared)
        on_their_own += 1
    if o.compared_matrix_file:
        # likewise on its own: one more upload and pack beside the other outputs, and the matrix in the layout of -m
        write_matrix(o.compared_matrix_file, *compared_of_matrix(default_device, file_ids, sym, lens))
        on_their_own += 1
    if o.nj_bootstrap is not None:
        # the bootstrap on its own too: one more upload and pack beside the other outputs; the tree is the one --amdNj alone writes,
        # its join nodes carrying their support, and the shared path does not write it again
        ids, rows = _sorted_rows(file_ids, sym, lens)
        if rows is None:
            rows = np.zeros((0, 0), dtype=np.uint8)
        tree = default_device().nj_bootstrap(rows, o.nj_bootstrap, 1 if o.nj_seed is None else o.nj_seed)
        if o.nj_file:
            write_nj(o.nj_file, ids, *tree[:6], support=tree[6], replicates=o.nj_bootstrap)
            on_their_own += 1
        if o.nj_support_file:
            write_nj_support(o.nj_support_file, ids, tree[0], tree[1], tree[6], o.nj_bootstrap)
            on_their_own += 1
    if len(outputs) == on_their_own:
        return
    _write_distance_outputs(default_device, o, file_ids, sym, lens, named_sites)


class DistanceOptions(object):
    """What calculate_snp_distances was asked for: the output paths and the values that go with them, as attributes."""


class DistancePlan(object):
    """How the outputs of one run share their device work (distance_plan)."""


def distance_plan(o, n, columns):
    """The plan of the outputs that share one matrix, from the options and the shape of the sorted rows alone — no device:
        want_tree, want_matrix  the spanning tree / the n x n matrix on the host are needed
        widest                  the largest threshold a CSR of pairs has to hold (close pairs, their sites, clusters, cluster
                                SNPs), or None
        compute                 the one ``Device.distance_outputs`` call is made
        keep_packed             ... and leaves the packed matrix on the device for the site files
        host_matrix             linkage and neighbour joining take the matrix the host has (``*_of_matrix``); else each computes
                                its own where the matrix is built, and only its merges come to the host
    The symbols are uploaded and packed once and the matrix is computed once, and only when a tree, a threshold or a table needs
    it; the n x n matrix comes to the host for -p / -m alone."""
    p = DistancePlan()
    sites = bool(o.close_sites_file or o.mst_sites_file or o.user_sites_file)
    p.want_tree = bool(o.mst_file or o.dendrogram_file or o.mst_sites_file)
    p.want_matrix = bool(o.pairwise_file or o.matrix_file)
    within = ([o.max_pair_distance] if (o.close_file or o.close_sites_file) else []) + (o.thresholds if (o.clusters_file or o.cluster_snps_file) else [])
    p.widest = max(within) if within else None
    # Degenerate shapes keep the calls they have always made (the table of tests/test_distance_plan_cpu.py): beside a site file
    # no record means no call; without one a tree is asked for even of no record, and tables alone of no column are zeros
    if sites:
        p.compute = n > 0 and (p.want_tree or p.want_matrix or p.widest is not None)
    else:
        p.compute = p.want_tree or (n > 0 and (p.widest is not None or (p.want_matrix and columns > 0)))
    p.keep_packed = sites and p.compute
    p.host_matrix = p.want_matrix or (sites and n == 0)
    return p


def _write_distance_outputs(device_of, o, file_ids, sym, lens, named_sites):
    """The outputs of calculate_snp_distances that share one matrix, by distance_plan.  The inputs are checked before a device
    is asked for; the packed matrix stays on the device until every pair list has been answered from it."""
    ids, rows = _sorted_rows(file_ids, sym, lens)
    sorted_rows = rows                                         # (None without a record: nothing to upload)
    if rows is None:
        rows = np.zeros((0, 0), dtype=np.uint8)
    n, columns = rows.shape
    snp_list = None
    if o.snp_list_file and (o.close_sites_file or o.mst_sites_file or o.user_sites_file):
        snp_list = utils.read_snp_position_list(o.snp_list_file)
        if len(snp_list) != columns:
            utils.global_error("Error: %s lists %d sites, the snp matrix has %d columns." % (o.snp_list_file, len(snp_list), columns))
    user_pairs = read_pair_list(o.user_pairs_file, ids) if o.user_sites_file else None
    plan = distance_plan(o, n, columns)
    dev = device_of()                                          # (the inputs have been checked: only now is a device needed)
    if plan.compute:
        tree, csr, mat = dev.distance_outputs(rows, want_tree=plan.want_tree, want_matrix=plan.want_matrix, pairs_within=plan.widest, keep_packed=plan.keep_packed)
    else:                                                      # nothing asks for the matrix, or a shape that has no entry to compute
        empty = np.zeros(0, dtype=np.uint32)
        tree, csr = (empty, empty, np.zeros(0, dtype=np.int32)), (np.zeros(1, dtype=np.uint64), empty, np.zeros(0, dtype=np.int32))
        mat = np.zeros((n, n), dtype=np.int32) if plan.host_matrix else None

    def sites_of(a, b, expect):
        if n == 0 or len(a) == 0:
            return np.zeros(len(a) + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint8)
        return dev.pair_sites_kept(a, b, expect=expect) if plan.keep_packed else dev.pair_sites(rows, a, b, expect=expect)

    try:
        if o.linkage_kind:
            merges = dev.linkage_of_matrix(mat, o.linkage_kind) if plan.host_matrix else dev.linkage(rows, o.linkage_kind)
            write_linkage_outputs(ids, o.linkage_kind, merges, o.linkage_files[0], o.linkage_files[1], o.linkage_files[2], o.thresholds)
        if o.nj_file and o.nj_bootstrap is None:
            write_nj(o.nj_file, ids, *(dev.nj_of_matrix(mat) if plan.host_matrix else dev.nj(rows)))
        if o.pairwise_file:
            write_pairwise(o.pairwise_file, ids, mat)
        if o.matrix_file:
            write_matrix(o.matrix_file, ids, mat)
        pairs_compared = tree_compared = None
        if o.with_compared:                                    # (not done: reuse of the kept packed matrix — one more upload and pack)
            pairs_compared, tree_compared = compared_columns(dev, sorted_rows, filter_pairs(csr[0], csr[1], csr[2], o.max_pair_distance) if o.close_file else None,
                                                             tree if o.mst_file else None)
        if o.close_file or o.clusters_file or o.cluster_snps_file:
            numbers = write_pairs_and_clusters(dev, ids, csr[0], csr[1], csr[2], o.close_file, o.max_pair_distance, o.clusters_file, o.thresholds, pairs_compared,
                                               want_numbers=bool(o.cluster_snps_file))
        if o.cluster_snps_file:                                # (not done: reuse of the kept packed matrix — one more upload and pack)
            write_cluster_snps_of_numbers(lambda: dev, o.cluster_snps_file, sorted_rows, cluster_thresholds(o.thresholds), numbers, snp_list=named_sites)
        if o.mst_file:
            write_mst(o.mst_file, ids, *tree, compared=tree_compared)
        if o.dendrogram_file:
            write_dendrogram(o.dendrogram_file, ids, *tree)
        if o.close_sites_file:
            a, b, d = pairs_of_csr(csr[0], csr[1], csr[2], o.max_pair_distance)
            write_pair_sites(o.close_sites_file, ids, a, b, *sites_of(a, b, int(d.sum(dtype=np.int64))), snp_list=snp_list)
        if o.mst_sites_file:
            u, v, d = tree
            write_pair_sites(o.mst_sites_file, ids, u, v, *sites_of(u, v, int(np.asarray(d).sum(dtype=np.int64))), snp_list=snp_list)
        if o.user_sites_file:
            a, b = user_pairs
            expect = int(mat[a.astype(np.int64), b.astype(np.int64)].sum(dtype=np.int64)) if (mat is not None and len(a)) else None
            write_pair_sites(o.user_sites_file, ids, a, b, *sites_of(a, b, expect), snp_list=snp_list)
    finally:
        if plan.keep_packed:
            dev.packed_drop()


def _write_nearest_output(device_of, file_ids, sym, lens, query_file, nearest_file, count, max_pair_distance, with_compared=False):
    """--amdNearest: the inputs are checked before a device is asked for; nothing but the lists crosses the host link.
    with_compared: the fourth column, the pairs (query row, database row) over the two matrices."""
    db_ids, db_rows = _sorted_rows(file_ids, sym, lens)
    q_file_ids, q_sym, q_lens = snp_matrix.load_matrix(query_file)
    q_ids, q_rows = query_rows(q_file_ids, q_sym, q_lens, None if db_rows is None else db_rows.shape[1])
    if db_rows is None or len(q_ids) == 0:                      # no pair at all: the header
        write_nearest(nearest_file, q_ids, db_ids, np.zeros(len(q_ids) + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.int32),
                      compared=np.zeros(0, dtype=np.int32) if with_compared else None)
        return
    dev = device_of()
    row_off, col, dist = dev.nearest(q_rows, db_rows, k=count, threshold=max_pair_distance)
    compared = dev.compared_pairs(q_rows, rows_of_csr(row_off), col, db_rows) if with_compared else None
    write_nearest(nearest_file, q_ids, db_ids, row_off, col, dist, compared=compared)
