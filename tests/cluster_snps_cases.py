"""The statements of the per-site allele counts and of the cluster-defining SNPs (csrc/cluster_snps.hip), in plain NumPy: what the
kernels, the library's host forms, the writers and the command are compared with.  Nothing here shares code with the package.

A byte is a base iff it is one of ACGT after upper-casing a-z (the distance's predicate); the bases are numbered A0 C1 G2 T3.

Site counts.   count[s][b] = the rows that hold base b at column s; Other(s) = n - the four.
Cluster SNPs.  For labels 1 ... C: (cluster c, column s, base b) is a row iff at least one member of c holds b at s, no member
               holds another base there, and no sample outside c holds b at s.  Members = the members of c that hold b at s.
               Rows come by cluster, then column."""
import numpy as np

from tests.nearest_cases import random_symbols  # noqa: F401  (the symbols of the cases: alphabet ACGTACGTACGTacgt-N, or every byte)

BASES = b"ACGT"
COUNTS_HEADER = "Site\tA\tC\tG\tT\tOther\n"
COUNTS_HEADER_NAMED = "Chrom\tPos\tA\tC\tG\tT\tOther\n"
SNPS_HEADER = "Threshold\tCluster\tSite\tBase\tMembers\tSize\n"
SNPS_HEADER_NAMED = "Threshold\tCluster\tChrom\tPos\tBase\tMembers\tSize\n"


def base_codes(sym):
    """(n, s) uint8 -> (n, s) int8: 0..3 for A, C, G, T in either case, -1 for every other byte."""
    a = np.asarray(sym, dtype=np.uint8)
    upper = np.where((a >= 97) & (a <= 122), a - 32, a).astype(np.uint8)
    out = np.full(a.shape, -1, dtype=np.int8)
    for b, letter in enumerate(BASES):
        out[upper == letter] = b
    return out


def site_counts(sym):
    """(n, s) uint8 -> (s, 4) int32."""
    code = base_codes(sym)
    return np.stack([(code == b).sum(axis=0) for b in range(4)], axis=1).astype(np.int32).reshape(code.shape[1], 4)


def cluster_snps(sym, labels, n_clusters=None):
    """One labelling (n,) of the rows of sym: (cluster_off uint64 [C + 1], site uint32, base uint8, members uint32)."""
    code = base_codes(sym)
    labels = np.asarray(labels, dtype=np.int64)
    n, s = code.shape
    assert labels.shape == (n,)
    c_total = int(labels.max()) if n_clusters is None and n else int(n_clusters or 0)
    assert n == 0 or (labels.min() >= 1 and labels.max() <= c_total)
    holds = np.stack([code == b for b in range(4)])                 # (4, n, s)
    everywhere = holds.sum(axis=1)                                  # (4, s)
    off, site, base, members = [0], [], [], []
    for c in range(1, c_total + 1):
        inside = holds[:, labels == c, :].sum(axis=1)               # (4, s): members of c per base
        one_base = (inside > 0).sum(axis=0) == 1                    # some member holds a base, no member another
        cols = np.flatnonzero(one_base)
        b = np.argmax(inside[:, cols], axis=0)
        private = inside[b, cols] == everywhere[b, cols]            # nobody outside holds it
        site.extend(cols[private].tolist())
        base.extend(b[private].tolist())
        members.extend(inside[b, cols][private].tolist())
        off.append(len(site))
    return np.asarray(off, dtype=np.uint64), np.asarray(site, dtype=np.uint32), np.asarray(base, dtype=np.uint8), np.asarray(members, dtype=np.uint32)


def sizes_of(labels, n_clusters=None):
    labels = np.asarray(labels, dtype=np.int64)
    c_total = (int(labels.max()) if len(labels) else 0) if n_clusters is None else int(n_clusters)
    return np.bincount(labels, minlength=c_total + 1)[1:]


def _site_fields(col, snp_list):
    return "%d" % (col + 1) if snp_list is None else "%s\t%d" % (snp_list[col][0], snp_list[col][1])


def site_counts_text(sym, snp_list=None):
    sym = np.asarray(sym, dtype=np.uint8)
    n = sym.shape[0]
    counts = site_counts(sym)
    rows = ["%s\t%d\t%d\t%d\t%d\t%d\n" % ((_site_fields(col, snp_list),) + tuple(int(x) for x in c) + (n - int(c.sum()),)) for col, c in enumerate(counts)]
    return (COUNTS_HEADER if snp_list is None else COUNTS_HEADER_NAMED) + "".join(rows)


def cluster_snps_text(sym, thresholds, labellings, snp_list=None):
    """The file: the labelling of every threshold in the order given, by cluster, then column."""
    out = [SNPS_HEADER if snp_list is None else SNPS_HEADER_NAMED]
    for t, labels in zip(thresholds, labellings):
        off, site, base, members = cluster_snps(sym, labels)
        sizes = sizes_of(labels)
        for c in range(len(off) - 1):
            for e in range(int(off[c]), int(off[c + 1])):
                out.append("%d\t%d\t%s\t%s\t%d\t%d\n" % (t, c + 1, _site_fields(int(site[e]), snp_list), "ACGT"[base[e]], members[e], sizes[c]))
    return "".join(out)


def labellings(n, seed):
    """{name: labels (n,) from 1} — interleaved (no cluster is contiguous), one cluster, all singletons, planted groups of random
    sizes in random places, one of them with numbers that no row carries."""
    rng = np.random.default_rng(seed)
    out = {"one": np.ones(n, dtype=np.uint32), "singletons": np.arange(1, n + 1, dtype=np.uint32)}
    k = max(1, min(5, n))
    out["interleaved"] = (np.arange(n) % k + 1).astype(np.uint32)
    groups = max(1, n // 7)
    out["planted"] = (rng.integers(0, groups, size=n) + 1).astype(np.uint32)
    if n:
        out["planted"][rng.integers(0, n)] = groups                 # the largest number is carried
    return out


def planted_symbols(n, s, labels, seed, missing=0.1):
    """Rows that share their group's founder, a few private changes and up to `missing` of a row without a base: the groups own SNPs."""
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"ACGTACGTacgt", dtype=np.uint8)
    labels = np.asarray(labels, dtype=np.int64)
    root = alphabet[rng.integers(0, len(alphabet), size=s)]
    founders = np.tile(root, (int(labels.max()) + 1 if n else 1, 1))
    for g in range(len(founders)):
        at = rng.integers(0, s, size=max(1, s // 20)) if s else np.zeros(0, dtype=np.int64)
        founders[g, at] = alphabet[rng.integers(0, len(alphabet), size=len(at))]
    sym = founders[labels].copy() if n else np.zeros((0, s), dtype=np.uint8)
    for r in range(n):
        at = rng.integers(0, s, size=int(rng.integers(0, 4))) if s else np.zeros(0, dtype=np.int64)
        sym[r, at] = alphabet[rng.integers(0, len(alphabet), size=len(at))]
        gone = rng.integers(0, s, size=int(rng.integers(0, int(missing * s) + 1))) if s else np.zeros(0, dtype=np.int64)
        sym[r, gone] = np.frombuffer(b"-N", dtype=np.uint8)[rng.integers(0, 2, size=len(gone))]
    return np.ascontiguousarray(sym)
