"""The statement of the query-against-database nearest neighbours (csrc/nearest.hip), in plain NumPy: what the kernels, the
library's host form and the command are compared with.  Nothing here shares code with the package."""
import numpy as np

HEADER = "Seq1\tSeq2\tDistance\n"
INT_MAX = 2 ** 31 - 1
BASES = b"ACGT"


def rect_distance(q_sym, db_sym):
    """(q, s) and (n, s) uint8 -> (q, n) int32, site by site: a site counts for a pair iff, after upper-casing a-z, both bytes
    are in ACGT and differ (utils.calculate_sequence_distance, utils.py:1135-1165)."""
    q_sym = np.asarray(q_sym, dtype=np.uint8)
    db_sym = np.asarray(db_sym, dtype=np.uint8)
    q, n = len(q_sym), len(db_sym)
    out = np.zeros((q, n), dtype=np.int32)
    if q == 0 or n == 0:
        return out
    assert q_sym.shape[1] == db_sym.shape[1]

    def upper(a):
        return np.where((a >= 97) & (a <= 122), a - 32, a).astype(np.uint8)

    qu, du = upper(q_sym), upper(db_sym)
    qv, dv = np.isin(qu, np.frombuffer(BASES, dtype=np.uint8)), np.isin(du, np.frombuffer(BASES, dtype=np.uint8))
    for i in range(q):
        out[i] = ((du != qu[i]) & dv & qv[i]).sum(axis=1)
    return out


def nearest_of_matrix(mat, k=0, t=None):
    """(q, n) signed matrix -> (row_off uint64 [q + 1], col uint32, dist int32): per row the entries <= t (None: all) ordered by
    (d, column), the first k of them (0: all)."""
    mat = np.asarray(mat)
    q = mat.shape[0]
    n = mat.shape[1] if mat.ndim == 2 else 0
    row_off, col, dist = [0], [], []
    for i in range(q):
        keep = [(int(mat[i, j]), j) for j in range(n) if t is None or int(mat[i, j]) <= t]
        keep.sort()
        if k:
            keep = keep[:k]
        col.extend(j for _, j in keep)
        dist.extend(d for d, _ in keep)
        row_off.append(len(col))
    return np.asarray(row_off, dtype=np.uint64), np.asarray(col, dtype=np.uint32), np.asarray(dist, dtype=np.int32)


def nearest_text(q_ids, db_ids, csr):
    """The file: the header, then "query id, database id, distance" per entry, query by query."""
    row_off, col, dist = csr
    out = [HEADER]
    for i, name in enumerate(q_ids):
        for e in range(int(row_off[i]), int(row_off[i + 1])):
            out.append("%s\t%s\t%i\n" % (name, db_ids[int(col[e])], int(dist[e])))
    return "".join(out)


def ties_across_the_cut(mat, k):
    """How many rows have a tie between their k-th and (k + 1)-th smallest entry: the rows whose answer the tie rule decides."""
    s = np.sort(np.asarray(mat), axis=1)
    return int((s[:, k - 1] == s[:, k]).sum()) if 0 < k < s.shape[1] else 0


def random_symbols(rows, sites, seed, every_byte=False):
    """Sequence bytes with lower case, '-' and 'N' among the bases; every_byte: all 256 byte values instead."""
    rng = np.random.default_rng(seed)
    if every_byte:
        return rng.integers(0, 256, size=(rows, sites), dtype=np.uint8)
    alphabet = np.frombuffer(b"ACGTACGTACGTacgt-N", dtype=np.uint8)
    return alphabet[rng.integers(0, len(alphabet), size=(rows, sites))]


def read_fasta_rows(path):
    """(sorted ids, (n, s) uint8 matrix) of a multi-FASTA whose sequences are equally long; equal ids keep their last record."""
    seqs, cur = {}, None
    with open(path) as f:
        for line in f.read().splitlines():
            if line.startswith(">"):
                cur = line[1:]
                seqs[cur] = ""
            elif cur is not None:
                seqs[cur] += line
    ids = sorted(seqs)
    if not ids:
        return ids, np.zeros((0, 0), dtype=np.uint8)
    return ids, np.asarray([np.frombuffer(seqs[i].encode("latin-1"), dtype=np.uint8) for i in ids], dtype=np.uint8)
