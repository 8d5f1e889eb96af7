"""The statement of the compared-site counts (csrc/compared.hip), in plain NumPy: what the kernels, the library's host forms, the
writer and the command are compared with.  Nothing here shares code with the package.

Compared(i, j) is the number of columns at which both bytes are in ACGT after upper-casing a-z: the predicate of the distance
(utils.calculate_sequence_distance, utils.py:1135-1165) without "and differ"."""
import numpy as np

from tests.nearest_cases import random_symbols  # noqa: F401  (the symbols of the cases: alphabet ACGTACGTACGTacgt-N, or every byte)

HEADER = "Seq1\tSeq2\tDistance\tCompared\n"
BASES = b"ACGT"


def valid_sites(sym):
    """(n, s) uint8 -> (n, s) bool: the byte is one of ACGT after upper-casing a-z."""
    a = np.asarray(sym, dtype=np.uint8)
    upper = np.where((a >= 97) & (a <= 122), a - 32, a).astype(np.uint8)
    return np.isin(upper, np.frombuffer(BASES, dtype=np.uint8))


def compared_rect(q_sym, db_sym):
    """(q, s) and (n, s) uint8 -> (q, n) int32, site by site."""
    q_sym = np.asarray(q_sym, dtype=np.uint8)
    db_sym = np.asarray(db_sym, dtype=np.uint8)
    q, n = len(q_sym), len(db_sym)
    out = np.zeros((q, n), dtype=np.int32)
    if q == 0 or n == 0:
        return out
    assert q_sym.shape[1] == db_sym.shape[1]
    qv, dv = valid_sites(q_sym), valid_sites(db_sym)
    for i in range(q):
        out[i] = (dv & qv[i]).sum(axis=1)
    return out


def compared_pairs(sym_a, a, b, sym_b=None):
    """Compared(row a[p] of sym_a, row b[p] of sym_b) per pair; sym_b None: both index sym_a."""
    va = valid_sites(sym_a)
    vb = va if sym_b is None else valid_sites(sym_b)
    return np.asarray([int((va[int(i)] & vb[int(j)]).sum()) for i, j in zip(a, b)], dtype=np.int32).reshape(len(a))


def plane_words(s, slab=16):
    """Words of a row of the valid plane: one per 32 sites, padded to whole slabs."""
    return ((s + 31) // 32 + slab - 1) // slab * slab


def valid_plane(sym, slab=16):
    """(n, s) uint8 -> (n, plane_words(s)) uint32: bit i of word w = column 32 w + i is valid; the padding is zero."""
    v = valid_sites(sym)
    n, s = v.shape
    bits = np.zeros((n, plane_words(s, slab) * 32), dtype=np.uint8)
    bits[:, :s] = v
    return np.packbits(bits.reshape(n, -1, 4, 8), axis=3, bitorder="little").reshape(n, -1, 4).copy().view("<u4").reshape(n, -1)


def matrix_text(ids, mat):
    """The layout of the matrix file of distance.py:107-114."""
    out = ["\t" + "\t".join(ids) + "\n"] if len(ids) else ["\t\n"]
    for i, name in enumerate(ids):
        out.append(name + "".join("\t%i" % int(x) for x in mat[i]) + "\n")
    return "".join(out)


def pair_rows_text(a_ids, b_ids, a, b, dist, compared):
    """The file of pair lists: the header, then "id of a, id of b, distance, compared" per row in the order given."""
    return HEADER + "".join("%s\t%s\t%i\t%i\n" % (a_ids[int(i)], b_ids[int(j)], int(d), int(c)) for i, j, d, c in zip(a, b, dist, compared))


def with_fourth_column(text, compared):
    """A three-column file with one more column: the header gains Compared, row r gains compared[r]."""
    lines = text.split("\n")
    assert lines[-1] == "" and lines[0] == "Seq1\tSeq2\tDistance" and len(lines) - 2 == len(compared)
    return HEADER + "".join("%s\t%i\n" % (line, int(c)) for line, c in zip(lines[1:-1], compared))


def sorted_rows_of_records(records):
    """[(id, bytes)] in file order -> (sorted ids, (n, s) uint8): equal ids keep their last record, shorter rows are padded with '-'
    (the rule of the distance step)."""
    last = {}
    for name, row in records:
        last[name] = bytes(row)
    ids = sorted(last)
    s = max([len(last[i]) for i in ids] or [0])
    sym = np.full((len(ids), s), 0x2D, dtype=np.uint8)
    for r, i in enumerate(ids):
        sym[r, :len(last[i])] = np.frombuffer(last[i], dtype=np.uint8)
    return ids, sym
