"""What the differing-sites outputs of the distance step must be, stated in NumPy and plain Python: the GPU tests compare the
kernel of csrc/pair_sites.hip and the files of the commands against these; tests/test_pair_sites_cpu.py pins the statements
themselves on the reference's own tables."""
import numpy as np

HEADER_SITE = "Seq1\tSeq2\tSite\tBase1\tBase2\n"
HEADER_POS = "Seq1\tSeq2\tChrom\tPos\tBase1\tBase2\n"
LETTERS = "ACGTacgt"


def upper(x):
    x = np.asarray(x, dtype=np.uint8)
    return np.where((x >= 97) & (x <= 122), x - 32, x).astype(np.uint8)


def differs(x, y):
    """utils.calculate_sequence_distance (utils.py:1135-1165) column by column: both bytes, upper-cased, in ACGT and unequal."""
    ux, uy = upper(x), upper(y)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    return np.isin(ux, acgt) & np.isin(uy, acgt) & (ux != uy)


def nibble(x):
    """bits 0-1: A0 C1 G2 T3, bit 2: lower case — of bytes that are letters of ACGTacgt."""
    x = np.asarray(x, dtype=np.uint8)
    code = np.searchsorted(np.frombuffer(b"ACGT", dtype=np.uint8), upper(x)).astype(np.uint8)
    return code | ((x >= 97).astype(np.uint8) << 2)


def pair_sites(sym, a, b):
    """(pair_off uint64 [m + 1], site uint32, bases uint8) of the pairs (a[p], b[p]) of rows of the byte matrix."""
    sym = np.asarray(sym, dtype=np.uint8)
    off = np.zeros(len(a) + 1, dtype=np.uint64)
    sites, bases = [np.zeros(0, dtype=np.uint32)], [np.zeros(0, dtype=np.uint8)]
    for p, (i, j) in enumerate(zip(a, b)):
        at = np.flatnonzero(differs(sym[i], sym[j])) if i != j else np.zeros(0, dtype=np.int64)
        off[p + 1] = off[p] + np.uint64(len(at))
        sites.append(at.astype(np.uint32))
        bases.append(nibble(sym[i][at]) | (nibble(sym[j][at]) << 4))
    return off, np.concatenate(sites), np.concatenate(bases).astype(np.uint8)


def counts(sym):
    """The matrix the distance step computes, from the predicate (n small)."""
    sym = np.asarray(sym, dtype=np.uint8)
    n = len(sym)
    return np.asarray([[int(differs(sym[i], sym[j]).sum()) for j in range(n)] for i in range(n)], dtype=np.int64).reshape(n, n)


def pairs_of_csr(row_off, col, dist, threshold):
    """The entries i < j, d <= T of a CSR, in its order."""
    a, b, d = [], [], []
    for i in range(len(row_off) - 1):
        for e in range(int(row_off[i]), int(row_off[i + 1])):
            if i < col[e] and dist[e] <= threshold:
                a.append(i)
                b.append(int(col[e]))
                d.append(int(dist[e]))
    return np.asarray(a, dtype=np.uint32), np.asarray(b, dtype=np.uint32), np.asarray(d, dtype=np.int32)


def close_pairs(mat, threshold):
    """The pairs i < j with d <= T in the pairwise file's order."""
    n = len(mat)
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n) if mat[i][j] <= threshold]
    return np.asarray([p[0] for p in pairs], dtype=np.uint32), np.asarray([p[1] for p in pairs], dtype=np.uint32)


def text(ids, a, b, pair_off, site, bases, snp_list=None):
    tails = ["\t%s\t%s\n" % (LETTERS[x & 7], LETTERS[(x >> 4) & 7]) for x in range(256)]
    site, bases = np.asarray(site).tolist(), np.asarray(bases).tolist()
    where = {}
    out = [HEADER_SITE if snp_list is None else HEADER_POS]
    for p in range(len(a)):
        lo, hi = int(pair_off[p]), int(pair_off[p + 1])
        for s in site[lo:hi]:
            if s not in where:
                where[s] = "%d" % (s + 1) if snp_list is None else "%s\t%d" % snp_list[s]
        head = "%s\t%s\t" % (ids[a[p]], ids[b[p]])
        out.extend([head + where[s] + tails[x] for s, x in zip(site[lo:hi], bases[lo:hi])])
    return "".join(out)


def text_of_rows(ids, sym, a, b, snp_list=None):
    """The file, straight from the bytes: a row per differing column with the two bytes as they are."""
    out = [HEADER_SITE if snp_list is None else HEADER_POS]
    for i, j in zip(a, b):
        if i == j:
            continue
        for s in np.flatnonzero(differs(sym[i], sym[j])):
            where = "%d" % (s + 1) if snp_list is None else "%s\t%d" % snp_list[s]
            out.append("%s\t%s\t%s\t%s\t%s\n" % (ids[i], ids[j], where, chr(sym[i][s]), chr(sym[j][s])))
    return "".join(out)


def read_fasta(path):
    """(sorted ids, byte matrix padded with '-') of a snpma.fasta with rows of non-decreasing length in sorted-id order."""
    seqs, name = {}, None
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line.startswith(">"):
                name = line[1:].split()[0]
                seqs[name] = []
            elif name is not None:
                seqs[name].append(line)
    return rows_of_seqs({k: "".join(v) for k, v in seqs.items()})


def rows_of_seqs(seqs):
    ids = sorted(seqs)
    width = max([len(seqs[i]) for i in ids] + [0])
    sym = np.full((len(ids), width), 0x2D, dtype=np.uint8)
    for r, i in enumerate(ids):
        sym[r, :len(seqs[i])] = np.frombuffer(seqs[i].encode("latin-1"), dtype=np.uint8)
    return ids, sym


def read_snp_list(path):
    with open(path) as f:
        return [(ln.split()[0], int(ln.split()[1])) for ln in f if ln.strip()]


def planted(n, s, groups, seed, spread=3):
    """n rows of s sites over ACGTacgtN-: `groups` founders, every row a founder with a few changed sites, so that some distances are small."""
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"ACGTACGTACGTacgtN-", dtype=np.uint8)
    founders = alphabet[rng.integers(0, len(alphabet), size=(groups, s))]
    sym = founders[rng.integers(0, groups, size=n)].copy()
    for r in range(n):
        k = int(rng.integers(0, spread + 1))
        at = rng.integers(0, s, size=k)
        sym[r, at] = alphabet[rng.integers(0, len(alphabet), size=k)]
    return np.ascontiguousarray(sym)
