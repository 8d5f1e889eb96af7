"""What ``distance`` costs on the device for every combination of its outputs: symbol uploads and matrix computations, counted
by a recording stand-in for ``Device`` that answers from the restatements of tests/*_cases.py.  The command decides these costs in
one plan (``distance.distance_plan``); the table below was recorded with this same file against the last version of distance.py
that decided them in two parallel bodies (profiles/r28/distance_host_forms.md), and the plan has to reproduce it exactly.  No GPU."""
import os

import numpy as np
import pytest

from tests import clusters_cases as cc
from tests import cluster_snps_cases as sc
from tests import compared_cases as pc
from tests import linkage_cases as lc
from tests import mst_cases as mc
from tests import nearest_cases as nc
from tests import nj_cases as jc
from tests import pair_sites_cases as ps


class RecordingDevice(object):
    """The public host forms the command calls.  A host form that takes symbols is one upload (two matrices: two); ``*_of_matrix``,
    ``*_kept`` and ``clusters`` upload no symbols.  ``distance``, ``close_pairs``, ``mst``, ``distance_outputs``, ``linkage`` and
    ``nj`` each compute the matrix once."""

    def __init__(self):
        self.uploads = self.computations = self.keeps = self.drops = 0
        self.kept = None

    def _matrix(self, sym, uploads=1):
        self.uploads += uploads
        self.computations += 1
        sym = np.asarray(sym, dtype=np.uint8)
        return nc.rect_distance(sym, sym) if sym.shape[1] else np.zeros((len(sym), len(sym)), dtype=np.int32)

    @staticmethod
    def _tree(mat):
        return mc.arrays(mc.mst_of_matrix(mat) if len(mat) > 1 else [])

    def distance(self, symbols):
        return self._matrix(symbols)

    def distance_outputs(self, symbols, want_tree=False, want_matrix=False, pairs_within=None, keep_packed=False, capacity=None):
        mat = self._matrix(symbols)
        if keep_packed:
            self.keeps += 1
            self.kept = np.asarray(symbols, dtype=np.uint8)
        return (self._tree(mat) if want_tree else None), (cc.filter_rows(mat, pairs_within) if pairs_within is not None else None), (mat if want_matrix else None)

    def close_pairs(self, symbols, threshold, capacity=None, want_matrix=False):
        mat = self._matrix(symbols)
        return cc.filter_rows(mat, threshold) + ((mat,) if want_matrix else ())

    def mst(self, symbols, want_matrix=False, pairs_within=None):
        mat = self._matrix(symbols)
        return self._tree(mat) + ((cc.filter_rows(mat, pairs_within),) if pairs_within is not None else ()) + ((mat,) if want_matrix else ())

    def linkage_of_matrix(self, matrix, kind, want_rounds=False):
        return lc.arrays(lc.rounds(matrix, kind)[0] if len(matrix) > 1 else [])

    def linkage(self, symbols, kind, want_matrix=False, want_rounds=False):
        return self.linkage_of_matrix(self._matrix(symbols), kind)

    def nj_of_matrix(self, matrix):
        return jc.arrays(jc.nj(matrix))

    def nj(self, symbols, want_matrix=False):
        return self.nj_of_matrix(self._matrix(symbols))

    def pair_sites(self, symbols, a, b, expect=None):
        self.uploads += 1
        return ps.pair_sites(symbols, a, b)

    def pair_sites_kept(self, a, b, expect=None):
        assert self.kept is not None, "no packed matrix was kept"
        return ps.pair_sites(self.kept, a, b)

    def packed_drop(self):
        self.drops += 1
        self.kept = None

    def clusters(self, n, row_off, col, dist, thresholds):
        numbers = np.asarray([cc.numbers_of_labels(cc.labels_of_reach(cc.reach(cc.adjacency(n, row_off, col, dist, t)))) for t in thresholds], dtype=np.uint32)
        return numbers.reshape(len(thresholds), n), np.asarray([int(r.max()) if n else 0 for r in numbers], dtype=np.uint32)

    def compared(self, symbols):
        self.uploads += 1
        return pc.compared_rect(symbols, symbols)

    def compared_pairs(self, symbols_a, a, b, symbols_b=None):
        self.uploads += 1 if symbols_b is None else 2
        return pc.compared_pairs(symbols_a, a, b, symbols_b)

    def site_counts(self, symbols):
        self.uploads += 1
        return sc.site_counts(symbols)

    def cluster_snps(self, symbols, labels, n_clusters=None, expect=None):
        self.uploads += 1
        labels = np.asarray(labels).reshape(-1, len(symbols))
        got = [sc.cluster_snps(symbols, row, None if n_clusters is None else n_clusters[t]) for t, row in enumerate(labels)]
        first = np.cumsum([0] + [len(g[1]) for g in got]).astype(np.uint64)
        return ([g[0] + first[t] for t, g in enumerate(got)],) + tuple(np.concatenate([g[k] for g in got]) if got else np.zeros(0, dtype=np.uint32) for k in (1, 2, 3))

    def nearest(self, q_symbols, db_symbols, k=0, threshold=None, band_rows=0, route=0, want_matrix=False):
        self.uploads += 2
        return nc.nearest_of_matrix(nc.rect_distance(q_symbols, db_symbols), k, threshold)


def planted_records():
    """6 samples x 40 columns: two groups of three a few sites apart, the groups far apart; some '-' and lower-case bytes; the
    records of the file are not in the order of their ids."""
    rng = np.random.default_rng(28)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    centres = [rng.integers(0, 4, size=40), None]
    centres[1] = (centres[0] + np.where(np.arange(40) % 2 == 0, 1, 0)) & 3                   # 20 sites from the first
    rows = []
    for r in range(6):
        code = centres[r // 3].copy()
        at = rng.choice(40, size=r % 3, replace=False)
        code[at] = (code[at] + 1) & 3
        rows.append(acgt[code].copy())
    rows[1][7] = rows[4][7] = rows[4][30] = 0x2D
    rows[2][3:6] += 32
    rows[5][38] += 32
    ids = ["s3", "s0", "s5", "s1", "s4", "s2"]
    assert ids != sorted(ids)
    return list(zip(ids, (bytes(r).decode("ascii") for r in rows)))


INPUTS = ("planted", "no record", "no column")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """Per input: the multi-FASTA, a query file, a pair list and a snplist that fit it."""
    out = {}
    for name in INPUTS:
        d = tmp_path_factory.mktemp(name.replace(" ", "_"))
        records = planted_records() if name == "planted" else [] if name == "no record" else [(i, "") for i in ("b", "c", "a")]
        columns = len(records[0][1]) if records else 0
        (d / "snpma.fasta").write_text("".join(">%s\n%s\n" % r for r in records))
        (d / "query.fasta").write_text("".join(">q%d\n%s\n" % (k, r[1].replace("A", "C", 2)) for k, r in enumerate(records[:2])))
        (d / "pairs.tsv").write_text("Seq1\tSeq2\n" + ("s4\ts0\ns2\ts5\ns1\ts1\n" if name == "planted" else "b\ta\n" if records else ""))
        (d / "snplist.txt").write_text("".join("chr%d\t%d\t2\tx\ty\n" % (1 + k // 25, 10 + 3 * k) for k in range(columns)))
        out[name] = d
    return out


T = "--amdClusterThresholds 1 3 25"
P = "-p {o}/p -m {o}/m"
CLOSE, CLUSTERS, MST, DENDRO = "--amdClosePairs {o}/close --amdMaxPairDistance 3", "--amdClusters {o}/clusters " + T, "--amdMst {o}/mst", "--amdDendrogram {o}/dendro"
LINKAGE, NJ = "--amdLinkage average --amdLinkageMerges {o}/merges --amdLinkageClusters {o}/lclusters " + T, "--amdNj {o}/nj"
NEAREST, COUNTS, CMATRIX = "--amdQuery {i}/query.fasta --amdNearest {o}/nearest --amdNearestCount 2", "--amdSiteCounts {o}/counts", "--amdComparedMatrix {o}/cmatrix"
CSNPS = "--amdClusterSnps {o}/csnps " + T
CLOSE_SITES, MST_SITES = "--amdClosePairSites {o}/csites --amdMaxPairDistance 3", "--amdMstSites {o}/msites"
USER_SITES = "--amdPairSitesPairs {i}/pairs.tsv --amdPairSitesOut {o}/usites"
ALONE = (("close", CLOSE), ("clusters", CLUSTERS), ("mst", MST), ("dendrogram", DENDRO), ("linkage", LINKAGE), ("nj", NJ), ("nearest", NEAREST), ("site counts", COUNTS),
         ("compared matrix", CMATRIX), ("cluster snps", CSNPS))
SITES = (("close sites", CLOSE_SITES), ("mst sites", MST_SITES), ("user sites", USER_SITES))
EVERYTHING = " ".join((P, CLOSE, "--amdClusters {o}/clusters", MST, DENDRO, LINKAGE, NJ, CSNPS.replace(T, ""), "--amdCompared"))
COMBINATIONS = dict(
    [("-p", "-p {o}/p"), ("-m", "-m {o}/m"), ("-p -m", P)] + list(ALONE) + [(name + " -p -m", text + " " + P) for name, text in ALONE]
    + [("tree close clusters", " ".join((MST, DENDRO, CLOSE, "--amdClusters {o}/clusters " + T)))]
    + list(SITES) + [(name + " everything", " ".join((text, EVERYTHING, "--amdSnpList {i}/snplist.txt"))) for name, text in SITES]
    + [("all sites", " ".join(text for _, text in SITES)), ("all sites -p -m", " ".join([text for _, text in SITES] + [P]))]
    + [("linkage mst", LINKAGE + " " + MST), ("nj mst", NJ + " " + MST), ("linkage nj", LINKAGE + " " + NJ), ("linkage nj user sites", " ".join((LINKAGE, NJ, USER_SITES)))]
    + [("compared close", CLOSE + " --amdCompared"), ("compared mst", MST + " --amdCompared"), ("compared nearest", NEAREST + " --amdCompared"),
       ("compared close mst nearest", " ".join((CLOSE, MST, NEAREST, "--amdCompared")))]
    + [("cluster snps close sites", CSNPS + " " + CLOSE_SITES), ("cluster snps snplist", CSNPS + " --amdSnpList {i}/snplist.txt")])

# (symbol uploads, matrix computations) per combination and input of INPUTS, recorded against the two-bodied distance.py (see the docstring)
EXPECTED = {
    '-m': ((1, 1), (0, 0), (0, 0)),
    '-p': ((1, 1), (0, 0), (0, 0)),
    '-p -m': ((1, 1), (0, 0), (0, 0)),
    'all sites': ((1, 1), (0, 0), (1, 1)),
    'all sites -p -m': ((1, 1), (0, 0), (1, 1)),
    'close': ((1, 1), (0, 0), (1, 1)),
    'close -p -m': ((1, 1), (0, 0), (1, 1)),
    'close sites': ((1, 1), (0, 0), (1, 1)),
    'close sites everything': ((3, 1), (0, 0), (2, 1)),
    'cluster snps': ((2, 1), (0, 0), (1, 1)),
    'cluster snps -p -m': ((2, 1), (0, 0), (1, 1)),
    'cluster snps close sites': ((2, 1), (0, 0), (1, 1)),
    'cluster snps snplist': ((2, 1), (0, 0), (1, 1)),
    'clusters': ((1, 1), (0, 0), (1, 1)),
    'clusters -p -m': ((1, 1), (0, 0), (1, 1)),
    'compared close': ((2, 1), (0, 0), (2, 1)),
    'compared close mst nearest': ((6, 1), (1, 1), (6, 1)),
    'compared matrix': ((1, 0), (0, 0), (0, 0)),
    'compared matrix -p -m': ((2, 1), (0, 0), (0, 0)),
    'compared mst': ((2, 1), (1, 1), (2, 1)),
    'compared nearest': ((4, 0), (0, 0), (4, 0)),
    'dendrogram': ((1, 1), (1, 1), (1, 1)),
    'dendrogram -p -m': ((1, 1), (1, 1), (1, 1)),
    'linkage': ((1, 1), (1, 1), (1, 1)),
    'linkage -p -m': ((1, 1), (0, 0), (0, 0)),
    'linkage mst': ((2, 2), (2, 2), (2, 2)),
    'linkage nj': ((2, 2), (2, 2), (2, 2)),
    'linkage nj user sites': ((3, 2), (0, 0), (3, 2)),
    'mst': ((1, 1), (1, 1), (1, 1)),
    'mst -p -m': ((1, 1), (1, 1), (1, 1)),
    'mst sites': ((1, 1), (0, 0), (1, 1)),
    'mst sites everything': ((3, 1), (0, 0), (2, 1)),
    'nearest': ((2, 0), (0, 0), (2, 0)),
    'nearest -p -m': ((3, 1), (0, 0), (2, 0)),
    'nj': ((1, 1), (1, 1), (1, 1)),
    'nj -p -m': ((1, 1), (0, 0), (0, 0)),
    'nj mst': ((2, 2), (2, 2), (2, 2)),
    'site counts': ((1, 0), (0, 0), (0, 0)),
    'site counts -p -m': ((2, 1), (0, 0), (0, 0)),
    'tree close clusters': ((1, 1), (1, 1), (1, 1)),
    'user sites': ((1, 0), (0, 0), (1, 0)),
    'user sites everything': ((3, 1), (0, 0), (2, 1)),
}


def run(module, text, in_dir, out_dir, monkeypatch):
    """One run of the command: (uploads, computations, keeps, drops, output files asked for)."""
    from snp_pipeline_amd import cfsan_snp_pipeline as cli
    from snp_pipeline_amd import device
    dev = RecordingDevice()
    monkeypatch.setattr(device, "default_device", lambda: dev)
    argv = ("distance -f {i}/snpma.fasta " + text).format(i=in_dir, o=out_dir).split()
    module.calculate_snp_distances(cli.parse_argument_list(argv))
    assert dev.kept is None
    return dev.uploads, dev.computations, dev.keeps, dev.drops, [a for a in argv if a.startswith(str(out_dir))]


def record(module, inputs, out_root, monkeypatch):
    """{combination: per input (uploads, computations)}, every other statement of the test checked on the way."""
    table = {}
    for k, (name, text) in enumerate(sorted(COMBINATIONS.items())):
        row = []
        for which in INPUTS:
            out_dir = os.path.join(str(out_root), "%d_%s" % (k, which.replace(" ", "_")))
            os.makedirs(out_dir)
            uploads, computations, keeps, drops, files = run(module, text, inputs[which], out_dir, monkeypatch)
            assert keeps <= 1 and drops == keeps, (name, which, keeps, drops)    # dropped iff something was kept
            assert files and all(os.path.isfile(f) for f in files), (name, which)
            row.append((uploads, computations))
        table[name] = tuple(row)
    return table


def test_every_combination_costs_what_it_cost_before(inputs, tmp_path, monkeypatch):
    from snp_pipeline_amd import distance
    got = record(distance, inputs, tmp_path, monkeypatch)
    assert sorted(got) == sorted(EXPECTED)
    assert {k: v for k, v in got.items() if v != EXPECTED[k]} == {}


def test_the_plan_needs_no_device():
    from snp_pipeline_amd import distance
    o = distance.DistanceOptions()
    for name in ("pairwise_file", "matrix_file", "close_file", "clusters_file", "mst_file", "dendrogram_file", "close_sites_file", "mst_sites_file", "user_sites_file",
                 "cluster_snps_file", "max_pair_distance"):
        setattr(o, name, None)
    o.thresholds = [5, 2]
    o.clusters_file, o.close_sites_file, o.max_pair_distance = "c", "s", 9
    plan = distance.distance_plan(o, 6, 40)
    assert (plan.want_tree, plan.want_matrix, plan.widest, plan.compute, plan.keep_packed, plan.host_matrix) == (False, False, 9, True, True, False)
    o.close_sites_file, o.pairwise_file = None, "p"
    plan = distance.distance_plan(o, 6, 40)
    assert (plan.want_tree, plan.want_matrix, plan.widest, plan.compute, plan.keep_packed, plan.host_matrix) == (False, True, 5, True, False, True)
