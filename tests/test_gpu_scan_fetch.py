"""The scan's tile stream at its seams: a site line starts a few bytes before every 4 KiB tile end, so that its name and position
are read from the halo the tile's last DMA instruction fetches (the bytes the next tile's first instruction reads again).  The
distances here are drawn at random; tests/test_gpu_scan_parse.py (case F) sweeps every distance from 0 to 72 bytes deterministically."""
import random

import pytest

from oracle import fuzz
from oracle import pileup_oracle as po

pytestmark = pytest.mark.gpu

TILE = 4096


@pytest.fixture(scope="module")
def d():
    from tests.gpu_util import get_device
    return get_device()


def _lines_at_tile_ends(seed, eol, switch_contig):
    """Pileup lines (short: 12x) whose positions are zero padded where that makes the next line start 1..40 bytes before a tile
    end.  switch_contig: the line at the seam is taken from the other contig (the wave's contig hint changes there).  Returns the
    file and the (contig, pos) keys of the lines at the seams."""
    contigs = ("seam_chr1", "chr2")
    data, _, _ = fuzz.synth_pileup(seed, genome_len=6000, contigs=contigs, mean_depth=12, n_sites=10)
    by_contig = {c.encode(): [] for c in contigs}
    for ln in data.split(b"\n")[:-1]:
        by_contig[ln.split(b"\t", 1)[0]].append(ln.split(b"\t"))
    src = [by_contig[c.encode()] for c in contigs]
    rng = random.Random(seed)
    out, off, cur, seam_keys = [], 0, 0, []
    next_is_seam = False
    while src[cur]:
        f = src[cur].pop(0)
        if next_is_seam:
            seam_keys.append((f[0], int(f[1])))
            next_is_seam = False
        j = rng.randint(1, 40)                                   # bytes of the next line before the tile end
        b = (off // TILE + 1) * TILE
        end = off + len(b"\t".join(f)) + len(eol)
        if 0 <= b - j - end < 48:
            f = [f[0], b"0" * (b - j - end) + f[1]] + f[2:]
            next_is_seam = True
            if switch_contig and src[1 - cur]:
                cur = 1 - cur
        line = b"\t".join(f) + eol
        out.append(line)
        off += len(line)
        if not src[cur] and src[1 - cur]:
            cur = 1 - cur
    return b"".join(out), seam_keys


@pytest.mark.parametrize("eol", [b"\n", b"\r\n"])
@pytest.mark.parametrize("switch_contig", [False, True])
def test_site_lines_that_start_just_before_every_tile_end(d, eol, switch_contig):
    from tests.gpu_util import check_against_oracle
    data, seam_keys = _lines_at_tile_ends(3 + len(eol), eol, switch_contig)
    n_tiles = len(data) // TILE
    assert n_tiles >= 40 and len(seam_keys) >= n_tiles * 3 // 4   # most tile ends have a line that needs the halo
    snps = sorted(set(seam_keys))
    check_against_oracle(d, data, snps, snps[::5], po.CallerParams(0, 0.6, 3, 0, 0.0))
