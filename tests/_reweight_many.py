"""Shared by tests/test_reweight_many.py and tests/test_gpu_reweight_many.py: crafted visit rows on a config's geometry
and the designs the tests re-weight them for."""
import numpy as np

from tests import _visits as V


def crafted_rows(c, n_rows=37, seed=7, num_lmd=3):
    """``(counts uint32 [n_rows, C], ends [n_rows], deposits bool [n_rows])``, C the channel count of the case's geometry
    (70 on the default design): counts 70 % zeros and the rest 1 .. 3, row 0 all zero and row 1 (when there is one)
    holding a count of 40 (in channel 17, or the last one of a narrower table); ends drawn inside each row's FoV's
    range; about one row in six not delivered (flags 2 or 0) and about one in nine with a tile index at or beyond the
    scene's count."""
    rng = np.random.default_rng(seed)
    C = 6 + 4 * c.geom.num_fc_slices + 6 * c.geom.num_oc_slices
    counts = np.where(rng.random((n_rows, C)) < 0.7, 0, rng.integers(1, 4, (n_rows, C))).astype(np.uint32)
    counts[0] = 0
    if n_rows > 1:
        counts[1, min(17, C - 1)] = 40
    rg = c.geom.eff_reg_FOV_range
    n_tiles = num_lmd * c.nx * c.ny
    ends = np.zeros(n_rows, V.DTYPE)
    tile = rng.integers(0, n_tiles, n_rows)
    m, n = tile // c.ny % c.nx, tile % c.ny
    u, v = rng.uniform(0.02, 0.98, n_rows), rng.uniform(0.02, 0.98, n_rows)
    ends["x"] = rg[m, n, 0] + u * (rg[m, n, 1] - rg[m, n, 0])
    ends["y"] = rg[m, n, 2] + v * (rg[m, n, 3] - rg[m, n, 2])
    ends["gid"] = np.arange(n_rows)
    ends["flags"] = 3
    off = rng.random(n_rows) < 1 / 6
    off[:2] = False                                     # the all-zero row and the count of 40 deposit
    ends["flags"][off] = rng.choice([0, 2], int(off.sum()))
    bad = (rng.random(n_rows) < 1 / 9) & ~off
    bad[:2] = False
    tile[bad] = n_tiles + rng.integers(0, 5, int(bad.sum())) * (rng.random(int(bad.sum())) < 0.5) * 1000
    ends["tile"] = tile
    return counts, ends, ~(off | bad)


def designs(K, C, seed=3, spread=0.2):
    """float64 ``[K, C]`` log-scales: design 0 all zeros (the nominal design), the rest uniform in ``[-spread, spread]``."""
    ln = np.random.default_rng(seed).uniform(-spread, spread, (K, C))
    ln[0] = 0.0
    return ln
