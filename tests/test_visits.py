"""Branch visit counts without a GPU: the channel table in its three statements (the library's, the Python layer's, the
checker's), ``luts.scale_channel``, the host twins of the two reductions against their numpy restatement, the driver's
argument handling, and the identity the feature rests on -- a delivered ray's probability is ``prod e_taken``, so the
same rays re-weighted by ``s^N_c`` are the scaled design's -- checked statistically on the checker alone."""
import numpy as np
import pytest

from gpu_ray_tracing_for_waveguide_based_ar_display_amd import gpu_ray_tracing_pro_fullColor as drv
from gpu_ray_tracing_for_waveguide_based_ar_display_amd import luts as LUTS
from gpu_ray_tracing_for_waveguide_based_ar_display_amd._lib import load
from gpu_ray_tracing_for_waveguide_based_ar_display_amd.AR_system_evaluation_functions import pupil_mask
from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import (VISIT_END_DTYPE, visit_channels,
                                                                       visits_reweight_host, visits_sensitivity_host)
from tests import _visits as V

STATES = {"ic": 9, "r0": 0, "r1": 1, "r2": 2, "r3": 3, "r4": 4, "r5": 5}


# 1. the channel table ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nfc", [1, 7])
@pytest.mark.parametrize("noc", [1, 6])
def test_channel_table_in_c_python_and_the_checker(nfc, noc):
    L = load()
    names = visit_channels((nfc, noc))
    C = 6 + 4 * nfc + 6 * noc
    assert len(names) == len(set(names)) == C == L.wgrt_visit_channel_count_host(nfc, noc) == V.n_channels(nfc, noc)
    seen = []
    for c, name in enumerate(names):
        lut, sl, quad = LUTS.channel_quad(name)
        state, b = STATES[name.split(".")[0].split("[")[0]], int(name[-1]) - 1
        assert L.wgrt_visit_channel_host(nfc, noc, state, 0 if sl is None else sl, b) == c, name
        assert V.channel(nfc, noc, state, 0 if sl is None else sl, b) == c, name
        seen.append((lut, sl, quad))
    assert len(set(seen)) == C                               # every channel is its own quadruple of its own LUT (slice)
    B = 6 + 4 * nfc
    assert names[:6] == ["ic.b1", "ic.b2", "r0.b1", "r0.b2", "r1.b1", "r1.b2"]
    assert names[6:10] == ["r2[0].b1", "r2[0].b2", "r3[0].b1", "r3[0].b2"]
    assert names[B:B + 6] == ["r4[0].b1", "r4[0].b2", "r4[0].b3", "r5[0].b1", "r5[0].b2", "r5[0].b3"]
    # what names no channel, in both C statements
    for state, sl, b in ((9, 0, 2), (0, 0, 2), (2, nfc, 0), (3, 0, 2), (4, noc, 0), (5, 0, 3), (6, 0, 0), (4, -1, 0), (4, 0, -1)):
        assert L.wgrt_visit_channel_host(nfc, noc, state, sl, b) == -1 == V.channel(nfc, noc, state, sl, b)


def test_the_design_geometry_has_70_channels():
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.couplers_coor import design_geometry
    g = design_geometry(5, 4)
    assert (g.num_fc_slices, g.num_oc_slices) == (7, 6)
    assert len(visit_channels((g.num_fc_slices, g.num_oc_slices))) == 70


def test_the_table_is_the_issue_s():
    quads = {"ic.b1": ("lut_ic1", (13, 18, 33, 38)), "ic.b2": ("lut_ic1", (15, 20, 35, 40)),
             "r0.b1": ("lut_ic2", (4, 9, 24, 29)), "r0.b2": ("lut_ic2", (6, 11, 26, 31)),
             "r1.b1": ("lut_ic3", (2, 22, 7, 27)), "r1.b2": ("lut_ic3", (4, 9, 24, 29)),
             "r2[3].b1": ("lut_fc1", (3, 6, 15, 18)), "r2[3].b2": ("lut_fc1", (2, 5, 14, 17)),
             "r3[3].b1": ("lut_fc2", (4, 7, 16, 19)), "r3[3].b2": ("lut_fc2", (3, 6, 15, 18)),
             "r4[2].b1": ("lut_oc1", (4, 9, 24, 29)), "r4[2].b2": ("lut_oc1", (2, 7, 22, 27)),
             "r4[2].b3": ("lut_oc1", (13, 18, 33, 38)), "r5[2].b1": ("lut_oc2", (6, 11, 26, 31)),
             "r5[2].b2": ("lut_oc2", (4, 9, 24, 29)), "r5[2].b3": ("lut_oc2", (15, 20, 35, 40))}
    for name, (lut, quad) in quads.items():
        got = LUTS.channel_quad(name)
        assert (got[0], got[2]) == (lut, quad), name
    for bad in ("ic.b3", "r0[1].b1", "r2.b1", "r2[0].b3", "r6[0].b1", "r4[0]", "ic"):
        with pytest.raises(ValueError):
            LUTS.channel_quad(bad)


# 2. scale_channel ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name, lmd", [("ic.b2", None), ("r1.b1", 2), ("r2[1].b2", None), ("r3[0].b1", 0),
                                       ("r4[2].b3", None), ("r5[1].b2", 1)])
def test_scale_channel_touches_exactly_its_quadruple(name, lmd):
    c = V.config(3, 2, [0, 1, 2], 4)
    before = {k: v.copy() for k, v in c.luts.items()}
    got = LUTS.scale_channel(c.luts, name, 1.44, lmd=lmd)
    lut, sl, quad = LUTS.channel_quad(name)
    for k in before:                                          # the input is untouched, the other LUTs are shared
        np.testing.assert_array_equal(c.luts[k], before[k])
        if k != lut:
            assert got[k] is c.luts[k]
    want = before[lut].copy()
    tiles = want if sl is None else want[sl]
    tiles = tiles if lmd is None else tiles[lmd]
    tiles[..., list(quad)] *= np.sqrt(1.44)
    np.testing.assert_array_equal(got[lut], want)
    changed = got[lut] != before[lut]
    n_tiles = (3 if lmd is None else 1) * 3 * 2
    assert changed.sum() == 4 * n_tiles                       # (no coefficient of the synthetic LUTs is zero)
    with pytest.raises(ValueError):
        LUTS.scale_channel(c.luts, name, 0.0)
    with pytest.raises(ValueError):
        LUTS.scale_channel(c.luts, "r4[6].b3", 1.1)
    with pytest.raises(ValueError):
        LUTS.scale_channel(c.luts, name, 1.1, lmd=3)


# 3. the host twins ---------------------------------------------------------------------------------------------------

def _rows(c, launches=1):
    from oracle import OracleScene
    sc = OracleScene.from_geometry(c.geom, c.luts)
    return V.checker(sc, c.rays, c.fresh_rng(), launches)


def test_host_twins_equal_the_numpy_restatement():
    c = V.config(5, 4, [0, 1, 2], 100)
    counts, ends, _, _, fates = _rows(c)
    counts, ends = counts[0], ends[0]
    assert ends.dtype == VISIT_END_DTYPE
    delivered = (ends["flags"] & 1) != 0
    assert delivered.sum() == (fates[0] % 10 == 3).sum() > 50
    assert ((ends["flags"] & 2) != 0).sum() == np.isin(fates[0] % 10, (3, 4)).sum() > delivered.sum()
    mask, rg = pupil_mask(), c.geom.eff_reg_FOV_range
    rng = np.random.default_rng(5)
    ln = rng.uniform(-0.2, 0.2, counts.shape[1])
    sens, rw, dep = V.np_reduce(counts, ends, c.nx, c.ny, 3, rg, mask, lnscale=ln)
    got = visits_sensitivity_host(counts, ends, c.nx, c.ny, 3, rg, mask)
    np.testing.assert_array_equal(got, sens)
    assert got[:, :, 0].sum() == counts[delivered].sum() > 0
    # the deposits of every delivered ray: its one out-coupling; its one in-coupling
    names = visit_channels((c.geom.num_fc_slices, c.geom.num_oc_slices))
    assert len(names) == counts.shape[1] == 70
    b3 = [k for k, n in enumerate(names) if n.endswith(".b3")]
    np.testing.assert_array_equal(got[b3].sum(axis=0), dep.astype(np.float64))
    np.testing.assert_array_equal(got[0] + got[1], dep.astype(np.float64))
    # added to, never zeroed
    again = visits_sensitivity_host(counts, ends, c.nx, c.ny, 3, rg, mask, out=got)
    assert again is got
    np.testing.assert_array_equal(got, 2 * sens)
    # re-weighted: zeros give the count table bit for bit; random log-scales give the restatement's deposits exactly
    # (the same libm's exp of the same sum)
    zero = visits_reweight_host(counts, ends, np.zeros_like(ln), c.nx, c.ny, 3, rg, mask)
    np.testing.assert_array_equal(zero, dep.astype(np.float64))
    got = visits_reweight_host(counts, ends, ln, c.nx, c.ny, 3, rg, mask)
    assert np.abs(got - rw).max() <= dep.max() * 2.0 ** -32    # (exp may differ by an ulp between libms: one quantum)
    assert (np.abs(got - rw) <= dep * 2.0 ** -32).all()
    assert got.sum() != zero.sum()
    # n_rows == 0, and what the twins refuse
    np.testing.assert_array_equal(visits_sensitivity_host(counts[:0], ends[:0], c.nx, c.ny, 3, rg, mask), 0 * sens)
    with pytest.raises(Exception, match="mask|binary"):
        visits_sensitivity_host(counts, ends, c.nx, c.ny, 3, rg, mask * 0.5)
    with pytest.raises(ValueError):
        visits_reweight_host(counts, ends, ln[:-1], c.nx, c.ny, 3, rg, mask)


def test_rows_that_deposit_nothing():
    """Not delivered, beside the eyebox, a tile outside the scene, a bin outside the buffer: nothing is added."""
    c = V.config(3, 2, [0, 1, 2], 4)
    rg = c.geom.eff_reg_FOV_range
    ends = np.zeros(5, VISIT_END_DTYPE)
    x = 0.5 * (rg[1, 1, 0] + rg[1, 1, 1])
    y = 0.5 * (rg[1, 1, 2] + rg[1, 1, 3])
    tile = (1 * 3 + 1) * 2 + 1
    ends[0] = (x, y, 7, tile, 3)              # delivered
    ends[1] = (x, y, 8, tile, 2)              # out-coupled beside the eyebox
    ends[2] = (x, y, 9, tile, 0)              # did not out-couple
    ends[3] = (x, y, 10, 3 * 3 * 2, 3)        # a tile the scene does not have
    ends[4] = (x, 1e9, 11, 17, 3)             # the last tile, a bin beyond the buffer
    counts = np.ones((5, 70), np.uint32)
    got = visits_sensitivity_host(counts, ends, 3, 2, 3, rg, pupil_mask())
    assert got[:, :, 0].sum() == 70 and (got[:, :, 0] != 0).sum() == 70
    slab = ((1 * 2 + 1) * 3 + 1)
    assert (got[:, slab, 0] == 1).all()


# 4. the driver's arguments ---------------------------------------------------------------------------------------------

@pytest.fixture
def calls(monkeypatch):
    seen = []

    def fake_run(*args, **kw):
        seen.append((args, kw))
        return {"sensitivity": np.zeros((2, 3, 4))}
    monkeypatch.setattr(drv, "run", fake_run)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    return seen


def test_cli_flags(calls, tmp_path):
    drv.main([])
    assert calls[0][1]["sensitivity"] is None and calls[0][1]["what_if"] is None
    out = tmp_path / "sens.npy"
    drv.main(["--eyebox", "windows", "--sensitivity", "--sensitivity-out", str(out)])
    assert calls[1][1]["sensitivity"] == 8 and calls[1][1]["what_if"] is None and calls[1][1]["eyebox"] == "windows"
    assert np.load(out).shape == (2, 3, 4)
    drv.main(["--eyebox", "windows", "--sensitivity", "3", "--what-if", "r4[2].b3=1.2,r2[0].b2=0.9"])
    assert calls[2][1]["sensitivity"] == 3 and calls[2][1]["what_if"] == {"r4[2].b3": 1.2, "r2[0].b2": 0.9}
    assert calls[2][1]["paths"] is None and calls[2][1]["hits"] is None


@pytest.mark.parametrize("argv", [["--what-if", "r4[2].b3"], ["--what-if", "r4[2].b3=abc"], ["--what-if", "=1.2"],
                                  ["--sensitivity", "0"]])
def test_a_bad_flag_is_an_argument_error(calls, argv, capsys):
    with pytest.raises(SystemExit) as e:
        drv.main(argv)
    assert e.value.code == 2 and not calls


def test_run_refuses_bad_arguments_before_any_gpu_work():
    ok = dict(eyebox="windows")
    for bad in (dict(sensitivity=0), dict(sensitivity=-2), dict(sensitivity=1.5), dict(what_if={}), dict(what_if="r4[0].b3"),
                dict(what_if={"r9[0].b1": 1.1}), dict(what_if={"r4[0].b3": 0.0}), dict(what_if={"r4[0].b3": float("nan")}),
                dict(sensitivity=True, budget=True), dict(sensitivity=True, error_bars=4),
                dict(sensitivity=True, estimator="expected"), dict(sensitivity=True, footprint=(64, 96)),
                dict(sensitivity=True, hits=True), dict(sensitivity=True, paths="eyebox"),
                dict(what_if={"ic.b1": 1.1}, budget=True), dict(what_if={"ic.b1": 1.1}, paths="all"),
                dict(what_if={"ic.b1": 1.1}, hits=True)):
        with pytest.raises(ValueError, match="sensitivity|what_if"):
            drv.run(5, 4, 256, 2, **{**ok, **bad})
    for eyebox in ("host", "device"):
        with pytest.raises(ValueError, match="windows"):
            drv.run(5, 4, 256, 2, eyebox=eyebox, sensitivity=True)


# 5. the identity, statistically, on the checker alone --------------------------------------------------------------------

NX, NY, R = 5, 4, 8192        # `small` with R raised: the baseline delivers > 2,000 rays per wavelength (asserted)
SCALE = 1.15


def identity_z(seed_a, seed_b):
    """Per wavelength: the delivered total of the baseline re-weighted to ``r4[i].b3 x 1.15`` (i: the slice with the most
    visits), the delivered count of the oracle on the ``scale_channel``'d LUTs from independent seeds, and their
    difference in standard errors -- ``sum w^2`` for the re-weighted side, the count for the direct side."""
    from oracle import OracleScene
    c = V.config(NX, NY, [0, 1, 2], R)
    names = visit_channels((7, 6))
    seeds = lambda s: np.random.default_rng(s).integers(1, 2 ** 32, c.N, dtype=np.uint32)
    sc = OracleScene.from_geometry(c.geom, c.luts)
    # first pass: the fates choose the rows, as the driver does
    rng = seeds(seed_a)
    fate = V.checker(sc, c.rays, rng.copy(), slot=np.full(c.N, -1, np.int32), n_rows=0)[4][0]
    mask = fate % 10 == 3
    slot = np.where(mask, np.cumsum(mask) - 1, -1).astype(np.int32)
    counts, ends, _, _, fates = V.checker(sc, c.rays, rng, slot=slot, n_rows=int(mask.sum()))
    counts, ends = counts[0], ends[0]
    np.testing.assert_array_equal(fates[0], fate)
    assert ((ends["flags"] & 1) != 0).all()
    lmd = (ends["tile"] // (NX * NY)).astype(np.int64)
    base = np.bincount(lmd, minlength=3)
    assert (base >= 2000).all(), base
    b3 = [names.index(f"r4[{i}].b3") for i in range(6)]
    i = int(np.argmax(counts[:, b3].sum(axis=0)))
    w = SCALE ** counts[:, b3[i]].astype(np.float64)
    t_rw = np.bincount(lmd, weights=w, minlength=3)
    v_rw = np.bincount(lmd, weights=w * w, minlength=3)
    # the direct run: the scaled design, independent seeds
    sc2 = OracleScene.from_geometry(c.geom, LUTS.scale_channel(c.luts, f"r4[{i}].b3", SCALE))
    f2 = V.checker(sc2, c.rays, seeds(seed_b), slot=np.full(c.N, -1, np.int32), n_rows=0)[4][0]
    direct = np.bincount(c.rays["lmd_num"].astype(np.int64)[f2 % 10 == 3], minlength=3)
    z = (t_rw - direct) / np.sqrt(v_rw + direct)
    return i, base, t_rw, direct, z


def test_reweighted_rays_are_the_scaled_design():
    """5 sigma is a condition on fixed seeds, not a tuned number.  The z-values of this pair and of three further pairs
    are in DESIGN.md 4.10."""
    i, base, t_rw, direct, z = identity_z(1, 2)
    print(f"slice {i}: baseline {base}, re-weighted {t_rw}, direct {direct}, z {z}")
    assert (t_rw > base).all()                              # more out-coupling in the most-visited slice delivers more
    assert (np.abs(z) <= 5.0).all(), z
    print(f"(the unweighted baseline against the direct run: z {(base - direct) / np.sqrt(base + direct)})")
