"""Branch visit counts on the GPU (``wgrt_trace_visits`` through ``torch.ops.wgrt.trace_visits``) and the two reductions
of a table of counted rays (``wgrt_visits_sensitivity``, ``wgrt_visits_reweight``).

Every comparison of counts and end records is equality with the checker's (``tests/oracle_visits.c``: the CPU oracle with
its hooks defined, restating the branch decision and the channel table on its own): the counts are integers, and the
positions are the same doubles on both lanes and in the oracle, as the hit-list and path tests already rely on.  The
sensitivity tables are compared with ``assert_array_equal`` on float64 integers.  The walk is compared as bytes with the
same launches without counts."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from gpu_ray_tracing_for_waveguide_based_ar_display_amd import _lib  # noqa: E402
from gpu_ray_tracing_for_waveguide_based_ar_display_amd._lib import STAT  # noqa: E402
from tests import _visits as V  # noqa: E402
from tests import _kernel_table as KT  # noqa: E402
from tests._fixtures import GoldenCase  # noqa: E402
from tests.test_gpu_parity import _config  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURES = ["c1_rgb", "h6_edge_rgb", "s1_532"]
_CONFIGS = {"c2s": dict(nx=11, ny=11, lambdas=[1], R=64),                      # 7,744 rays: > replay_tail's 256 threads
            "small": dict(nx=5, ny=4, lambdas=[0, 1, 2], R=100),
            "small_amp": dict(nx=5, ny=4, lambdas=[0, 1, 2], R=100, profile="adversarial_polarizing", seed=3)}
CANARY = 0xA5
PAD = 8          # canary rows behind both arrays


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


@pytest.fixture(autouse=True)
def _switches():
    yield
    _lib.set_byte_locator(True)


_cases, _checked = {}, {}


def _case(name):
    if name not in _cases:
        if KT.is_case(name):   # the kernel table's four cases (tests/_kernel_table.py), shared by every sink module
            _cases[name] = KT.case(name)
        else:
            _cases[name] = GoldenCase(name) if name in FIXTURES else _config(**_CONFIGS[name])
    return _cases[name]


def _nl(c):
    return 1 if getattr(c, "wavelength", None) is not None else 3


def checked(name, launches=1):
    """The checker on case ``name`` with every ray counted into its own row, the rows zeroed at every launch, once per
    key and shared, read-only: ``dict(counts [launches, N, C], ends [launches, N], rng, bounces, fates, eb)``."""
    key = (name, launches)
    if key not in _checked:
        from oracle import OracleScene
        c = _case(name)
        sc = OracleScene.from_geometry(c.geom, c.luts, wavelength=getattr(c, "wavelength", None))
        eb = np.zeros(c.eb_shape(), np.float32)
        counts, ends, rng, bounces, fates = V.checker(sc, c.rays, c.fresh_rng(), launches, eb=eb)
        r = dict(counts=counts, ends=ends, rng=rng, bounces=bounces, fates=fates, eb=eb)
        for v in r.values():
            v.setflags(write=False)
        _checked[key] = r
    return _checked[key]


def _table(scene, n_rows, dev):
    """A VisitTable of ``n_rows`` rows inside buffers with PAD canary rows behind them."""
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import VisitTable
    vt = VisitTable(scene, n_rows + PAD, dev)
    vt.counts[n_rows:].fill_(-1)
    vt.ends[n_rows:].fill_(CANARY)
    vt.n_rows = n_rows
    return vt


def _rows(vt):
    """``(counts uint32 [n_rows, C], ends [n_rows])`` on the host, the canary rows checked and cut off."""
    counts, ends = vt.counts.cpu().numpy().view(np.uint32), vt.ends.cpu().numpy()
    assert (counts[vt.n_rows:] == 0xFFFFFFFF).all() and (ends[vt.n_rows:] == CANARY).all()
    return counts[:vt.n_rows].copy(), ends[:vt.n_rows].reshape(-1).view(V.DTYPE).copy()


def _trace(c, dev, launches=1, variant=0, visits=True, slot=None, n_rows=None, rays=None, rng=None, scene=None, vt=None,
           keep=False, **kw):
    """``launches`` single launches into the grid, the window table and (``visits``) a visit table that is read back and
    zeroed after every launch: ``SimpleNamespace(counts [launches, n_rows, C], ends [launches, n_rows], rng, eb, table,
    stats, per)`` on the host.  ``visits=False``: the same calls without counts.  ``keep``: also ``vt``, ``scene`` and
    ``plan``, left open (the table as the last launch left it)."""
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import (Scene, WindowPlan, new_stats, rays_to_device,
                                                                           trace_fullcolor, trace_single)
    wl = getattr(c, "wavelength", None)
    own = scene is None
    if own:
        scene = Scene.from_geometry(c.geom, c.luts, wavelength=wl)
    plan = WindowPlan()
    trace = trace_single if wl is not None else trace_fullcolor
    table = plan.new_table(scene)
    eb = torch.zeros(scene.eb_shape(), dtype=torch.float32, device=dev)
    rays = rays_to_device(c.rays, dev) if rays is None else rays
    rng = torch.from_numpy(c.fresh_rng().view(np.int32)).to(dev) if rng is None else rng
    if vt is None and visits:
        vt = _table(scene, rng.numel() if n_rows is None else n_rows, dev)
    stats = new_stats(dev)
    per = torch.zeros(rng.numel(), dtype=torch.int32, device=dev)
    counts, ends = [], []
    for k in range(launches):
        kw2 = dict(visits=(vt, slot[k] if isinstance(slot, list) else slot)) if visits else {}
        trace(scene, rays, rng, eb, stats=stats, per_ray_bounces=per, variant=variant, windows=(plan, table), **kw2, **kw)
        if visits:
            torch.cuda.synchronize()
            a, b = _rows(vt)
            counts.append(a)
            ends.append(b)
            if k + 1 < launches:
                vt.counts[:vt.n_rows].zero_()
                vt.ends[:vt.n_rows].zero_()
    torch.cuda.synchronize()
    out = SimpleNamespace(counts=np.stack(counts) if visits else None, ends=np.stack(ends) if visits else None,
                          rng=rng.cpu().numpy().view(np.uint32).copy(), eb=eb.cpu().numpy(), table=table.cpu().numpy(),
                          stats=stats.cpu().numpy().copy(), per=per.cpu().numpy().view(np.uint32).copy())
    if keep:
        out.vt, out.scene, out.plan = vt, scene, plan
    else:
        plan.close()
        if own:
            scene.close()
    return out


def _same_walk(a, b):
    np.testing.assert_array_equal(a.rng, b.rng)
    np.testing.assert_array_equal(a.per, b.per)
    np.testing.assert_array_equal(a.stats, b.stats)
    assert a.eb.tobytes() == b.eb.tobytes() and a.table.tobytes() == b.table.tobytes()


def _same_rows(got_counts, got_ends, counts, ends):
    assert got_counts.dtype == np.uint32 and got_counts.shape == counts.shape, (got_counts.shape, counts.shape)
    np.testing.assert_array_equal(got_counts, counts)
    assert got_ends.dtype == V.DTYPE and got_ends.shape == ends.shape
    assert got_ends.tobytes() == np.ascontiguousarray(ends).tobytes()


# 1. every ray counted: every variant, two chained launches; the anchor --------------------------------------------------

@pytest.mark.parametrize("variant", [1, 7, 9])
@pytest.mark.parametrize("name", FIXTURES + ["small", "c2s"])
def test_counts_ends_and_walk(dev, name, variant):
    c = _case(name)
    chk = checked(name, 2)
    got = _trace(c, dev, launches=2, variant=variant)
    _same_rows(got.counts, got.ends, chk["counts"], chk["ends"])
    assert got.counts.sum() > c.N                                          # the event's branch and the loop's
    # every counted draw but the in-coupling event's is an interaction; a lost ray's last draw counts nothing
    lost = int((chk["fates"] % 10 == 2).sum())
    traced = int((chk["fates"] != 0).sum())
    assert int(got.counts.sum()) == int(got.stats[STAT.interactions]) + traced - lost
    assert ((got.ends["flags"] & 2) != 0).sum() == np.isin(chk["fates"] % 10, (3, 4)).sum() > 0
    # (a ray inside its rectangle whose bin lies outside the buffer is delivered and no hit: h6_edge_rgb has some)
    assert ((got.ends["flags"] & 1) != 0).sum() == (chk["fates"] % 10 == 3).sum() >= int(got.stats[STAT.eyebox_hits])
    np.testing.assert_array_equal(got.rng, chk["rng"])
    np.testing.assert_array_equal(got.per, chk["bounces"])
    assert got.eb.tobytes() == chk["eb"].tobytes()
    _same_walk(got, _trace(c, dev, launches=2, variant=variant, visits=False))


# 2. two-pass selection: a fate launch from a clone of the states gives the delivered rays their rows ------------------

@pytest.mark.parametrize("variant", [1, 7])
@pytest.mark.parametrize("name", ["small", "c2s"])
def test_two_pass_selection(dev, name, variant):
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import (Scene, rays_to_device, select_by_fate,
                                                                           trace_fullcolor)
    c = _case(name)
    chk = checked(name)
    scene = Scene.from_geometry(c.geom, c.luts)
    rays = rays_to_device(c.rays, dev)
    rng = torch.from_numpy(c.fresh_rng().view(np.int32)).to(dev)
    fate = torch.zeros(c.N, dtype=torch.uint8, device=dev)
    eb = torch.zeros(scene.eb_shape(), dtype=torch.float32, device=dev)
    trace_fullcolor(scene, rays, rng.clone(), eb, variant=variant, fate=fate)
    mask = select_by_fate(fate, "eyebox").to(torch.int32)
    slot = torch.where(mask != 0, torch.cumsum(mask, 0, dtype=torch.int32) - mask, torch.full_like(mask, -1))
    n = int(mask.sum())
    got = _trace(c, dev, variant=variant, slot=slot, n_rows=n, rays=rays, rng=rng, scene=scene)
    m = mask.cpu().numpy() != 0
    np.testing.assert_array_equal(fate.cpu().numpy(), chk["fates"][0])
    assert 0 < n < c.N
    # the rows are compact, in ray order, and the checker's rows of those rays; every one is a delivered ray's
    _same_rows(got.counts[0], got.ends[0], chk["counts"][0][m], chk["ends"][0][m])
    assert (got.ends[0]["flags"] == 3).all() and (np.diff(got.ends[0]["gid"]) > 0).all()
    np.testing.assert_array_equal(got.rng, chk["rng"])
    _same_walk(got, _trace(c, dev, variant=variant, visits=False, scene=scene))
    # an all-negative slot array leaves both arrays zero
    none = _trace(c, dev, variant=variant, slot=torch.full((c.N,), -1, dtype=torch.int32, device=dev), n_rows=n,
                  scene=scene)
    assert not none.counts.any() and not none.ends.view(np.uint8).any()
    _same_walk(none, got)
    scene.close()


# 3. abandoned rays: the replay passes over what the Jones lane had counted -------------------------------------------

@pytest.mark.parametrize("debug, every", [(dict(cert_tol=1e-2), False), (dict(cert_tol=1e3, cert_tol32=1e3), True)])
def test_abandoned_rays_are_counted_once(dev, debug, every):
    c = _case("c2s")
    chk = checked("c2s")
    got = _trace(c, dev, variant=7, debug=debug)
    traced, replayed = c.N - int(got.stats[STAT.bad_rays]), int(got.stats[STAT.replayed])
    print(f"replayed {replayed} of {traced}")
    if every:
        assert replayed == traced > 256
    else:
        assert 0 < replayed < traced
    _same_rows(got.counts, got.ends, chk["counts"], chk["ends"])
    np.testing.assert_array_equal(got.per, chk["bounces"])
    np.testing.assert_array_equal(got.rng, chk["rng"])
    _same_walk(got, _trace(c, dev, variant=7, debug=debug, visits=False))


# 4. both locator forms, the single-wavelength kernel, the AMP profile, split batches ---------------------------------

@pytest.mark.parametrize("variant", [7, 9])
def test_byte_and_word_locator(dev, variant):
    c = _case("small")
    chk = checked("small")
    for byte in (True, False):
        _lib.set_byte_locator(byte)
        got = _trace(c, dev, variant=variant)
        _same_rows(got.counts, got.ends, chk["counts"], chk["ends"])
        np.testing.assert_array_equal(got.rng, chk["rng"])
    _lib.set_byte_locator(True)


def test_single_wavelength(dev):
    c = _case("s1_532")
    assert getattr(c, "wavelength", None) is not None
    chk = checked("s1_532")
    for variant in (1, 7, 9):
        got = _trace(c, dev, variant=variant)
        assert (got.ends["tile"] < c.nx * c.ny).all()
        _same_rows(got.counts, got.ends, chk["counts"], chk["ends"])
        np.testing.assert_array_equal(got.rng, chk["rng"])


def test_amp_profile(dev):
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import Scene
    c = _case("small_amp")
    sc = Scene.from_geometry(c.geom, c.luts)
    assert sc.info()["nonunitary_blocks"] > 0
    sc.close()
    chk = checked("small_amp", 2)
    for variant in (7, 9):
        got = _trace(c, dev, launches=2, variant=variant)
        _same_rows(got.counts, got.ends, chk["counts"], chk["ends"])
        np.testing.assert_array_equal(got.rng, chk["rng"])
    # ``small_amp`` delivers no ray in its two launches (every table of its profile is near-singular), so its rows hold no flags 3: it keeps
    # the abandon path of near-singular matrices.  The delivering AMP case (tests/_kernel_table.py: the default LUTs with
    # a non-unitary lut_fc2) makes the AMP kernels write delivered rows.
    name = KT.CASE_OF[(0, 1)]
    c = _case(name)
    sc = Scene.from_geometry(c.geom, c.luts)
    assert sc.info()["nonunitary_blocks"] > 0
    sc.close()
    chk = checked(name, 2)
    assert (chk["ends"]["flags"] == 3).sum() > 0 and chk["eb"].sum() > 0
    for variant in (7, 9):
        got = _trace(c, dev, launches=2, variant=variant)
        _same_rows(got.counts, got.ends, chk["counts"], chk["ends"])
        np.testing.assert_array_equal(got.rng, chk["rng"])
        assert got.eb.tobytes() == chk["eb"].tobytes()


@pytest.mark.parametrize("variant", [1, 7])
def test_a_batch_split_at_ray_37(dev, variant):
    """The two parts count into one table: the slots are global rows, the ids come from ``gid_offset``."""
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import Scene, rays_to_device
    c = _case("c1_rgb")
    chk = checked("c1_rgb")
    scene = Scene.from_geometry(c.geom, c.luts)
    vt = _table(scene, c.N, dev)
    full = rays_to_device(c.rays, dev)
    rng_all = torch.from_numpy(c.fresh_rng().view(np.int32)).to(dev)
    rows = torch.arange(c.N, dtype=torch.int32, device=dev)
    got_rng = []
    for lo, hi in ((0, 37), (37, c.N)):
        rays = {k: v[lo:hi].contiguous() for k, v in full.items()}
        r = _trace(c, dev, variant=variant, rays=rays, rng=rng_all[lo:hi].contiguous(), vt=vt, scene=scene,
                   slot=rows[lo:hi].contiguous(), gid_offset=lo)
        got_rng.append(r.rng)
    counts, ends = _rows(vt)
    scene.close()
    _same_rows(counts, ends, chk["counts"][0], chk["ends"][0])
    np.testing.assert_array_equal(np.concatenate(got_rng), chk["rng"])


def test_two_gid_blocks_shards_add_up_to_the_whole(dev):
    """Rows are local to a shard; the ids in the end records are global, and the shards' sensitivity tables add up to the
    whole batch's."""
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.AR_system_evaluation_functions import pupil_mask
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.distributed import make_shard
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import init_rays, visits_sensitivity_host
    c = _case("c1_rgb")
    chk = checked("c1_rgb")
    sens, gids, total = None, [], 0
    for r in range(2):
        shard = make_shard(c.nx, c.ny, len(c.lambdas), c.R, 2, r)
        rays, rng = init_rays(c.f["points"], c.nx, c.ny, c.lambdas, c.R, block_list=shard.blocks, device=dev)
        gb = torch.from_numpy(shard.gid.block_gid).to(dev)
        got = _trace(c, dev, variant=7, rays=rays, rng=rng, n_rays=rng.numel(), gid_blocks=gb, gid_block_rays=c.R,
                     keep=True)
        out = got.ends[0]["flags"] != 0
        g = got.ends[0]["gid"][out]
        gids.append(g)
        # a shard's rows are the checker's rows of the rays with those global ids
        np.testing.assert_array_equal(got.counts[0][out], chk["counts"][0][g])
        assert got.ends[0][out].tobytes() == chk["ends"][0][g].tobytes()
        total += int(got.counts.sum())
        sens = got.vt.sensitivity(got.plan, out=sens)
        got.plan.close()
        got.scene.close()
    torch.cuda.synchronize()
    assert total == int(chk["counts"].sum()) and len(np.unique(np.concatenate(gids))) == (chk["ends"]["flags"] != 0).sum()
    want = visits_sensitivity_host(chk["counts"][0], chk["ends"][0], c.nx, c.ny, 3, c.geom.eff_reg_FOV_range, pupil_mask())
    np.testing.assert_array_equal(sens.cpu().numpy(), want)
    assert want.sum() > 0


# 5. the reductions ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["small", "h6_edge_rgb", "s1_532"])
def test_reductions(dev, name):
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.AR_system_evaluation_functions import pupil_mask
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import (visit_channels, visits_reweight_host,
                                                                           visits_sensitivity_host)
    c = _case(name)
    chk = checked(name)
    nl = _nl(c)
    got = _trace(c, dev, variant=7, keep=True)
    vt, plan = got.vt, got.plan
    try:
        _same_rows(got.counts, got.ends, chk["counts"], chk["ends"])
        rg, mask = c.geom.eff_reg_FOV_range, pupil_mask()
        ln = np.random.default_rng(11).uniform(-0.2, 0.2, vt.n_channels)
        want, _, dep = V.np_reduce(chk["counts"][0], chk["ends"][0], c.nx, c.ny, nl, rg, mask)
        sens = vt.sensitivity(plan)
        torch.cuda.synchronize()
        assert sens.dtype == torch.float64 and tuple(sens.shape) == (vt.n_channels,) + got.table.shape
        s = sens.cpu().numpy()
        np.testing.assert_array_equal(s, want)
        np.testing.assert_array_equal(s, visits_sensitivity_host(chk["counts"][0], chk["ends"][0], c.nx, c.ny, nl, rg, mask))
        # every delivered ray out-coupled once and in-coupled once: both sums are the launch's window table
        b3 = [k for k, n in enumerate(visit_channels(got.scene)) if n.endswith(".b3")]
        np.testing.assert_array_equal(s[b3].sum(axis=0), got.table)
        np.testing.assert_array_equal(s[0] + s[1], got.table)
        np.testing.assert_array_equal(dep.astype(np.float64), got.table)
        assert got.table.sum() > 0
        # added to, never zeroed
        assert vt.sensitivity(plan, out=sens) is sens
        np.testing.assert_array_equal(sens.cpu().numpy(), 2 * want)
        # re-weighted with zeros: the launch's window table, bit for bit (a dict of ones and a tensor of ones alike)
        one = vt.reweight(plan, torch.ones(vt.n_channels, dtype=torch.float64))
        assert one.cpu().numpy().tobytes() == got.table.tobytes()
        assert vt.reweight(plan, {"ic.b1": 1.0}).cpu().numpy().tobytes() == got.table.tobytes()
        # ... with log-scales drawn from [-0.2, 0.2]: within D * 2^-32 per entry of the host twin, D the entry's deposits
        rw = vt.reweight(plan, np.exp(ln)).cpu().numpy()
        twin = visits_reweight_host(chk["counts"][0], chk["ends"][0], ln, c.nx, c.ny, nl, rg, mask)
        diff = np.abs(rw - twin)
        print(f"{name}: {int((diff != 0).sum())} of {int((dep != 0).sum())} entries differ from the host twin, "
              f"at most {diff.max() * 2.0 ** 32:g} quanta")
        assert (diff <= dep * 2.0 ** -32).all()
        assert np.abs(rw - got.table).max() > 0
        # the effective sample size: torch, from the same rows
        on = (chk["ends"][0]["flags"] & 1) != 0
        w = np.exp(chk["counts"][0][on].astype(np.float64) @ ln)
        l = chk["ends"][0]["tile"][on] // (c.nx * c.ny)
        s1, s2 = np.bincount(l, weights=w, minlength=nl), np.bincount(l, weights=w * w, minlength=nl)
        np.testing.assert_allclose(vt.ess(np.exp(ln)).cpu().numpy(), s1 * s1 / np.maximum(s2, 1e-300), rtol=1e-12)
        np.testing.assert_allclose(vt.ess({"r2[0].b1": 1.0}).cpu().numpy(), np.bincount(l, minlength=nl), rtol=1e-12)
        # n_rows == 0 launches nothing
        vt.n_rows = 0
        np.testing.assert_array_equal(vt.sensitivity(plan).cpu().numpy(), 0 * want)
        assert not vt.reweight(plan, np.exp(ln)).any()
    finally:
        plan.close()
        got.scene.close()


# 6. refusals --------------------------------------------------------------------------------------------------------

def test_refusals(dev):
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import (FootprintPlan, HitList, PathList, Scene,
                                                                           TraceChain, VisitTable, WindowPlan, _debug_opts,
                                                                           rays_to_device, trace_fullcolor)
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd._lib import load, ops
    c = _case("c1_rgb")
    scene, plan = Scene.from_geometry(c.geom, c.luts), WindowPlan()
    rays = rays_to_device(c.rays, dev)
    rng = torch.from_numpy(c.fresh_rng().view(np.int32)).to(dev)
    before = rng.clone()
    vt = VisitTable(scene, c.N, dev)
    grid = torch.zeros(c.eb_shape(), dtype=torch.float32, device=dev)
    table = plan.new_table(scene)
    go = lambda **kw: trace_fullcolor(scene, rays, rng, grid, variant=7, visits=(vt, None), **kw)
    with pytest.raises(ValueError, match="num_iter"):
        go(num_iter=2)
    with pytest.raises(ValueError, match="fate"):
        go(fate=torch.zeros(c.N, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="replicas"):
        go(windows=(plan, plan.new_table(scene, replicas=4)), replicas=4)
    with pytest.raises(ValueError, match="expected"):
        trace_fullcolor(scene, rays, rng, None, windows=(plan, table), expected=True, visits=(vt, None))
    fp = FootprintPlan.for_scene(c.geom, cells=(8, 8))
    with pytest.raises(ValueError, match="footprint"):
        go(footprint=(fp, fp.new_map(scene)))
    with pytest.raises(ValueError, match="hits"):
        go(hits=(HitList(4, dev), 0))
    with pytest.raises(ValueError, match="paths"):
        go(paths=(PathList(4, dev), 0))
    with pytest.raises(ValueError, match="chain"):
        TraceChain(scene, rays, rng, grid, visits=(vt, None))
    with pytest.raises(TypeError):
        trace_fullcolor(scene, rays, rng, grid, visits=(vt.counts, None))
    # the device does not validate slots: the Python layer does
    slot = torch.zeros(c.N, dtype=torch.int32, device=dev)
    slot[5] = c.N
    with pytest.raises(ValueError, match="slot"):
        trace_fullcolor(scene, rays, rng, grid, variant=7, visits=(vt, slot))
    with pytest.raises(ValueError, match="rows"):
        trace_fullcolor(scene, rays, rng, grid, variant=7, visits=(VisitTable(scene, c.N - 1, dev), None))

    # the operator and the C entry point themselves: each returns its status and launches nothing
    def op(counts=vt.counts, ends=vt.ends, n_rows=c.N, slot=None, num_iter=1, debug=0, variant=7):
        return ops().trace_visits(scene.handle.value, rays["x"], rays["y"], rays["m"], rays["n"], rays["lmd_num"],
                                  rays["te"], rays["tm"], rays["delta_phase"], rng, grid, None, None, c.N, 0, 0, 0, variant,
                                  0, None, num_iter, None, 0, debug, 0.0, 0, None, slot, n_rows, counts, ends)
    for v in (1, 7):
        assert op(num_iter=2, variant=v) == 1                                      # WGRT_ERR_INVALID_ARGUMENT
        assert op(n_rows=-1, variant=v) == 1
        assert op(n_rows=c.N - 1, variant=v) == 1                                  # no slots: row i for ray i
        assert op(ends=vt.ends.reshape(-1)[8:], n_rows=c.N - 1, slot=torch.zeros(c.N, dtype=torch.int32, device=dev),
                  variant=v) == 1                                                  # a misaligned ends
    tl = torch.zeros(8 * 64, dtype=torch.int64, device=dev)
    dbg = _debug_opts(dict(timeline=tl))
    assert op(debug=ctypes.addressof(dbg)) == 4                                    # WGRT_ERR_UNSUPPORTED
    with pytest.raises(RuntimeError, match="int32"):
        op(counts=vt.counts.to(torch.int64))
    with pytest.raises(RuntimeError, match="n_rows"):
        op(n_rows=c.N + 1)
    with pytest.raises(RuntimeError, match="slot"):
        op(slot=torch.zeros(c.N, dtype=torch.int64, device=dev))
    # the reductions' own refusals
    sens = torch.zeros((vt.n_channels,) + tuple(table.shape), dtype=torch.float64, device=dev)
    red = lambda **kw: ops().visits_reduce(*[{**dict(scene=scene.handle.value, plan=plan.handle.value, counts=vt.counts,
                                                     ends=vt.ends, n_rows=c.N, lnscale=None, out=sens, stream=0), **kw}[k]
                                             for k in ("scene", "plan", "counts", "ends", "n_rows", "lnscale", "out", "stream")])
    with pytest.raises(RuntimeError, match="n_rows"):
        red(n_rows=-1)
    with pytest.raises(RuntimeError, match="out"):
        red(out=table)
    with pytest.raises(RuntimeError, match="lnscale"):
        red(out=table, lnscale=torch.zeros(3, dtype=torch.float64, device=dev))
    L = load()
    assert L.wgrt_visits_sensitivity(scene.handle, plan.handle, vt.counts.data_ptr(), vt.ends.data_ptr() + 8, 4,
                                     sens.data_ptr(), None) == 1               # a misaligned ends
    assert L.wgrt_visits_sensitivity(scene.handle, plan.handle, vt.counts.data_ptr(), vt.ends.data_ptr(), -1,
                                     sens.data_ptr(), None) == 1
    assert L.wgrt_visits_reweight(scene.handle, plan.handle, vt.counts.data_ptr(), vt.ends.data_ptr(), 4, None,
                                  table.data_ptr(), None) == 1                 # no lnscale
    assert L.wgrt_visits_sensitivity(scene.handle, None, vt.counts.data_ptr(), vt.ends.data_ptr(), 4, sens.data_ptr(),
                                     None) == 1
    assert L.wgrt_visit_channels(scene.handle) == vt.n_channels == 70 and L.wgrt_visit_channels(None) == -1
    torch.cuda.synchronize()
    assert torch.equal(rng, before) and not grid.any() and not tl.any()            # nothing was launched
    assert not vt.counts.any() and not vt.ends.any() and not sens.any() and not table.any()

    # counts == NULL: the windows launch, bit for bit (slot, n_rows and ends are not looked at)
    cols = _lib.Rays(**{k: ctypes.c_void_p(rays[k].data_ptr()) for k in ("x", "y", "m", "n", "lmd_num", "te", "tm",
                                                                          "delta_phase")})
    opts = _lib.LaunchOpts()
    opts.variant = 7
    st = torch.zeros(_lib.STATS_LEN, dtype=torch.int64, device=dev)
    assert L.wgrt_trace_visits(scene.handle, ctypes.byref(cols), c.N, 0, rng.data_ptr(), grid.data_ptr(),
                               st.data_ptr(), None, None, ctypes.byref(opts), plan.handle, table.data_ptr(), None,
                               -5, None, None) == 0
    rng2, grid2, table2, st2 = before.clone(), torch.zeros_like(grid), torch.zeros_like(table), torch.zeros_like(st)
    assert L.wgrt_trace_windows(scene.handle, ctypes.byref(cols), c.N, 0, rng2.data_ptr(), grid2.data_ptr(),
                                st2.data_ptr(), None, None, ctypes.byref(opts), plan.handle, table2.data_ptr()) == 0
    # counts without ends is refused
    assert L.wgrt_trace_visits(scene.handle, ctypes.byref(cols), c.N, 0, rng2.data_ptr(), grid2.data_ptr(),
                               st2.data_ptr(), None, None, ctypes.byref(opts), plan.handle, table2.data_ptr(), None,
                               c.N, vt.counts.data_ptr(), None) == 1
    torch.cuda.synchronize()
    assert torch.equal(rng, rng2) and torch.equal(grid, grid2) and torch.equal(table, table2) and torch.equal(st, st2)
    assert grid.sum() > 0 and not vt.counts.any()
    plan.close()
    scene.close()


# 7. the driver ------------------------------------------------------------------------------------------------------
# the small job of tests/test_gpu_paths.py ("deep" LUT profile)

NX, NY, R, STEPS = 5, 4, 256, 2
WHAT_IF = {"r4[2].b3": 1.2, "r2[0].b2": 0.9}
_runs = {}


def _run(on, **kw):
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.gpu_ray_tracing_pro_fullColor import run
    from tests import _dist
    pts = _dist.small_job(NX, NY, R, 3, 6, "deep")[2]
    more = dict(sensitivity=True, what_if=WHAT_IF) if on else {}
    return run(NX, NY, R, STEPS, lut_seed=3, lut_profile="deep", points=pts, verbose=False, eyebox="windows",
               evaluate_on="device", **more, **kw)


def _run_once(on):
    if on not in _runs:
        _runs[on] = _run(on)
    return _runs[on]


def _by_hand():
    """The sum of the per-launch reductions, by hand: the checker on the driver's batch, launch k's rows the rays its own
    fates of launch k deliver, reduced by the host twins."""
    from oracle import OracleScene
    from tests import _dist
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.AR_system_evaluation_functions import pupil_mask
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import (visit_channels, visits_reweight_host,
                                                                           visits_sensitivity_host)
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.rays import build_rays, rng_seeds
    geom, luts, pts = _dist.small_job(NX, NY, R, 3, 6, "deep")
    rays = build_rays(pts, NX, NY, (0, 1, 2), R)
    N = rays["x"].shape[0]
    sc = OracleScene.from_geometry(geom, luts)
    counts, ends, rng, _, fates = V.checker(sc, rays, rng_seeds(N), STEPS)
    names = visit_channels((geom.num_fc_slices, geom.num_oc_slices))
    ln = np.zeros(len(names))
    for k, v in WHAT_IF.items():
        ln[names.index(k)] = np.log(v)
    sens = table = None
    dep = 0
    sums = np.zeros((2, 3))
    for k in range(STEPS):
        m = fates[k] % 10 == 3
        a = (counts[k][m], ends[k][m], NX, NY, 3, geom.eff_reg_FOV_range, pupil_mask())
        sens = visits_sensitivity_host(*a, out=sens)
        table = visits_reweight_host(a[0], a[1], ln, *a[2:], out=table)
        dep = dep + visits_reweight_host(a[0], a[1], 0 * ln, *a[2:])
        w = np.exp(a[0].astype(np.float64) @ ln)
        l = a[1]["tile"] // (NX * NY)
        sums += np.stack([np.bincount(l, weights=w, minlength=3), np.bincount(l, weights=w * w, minlength=3)])
    return sens, table, dep, sums, rng, names


def _check_driver(got, plain):
    assert set(got) - set(plain) == {"sensitivity", "sensitivity_channels", "what_if"}
    for k in plain:   # efficiencies, evaluation and everything else returned before, bit for bit (the timings aside)
        if k in ("gpu_seconds", "post_seconds"):
            continue
        a, b = got[k], plain[k]
        if isinstance(a, np.ndarray):
            assert a.tobytes() == b.tobytes(), k
        else:
            assert a == b or (isinstance(a, float) and float(a).hex() == float(b).hex()), k
    sens, table, dep, sums, rng, names = _by_hand()
    np.testing.assert_array_equal(got["rng_states"], rng)
    assert got["sensitivity_channels"] == names
    np.testing.assert_array_equal(got["sensitivity"], sens)
    assert sens.sum() > 0
    w = got["what_if"]
    assert w["scales"] == WHAT_IF
    assert (np.abs(w["table"] - table) <= dep * 2.0 ** -32).all() and np.abs(w["table"] - dep).max() > 0
    np.testing.assert_allclose(w["ess"], sums[0] ** 2 / sums[1], rtol=1e-9)
    A = w["table"][:, 0].reshape(3, NY, NX).astype(np.float32) / (NX * NY * 3 * R) / STEPS
    np.testing.assert_array_equal(w["A"], A)
    assert w["efficiency"] == {n: float(np.sum(A[k] * 3)) for k, n in ((0, "Blue"), (1, "Green"), (2, "Red"))}
    assert all(np.isfinite(w[k]) for k in ("delta_e", "U_fov", "U_EB"))
    # the elasticity of the in-coupling event's two branches sums to 1: every delivered ray took one of them once
    per = got["sensitivity"][:2, :, 0].reshape(2, 3, -1).sum(axis=(0, 2))
    np.testing.assert_array_equal(per, dep[:, 0].reshape(3, -1).sum(axis=1))


def test_driver_sensitivity_and_what_if(dev):
    _check_driver(_run_once(True), _run_once(False))
    only = _run(False, sensitivity=3)
    assert "what_if" not in only
    np.testing.assert_array_equal(only["sensitivity"], _run_once(True)["sensitivity"])
    for bad in (dict(budget=True), dict(error_bars=4), dict(estimator="expected"), dict(footprint=(64, 96)),
                dict(hits=True), dict(paths="eyebox")):
        with pytest.raises(ValueError, match="sensitivity"):
            _run(True, **bad)


def _driver_worker(rank, world, outdir):
    torch.cuda.set_device(torch.device("cuda", 0))
    res = _run(True)
    if rank != 0:
        assert "sensitivity" not in res and "what_if" not in res
        return
    np.save(f"{outdir}/sens.npy", res["sensitivity"])
    np.save(f"{outdir}/what_if.npy", res["what_if"]["table"])
    np.save(f"{outdir}/ess.npy", res["what_if"]["ess"])


def test_driver_in_two_ranks(dev, tmp_path):
    """Two ranks on the one GPU over gloo: the tables are sums over rays, so the ranks' tables add up to the
    single-process tables."""
    from tests import _dist
    _dist.spawn(_driver_worker, 2, str(tmp_path))
    one = _run_once(True)
    np.testing.assert_array_equal(np.load(tmp_path / "sens.npy"), one["sensitivity"])
    # (multiples of 2^-32: the order of the sums does not matter)
    np.testing.assert_array_equal(np.load(tmp_path / "what_if.npy"), one["what_if"]["table"])
    np.testing.assert_allclose(np.load(tmp_path / "ess.npy"), one["what_if"]["ess"], rtol=1e-9)
