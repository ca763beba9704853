"""The footprint maps on the GPU (``wgrt_trace_footprint`` through ``torch.ops.wgrt.trace_footprint``) and the driver's
``run(footprint=(H, W))``.

Every comparison with the checker (``tests/oracle_footprint.c``: the CPU oracle with its event hook defined) is exact
equality of the whole int64 map: the positions are the same doubles on both lanes and in the oracle, and the rule is a
subtraction, a division and a floor.  The walk is compared as bytes with the same launch without a map."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from gpu_ray_tracing_for_waveguide_based_ar_display_amd import _lib  # noqa: E402
from gpu_ray_tracing_for_waveguide_based_ar_display_amd._lib import STAT  # noqa: E402
from tests import _footprint as F  # noqa: E402
from tests import _kernel_table as KT  # noqa: E402
from tests._fixtures import GoldenCase  # noqa: E402
from tests.test_gpu_parity import _config  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURES = ["c1_rgb", "h6_edge_rgb", "s1_532"]
_CONFIGS = {"c2s": dict(nx=11, ny=11, lambdas=[1], R=64),                      # 7,744 rays: > replay_tail's 256 threads
            "small": dict(nx=5, ny=4, lambdas=[0, 1, 2], R=100),
            "small_deep": dict(nx=5, ny=4, lambdas=[0, 1, 2], R=100, profile="deep", seed=3),
            "small_amp": dict(nx=5, ny=4, lambdas=[0, 1, 2], R=100, profile="adversarial_polarizing", seed=3)}
CELLS = (48, 80)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


@pytest.fixture(autouse=True)
def _switches():
    yield
    _lib.set_byte_locator(True)
    _lib.set_footprint_aggregate(True)


_cases, _checked = {}, {}


def _case(name):
    if name not in _cases:
        if KT.is_case(name):   # the kernel table's four cases (tests/_kernel_table.py), shared by every sink module
            _cases[name] = KT.case(name)
        else:
            _cases[name] = GoldenCase(name) if name in FIXTURES else _config(**_CONFIGS[name])
    return _cases[name]


def _plan(c, kind="scene"):
    """The plans the tests use: ``for_scene`` at CELLS; one cell over the whole plate; 1024 x 1024; a rectangle
    smaller than the plate."""
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import FootprintPlan
    fp = FootprintPlan.for_scene(c.geom, cells=CELLS)
    if kind == "scene":
        return fp
    if kind == "fine":
        return FootprintPlan.for_scene(c.geom, cells=(1024, 1024))
    if kind == "one":
        return FootprintPlan(fp.x0, fp.y0, fp.cell_x * fp.nx_cells, fp.cell_y * fp.ny_cells, 1, 1)
    assert kind == "cut"
    return FootprintPlan(fp.x0 + 20 * fp.cell_x, fp.y0 + 10 * fp.cell_y, fp.cell_x, fp.cell_y, 30, 20)


def checked(name, launches=1, kind="scene", stride=(0, 1)):
    """The checker on case ``name`` (rays ``stride[0]::stride[1]``), once per key and shared, read-only:
    ``dict(map, rng, bounces, eb)``."""
    key = (name, launches, kind, stride)
    if key not in _checked:
        from oracle import OracleScene
        c = _case(name)
        sc = OracleScene.from_geometry(c.geom, c.luts, wavelength=getattr(c, "wavelength", None))
        sl = slice(stride[0], None, stride[1])
        rays = {k: np.ascontiguousarray(v[sl]) for k, v in c.rays.items()}
        eb = np.zeros(c.eb_shape(), np.float32)
        out = F.checker(sc, rays, np.ascontiguousarray(c.fresh_rng()[sl]), _plan(c, kind), launches, eb=eb)
        r = dict(map=out[0], rng=out[1], bounces=out[2], eb=eb)
        for v in r.values():
            v.setflags(write=False)
        _checked[key] = r
    return _checked[key]


def _trace(c, dev, launches=1, variant=0, kind="scene", footprint=True, rays=None, rng=None, fmap=None, scene=None,
           **kw):
    """``launches`` single launches into the grid, the window table and (``footprint``) the map of plan ``kind``:
    ``SimpleNamespace(map, rng, eb, table, stats, per)`` on the host.  ``footprint=False``: the same call without a
    map."""
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import (Scene, WindowPlan, new_stats, rays_to_device,
                                                                           trace_fullcolor, trace_single)
    wl = getattr(c, "wavelength", None)
    own = scene is None
    if own:
        scene = Scene.from_geometry(c.geom, c.luts, wavelength=wl)
    plan = WindowPlan()
    trace = trace_single if wl is not None else trace_fullcolor
    fp = _plan(c, kind)
    if fmap is None and footprint:
        fmap = fp.new_map(scene)
    table = plan.new_table(scene)
    eb = torch.zeros(scene.eb_shape(), dtype=torch.float32, device=dev)
    rays = rays_to_device(c.rays, dev) if rays is None else rays
    rng = torch.from_numpy(c.fresh_rng().view(np.int32)).to(dev) if rng is None else rng
    stats = new_stats(dev)
    per = torch.zeros(rng.numel(), dtype=torch.int32, device=dev)
    for _ in range(launches):
        trace(scene, rays, rng, eb, stats=stats, per_ray_bounces=per, variant=variant, windows=(plan, table),
              footprint=(fp, fmap) if footprint else None, **kw)
    torch.cuda.synchronize()
    out = SimpleNamespace(map=fmap.cpu().numpy() if footprint else None, rng=rng.cpu().numpy().view(np.uint32).copy(),
                          eb=eb.cpu().numpy(), table=table.cpu().numpy(), stats=stats.cpu().numpy().copy(),
                          per=per.cpu().numpy().view(np.uint32).copy())
    plan.close()
    if own:
        scene.close()
    return out


def _same_walk(a, b):
    np.testing.assert_array_equal(a.rng, b.rng)
    np.testing.assert_array_equal(a.per, b.per)
    np.testing.assert_array_equal(a.stats, b.stats)
    assert a.eb.tobytes() == b.eb.tobytes() and a.table.tobytes() == b.table.tobytes()


# 1. the fixtures and the small jobs, every variant, four launches into one map -------------------------------------

@pytest.mark.parametrize("variant", [1, 7, 9])
@pytest.mark.parametrize("name", FIXTURES + ["small", "c2s"])
def test_walk_and_map(dev, name, variant):
    c = _case(name)
    chk = checked(name, 4)
    got = _trace(c, dev, launches=4, variant=variant)
    assert got.map.dtype == np.int64 and got.map.shape == chk["map"].shape
    np.testing.assert_array_equal(got.map, chk["map"])
    np.testing.assert_array_equal(got.rng, chk["rng"])
    np.testing.assert_array_equal(got.per, chk["bounces"])
    np.testing.assert_array_equal(got.eb, chk["eb"])
    _same_walk(got, _trace(c, dev, launches=4, variant=variant, footprint=False))
    assert int(got.map[:, 0:6].sum()) == int(got.stats[STAT.interactions]) > 0
    assert got.map[:, 6].sum() > 0 and int(got.stats[STAT.bad_rays]) == 0


# 2. one cell for the whole plate (every add of a channel on one address) and a fine map; both forms of the sink -----

@pytest.mark.parametrize("variant", [1, 7])
@pytest.mark.parametrize("kind", ["one", "fine"])
def test_hot_cell_and_fine_map(dev, kind, variant):
    c = _case("small")
    chk = checked("small", 1, kind)
    got = {}
    for agg in (False, True):
        _lib.set_footprint_aggregate(agg)
        got[agg] = _trace(c, dev, variant=variant, kind=kind)
    _lib.set_footprint_aggregate(True)
    np.testing.assert_array_equal(got[True].map, got[False].map)
    np.testing.assert_array_equal(got[True].map, chk["map"])
    _same_walk(got[True], got[False])
    if kind == "one":   # the exact channel totals
        np.testing.assert_array_equal(got[True].map.reshape(-1, 9), checked("small")["map"].sum(axis=(2, 3)))
    assert int(got[True].map[:, 0:6].sum()) == int(got[True].stats[STAT.interactions])


# 3. refills: 13-ray work items on two workgroups ------------------------------------------------------------------

def test_refills(dev):
    c = _case("small_deep")
    chk = checked("small_deep")
    got = _trace(c, dev, variant=7, workgroups=2, debug=dict(chunk_rays=13))
    np.testing.assert_array_equal(got.map, chk["map"])
    np.testing.assert_array_equal(got.rng, chk["rng"])
    _same_walk(got, _trace(c, dev, variant=7, workgroups=2, debug=dict(chunk_rays=13), footprint=False))


# 4. abandoned rays: replayed past the draws already counted ---------------------------------------------------------

@pytest.mark.parametrize("debug, every", [(dict(cert_tol=1e-2), False), (dict(cert_tol=1e3, cert_tol32=1e3), True)])
def test_abandoned_rays_are_not_counted_twice(dev, debug, every):
    """A raised certification bound abandons rays in mid-walk (every ray at its first draw with ``cert_tol=1e3``): the
    exact lane re-traces them from the start and passes over the draws the Jones lane had counted."""
    c = _case("c2s")
    chk = checked("c2s")
    got = _trace(c, dev, variant=7, debug=debug)
    traced, replayed = c.N - int(got.stats[STAT.bad_rays]), int(got.stats[STAT.replayed])
    print(f"replayed {replayed} of {traced}")
    if every:
        assert replayed == traced > 256
    else:
        assert 0 < replayed < traced
    np.testing.assert_array_equal(got.map, chk["map"])
    np.testing.assert_array_equal(got.rng, chk["rng"])
    np.testing.assert_array_equal(got.per, chk["bounces"])
    _same_walk(got, _trace(c, dev, variant=7, debug=debug, footprint=False))


# 5. both locator forms, the single-wavelength kernel, an AMP profile, split batches ----------------------------------

@pytest.mark.parametrize("variant", [7, 9])
def test_byte_and_word_locator(dev, variant):
    c = _case("small")
    chk = checked("small")
    for byte in (True, False):
        _lib.set_byte_locator(byte)
        got = _trace(c, dev, variant=variant)
        np.testing.assert_array_equal(got.map, chk["map"])
        np.testing.assert_array_equal(got.rng, chk["rng"])
    _lib.set_byte_locator(True)


def test_single_wavelength(dev):
    c = _case("s1_532")
    assert getattr(c, "wavelength", None) is not None
    chk = checked("s1_532")
    for variant in (1, 7, 9):
        got = _trace(c, dev, variant=variant)
        assert got.map.shape[0] == 1
        np.testing.assert_array_equal(got.map, chk["map"])
        np.testing.assert_array_equal(got.rng, chk["rng"])


def test_amp_profile(dev):
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import Scene
    c = _case("small_amp")
    sc = Scene.from_geometry(c.geom, c.luts)
    assert sc.info()["nonunitary_blocks"] > 0
    sc.close()
    chk = checked("small_amp", 4)
    got = _trace(c, dev, launches=4, variant=7)
    np.testing.assert_array_equal(got.map, chk["map"])
    np.testing.assert_array_equal(got.rng, chk["rng"])
    assert int(got.map[:, 0:6].sum()) == int(got.stats[STAT.interactions]) > 0
    # ``small_amp`` delivers one ray in its four launches (every table of its profile is near-singular): channel 7
    # holds a single count.  The
    # delivering AMP case (tests/_kernel_table.py: the default LUTs with a non-unitary lut_fc2) makes the AMP kernels
    # count out-couplings inside the eyebox rectangle.
    name = KT.CASE_OF[(0, 1)]
    c = _case(name)
    sc = Scene.from_geometry(c.geom, c.luts)
    assert sc.info()["nonunitary_blocks"] > 0
    sc.close()
    chk = checked(name, 4)
    assert chk["map"][:, 7].sum() > 0 and chk["eb"].sum() > 0
    for variant in (7, 9):
        got = _trace(c, dev, launches=4, variant=variant)
        np.testing.assert_array_equal(got.map, chk["map"])
        np.testing.assert_array_equal(got.rng, chk["rng"])
        np.testing.assert_array_equal(got.eb, chk["eb"])
        assert int(got.map[:, 0:6].sum()) == int(got.stats[STAT.interactions]) > 0


@pytest.mark.parametrize("variant", [1, 7])
def test_a_batch_split_at_ray_37(dev, variant):
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import Scene, rays_to_device
    c = _case("c1_rgb")
    chk = checked("c1_rgb")
    scene = Scene.from_geometry(c.geom, c.luts)
    fmap = _plan(c).new_map(scene)
    full = rays_to_device(c.rays, dev)
    rng_all = torch.from_numpy(c.fresh_rng().view(np.int32)).to(dev)
    got_rng = []
    for lo, hi in ((0, 37), (37, c.N)):
        rays = {k: v[lo:hi].contiguous() for k, v in full.items()}
        r = _trace(c, dev, variant=variant, rays=rays, rng=rng_all[lo:hi].contiguous(), fmap=fmap, scene=scene,
                   gid_offset=lo)
        got_rng.append(r.rng)
    got = fmap.cpu().numpy()
    scene.close()
    np.testing.assert_array_equal(got, chk["map"])
    np.testing.assert_array_equal(np.concatenate(got_rng), chk["rng"])


def test_two_gid_blocks_shards_add_up(dev):
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.distributed import make_shard
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import init_rays
    c = _case("c1_rgb")
    chk = checked("c1_rgb")
    parts = []
    for r in range(2):
        shard = make_shard(c.nx, c.ny, len(c.lambdas), c.R, 2, r)
        rays, rng = init_rays(c.f["points"], c.nx, c.ny, c.lambdas, c.R, block_list=shard.blocks, device=dev)
        gb = torch.from_numpy(shard.gid.block_gid).to(dev)
        m = _trace(c, dev, variant=7, rays=rays, rng=rng, n_rays=rng.numel(), gid_blocks=gb, gid_block_rays=c.R).map
        assert m.sum() > 0
        parts.append(m)
    np.testing.assert_array_equal(parts[0] + parts[1], chk["map"])


# 6. a plan smaller than the plate -------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", [1, 7])
def test_a_plan_smaller_than_the_plate(dev, variant):
    c = _case("small")
    chk, whole = checked("small", 1, "cut"), checked("small")
    got = _trace(c, dev, variant=variant, kind="cut")
    np.testing.assert_array_equal(got.map, chk["map"])
    assert 0 < got.map.sum() < whole["map"].sum()
    np.testing.assert_array_equal(got.map, whole["map"][:, :, 10:30, 20:50])   # the rest is unchanged
    np.testing.assert_array_equal(got.rng, chk["rng"])


# 7. argument errors -----------------------------------------------------------------------------------------------------

def test_argument_errors(dev):
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import (Scene, TraceChain, WindowPlan, _debug_opts,
                                                                           rays_to_device, trace_fullcolor)
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd._lib import load, ops
    c = _case("c1_rgb")
    scene, plan = Scene.from_geometry(c.geom, c.luts), WindowPlan()
    rays = rays_to_device(c.rays, dev)
    rng = torch.from_numpy(c.fresh_rng().view(np.int32)).to(dev)
    before = rng.clone()
    fp = _plan(c)
    fmap = fp.new_map(scene)
    grid = torch.zeros(c.eb_shape(), dtype=torch.float32, device=dev)
    table = plan.new_table(scene)
    go = lambda **kw: trace_fullcolor(scene, rays, rng, grid, variant=7, footprint=(fp, fmap), **kw)
    with pytest.raises(ValueError, match="num_iter"):
        go(num_iter=2)
    with pytest.raises(ValueError, match="fate"):
        go(fate=torch.zeros(c.N, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="replicas"):
        go(windows=(plan, plan.new_table(scene, replicas=4)), replicas=4)
    with pytest.raises(ValueError, match="expected"):
        trace_fullcolor(scene, rays, rng, None, windows=(plan, table), expected=True, footprint=(fp, fmap))
    with pytest.raises(ValueError, match="shape"):
        trace_fullcolor(scene, rays, rng, grid, footprint=(_plan(c, "cut"), fmap))
    with pytest.raises(ValueError, match="chain"):
        TraceChain(scene, rays, rng, grid, footprint=(fp, fmap))

    # the operator and the C entry point themselves
    def op(m=fmap, num_iter=1, debug=0, nx_cells=None, cell_x=None):
        return ops().trace_footprint(scene.handle.value, rays["x"], rays["y"], rays["m"], rays["n"], rays["lmd_num"],
                                     rays["te"], rays["tm"], rays["delta_phase"], rng, grid, None, None, c.N, 0, 0, 0, 7,
                                     0, None, num_iter, None, 0, debug, 0.0, 0, None, fp.x0, fp.y0,
                                     fp.cell_x if cell_x is None else cell_x, fp.cell_y,
                                     fp.nx_cells if nx_cells is None else nx_cells, fp.ny_cells, m)
    assert op(num_iter=2) == 1                                                     # WGRT_ERR_INVALID_ARGUMENT
    assert op(nx_cells=0) == 1 and op(nx_cells=4097) == 1 and op(cell_x=0.0) == 1 and op(cell_x=float("nan")) == 1
    tl = torch.zeros(8 * 64, dtype=torch.int64, device=dev)
    dbg = _debug_opts(dict(timeline=tl))
    assert op(debug=ctypes.addressof(dbg)) == 4                                    # WGRT_ERR_UNSUPPORTED
    with pytest.raises(RuntimeError, match="int64"):
        op(fmap.to(torch.int32))
    with pytest.raises(RuntimeError, match="must be on"):
        op(fmap.cpu())
    with pytest.raises(RuntimeError, match="contiguous"):
        op(fmap[:, :, :, :-1])
    torch.cuda.synchronize()
    assert torch.equal(rng, before) and not fmap.any() and not grid.any() and not tl.any()   # nothing was launched

    # map == NULL: the windows launch, bit for bit
    L = load()
    cols = _lib.Rays(**{k: ctypes.c_void_p(rays[k].data_ptr()) for k in ("x", "y", "m", "n", "lmd_num", "te", "tm",
                                                                          "delta_phase")})
    opts = _lib.LaunchOpts()
    opts.variant = 7
    st = torch.zeros(_lib.STATS_LEN, dtype=torch.int64, device=dev)
    assert L.wgrt_trace_footprint(scene.handle, ctypes.byref(cols), c.N, 0, rng.data_ptr(), grid.data_ptr(),
                                  st.data_ptr(), None, None, ctypes.byref(opts), plan.handle, table.data_ptr(), None,
                                  None) == 0
    rng2, grid2, table2, st2 = before.clone(), torch.zeros_like(grid), torch.zeros_like(table), torch.zeros_like(st)
    assert L.wgrt_trace_windows(scene.handle, ctypes.byref(cols), c.N, 0, rng2.data_ptr(), grid2.data_ptr(),
                                st2.data_ptr(), None, None, ctypes.byref(opts), plan.handle, table2.data_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(rng, rng2) and torch.equal(grid, grid2) and torch.equal(table, table2) and torch.equal(st, st2)
    assert grid.sum() > 0 and not fmap.any()
    # a map and no plan
    assert L.wgrt_trace_footprint(scene.handle, ctypes.byref(cols), c.N, 0, rng.data_ptr(), grid.data_ptr(), None, None,
                                  None, ctypes.byref(opts), None, None, None, fmap.data_ptr()) == 1
    plan.close()
    scene.close()


# 8. the driver ------------------------------------------------------------------------------------------------------------
# the small job of tests/test_gpu_window_sink.py ("deep" LUT profile)

NX, NY, R, STEPS = 5, 4, 256, 2
_runs = {}


def _run(footprint, **kw):
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.gpu_ray_tracing_pro_fullColor import run
    from tests import _dist
    pts = _dist.small_job(NX, NY, R, 3, 6, "deep")[2]
    return run(NX, NY, R, STEPS, lut_seed=3, lut_profile="deep", points=pts, verbose=False, eyebox="windows",
               evaluate_on="device", footprint=footprint, **kw)


def _run_once(footprint):
    if footprint not in _runs:
        _runs[footprint] = _run(footprint)
    return _runs[footprint]


def test_driver_footprint(dev):
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import FootprintPlan
    from oracle import OracleScene
    from tests import _dist
    got, plain = _run_once((64, 96)), _run_once(None)
    assert set(got) - set(plain) == {"footprint", "footprint_plan"}
    for k in plain:   # everything returned before, bit for bit (the timings aside)
        if k in ("gpu_seconds", "post_seconds"):
            continue
        a, b = got[k], plain[k]
        if isinstance(a, np.ndarray):
            assert a.tobytes() == b.tobytes(), k
        else:
            assert a == b or (isinstance(a, float) and float(a).hex() == float(b).hex()), k
    m = got["footprint"]
    assert m.dtype == np.int64 and m.shape == (3, 9, 64, 96)
    # the checker on the driver's batch
    geom, luts, pts = _dist.small_job(NX, NY, R, 3, 6, "deep")
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.rays import build_rays, rng_seeds
    rays = build_rays(pts, NX, NY, (0, 1, 2), R)
    fp = FootprintPlan.for_scene(geom, cells=(64, 96))
    assert got["footprint_plan"] == fp.as_dict()
    want = F.checker(OracleScene.from_geometry(geom, luts), rays, rng_seeds(rays["x"].shape[0]), fp, STEPS)
    np.testing.assert_array_equal(m, want[0])
    np.testing.assert_array_equal(got["rng_states"], want[1])
    for bad in (dict(budget=True), dict(error_bars=4), dict(estimator="expected")):
        with pytest.raises(ValueError, match="footprint"):
            _run((64, 96), **bad)
    with pytest.raises(ValueError, match="footprint"):
        _run((64, 5000))


def _driver_worker(rank, world, outdir):
    torch.cuda.set_device(torch.device("cuda", 0))
    res = _run((64, 96))
    np.save(f"{outdir}/rng{rank}.npy", res["rng_states"])
    if rank != 0:
        assert "footprint" not in res
        return
    np.save(f"{outdir}/footprint.npy", res["footprint"])


def test_driver_footprint_in_two_ranks(dev, tmp_path):
    """Two ranks on the one GPU over gloo: the ranks' maps are integer counts and add exactly."""
    from tests import _dist
    _dist.spawn(_driver_worker, 2, str(tmp_path))
    one = _run_once((64, 96))
    np.testing.assert_array_equal(np.load(tmp_path / "footprint.npy"), one["footprint"])
