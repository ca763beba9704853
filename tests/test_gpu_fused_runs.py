"""Fused launches whose lanes keep a ray for a run of chained traces (``wgrt_debug_set_fused_run``; DESIGN.md §4.3,
csrc/wgrt_items.h): whatever the run length, a fused launch leaves what ``num_iter`` chained oracle launches leave.

Shapes: ``tests/test_gpu_chain.py``'s 5 x 4 FoVs x 3 wavelengths x 100 = 6,000 rays on two workgroups (8 waves, 512
lanes), so every lane restarts and is refilled many times; the kernel table's four small shapes for the
single-wavelength and AMP instantiations.  The oracle's nine chained traces are computed once and shared.

Tolerance: none -- RNG states, grid, bounces, interactions and eyebox hits are compared exactly, and no hand-off is
given up unless the test says so."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gpu_ray_tracing_for_waveguide_based_ar_display_amd import _lib  # noqa: E402
from gpu_ray_tracing_for_waveguide_based_ar_display_amd._lib import STAT  # noqa: E402
from tests.test_gpu_chain import SMALL, _assert_oracle, _Run, _want  # noqa: E402
from tests.test_gpu_parity import _TABLE_CFG, _config, _trace_fused  # noqa: E402

STEPS = 9


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


@pytest.fixture(autouse=True)
def _switches():
    _lib.load().wgrt_debug_set_auto_order(0)
    _lib.set_fused_run(0)
    yield
    _lib.set_fused_run(0)
    _lib.load().wgrt_debug_set_auto_order(1)


def _fused(c, dev, num_iter, run, **kw):
    """One fused launch of ``num_iter`` traces with runs of ``run`` (0: the automatic rule) on a fresh scene."""
    _lib.set_fused_run(run)
    r = _Run(c, dev, **kw)
    got = r.plain(1, num_iter=num_iter).out()
    r.close()
    return got


@pytest.mark.parametrize("variant", [7, 9])
@pytest.mark.parametrize("num_iter", [2, 3, 5, 8, 9])
@pytest.mark.parametrize("run", [1, 2, 4, 8])
def test_run_lengths_match_oracle(dev, run, num_iter, variant):
    """num_iter below, at and above the run length, and a short last run."""
    c, want = _want("small9", SMALL, steps=STEPS)
    got = _fused(c, dev, num_iter, run, variant=variant)
    _assert_oracle(got, want[num_iter - 1])
    assert int(got["stats"][STAT.bad_rays]) == 0 and int(got["stats"][STAT.replayed]) <= 2


@pytest.mark.parametrize("chunk", [13, 64])
def test_small_items(dev, chunk):
    """Items smaller than a wave: the staged buffers are overwritten while lanes still restart from their private
    slots (a ray stays for four traces; a 13-ray item's buffer is reused two items later)."""
    c, want = _want("small9", SMALL, steps=STEPS)
    got = _fused(c, dev, 6, 4, debug=dict(chunk_rays=chunk))
    _assert_oracle(got, want[5])


@pytest.mark.parametrize("debug,every", [(dict(cert_tol=1e-4), False), (dict(cert_tol=1e-2), False),
                                         (dict(cert_tol=1e3, cert_tol32=1e3), True)])
def test_forced_replays(dev, debug, every):
    """Rays abandoned inside a run are not restarted: the epilogue finishes their traces, later runs skip them, and
    the launch counts each once -- as many as with a hand-off after every trace."""
    c, want = _want("small9", SMALL, steps=STEPS)
    one = _fused(c, dev, 6, 1, debug=debug)
    got = _fused(c, dev, 6, 4, debug=debug)
    for g in (one, got):
        _assert_oracle(g, want[5])
    assert int(got["stats"][STAT.replayed]) == int(one["stats"][STAT.replayed]) > 0
    if every:
        assert int(got["stats"][STAT.replayed]) == c.N
    else:
        # some rays are abandoned in a trace that is not the first of its run: a launch of the first run's four traces
        # abandons more rays than a launch of the first trace alone (counted by the launches themselves: which
        # decisions the Jones-vector lane cannot certify is not something the exact oracle knows)
        first = _fused(c, dev, 1, 1, debug=debug)
        four = _fused(c, dev, 4, 4, debug=debug)
        _assert_oracle(four, want[3])
        assert int(four["stats"][STAT.replayed]) > int(first["stats"][STAT.replayed]) > 0


@pytest.mark.parametrize("run", [1, 4])
def test_bad_rays_count_once_per_trace(dev, run):
    """Rays whose FoV index is out of range are not traced and count once per trace the launch covers."""
    c, _ = _want("small9", SMALL, steps=STEPS)
    from oracle import OracleScene
    b = _config(**SMALL)
    bad = np.array([0, 63, 64, 1000, 4097, b.N - 1])
    b.rays = {k: v.copy() for k, v in c.rays.items()}
    b.rays["m"][bad] = 99
    ok = np.ones(b.N, bool)
    ok[bad] = False
    got = _fused(b, dev, 5, run)
    sc = OracleScene.from_geometry(c.geom, c.luts)
    good = {k: v[ok] for k, v in c.rays.items()}
    rng, eb, total = c.fresh_rng()[ok], np.zeros(c.eb_shape(), np.float32), 0
    for _ in range(5):
        total += sc.trace(good, rng, eb)[0]
    assert int(got["stats"][STAT.bad_rays]) == bad.size * 5
    np.testing.assert_array_equal(got["rng"][ok], rng)
    np.testing.assert_array_equal(got["rng"][bad], c.fresh_rng()[bad])   # never traced
    np.testing.assert_array_equal(got["eb"], eb)
    assert int(got["stats"][STAT.bounces]) == total and int(got["stats"][STAT.handoff_giveups]) == 0


def test_epochs_with_changing_run_length(dev):
    """``test_fused_iterations_repeat_epochs``'s sequence of calls on one scene and stream with the run length
    changing between them: the granules carry stale tags of other epochs and other run boundaries."""
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import (Scene, new_stats, rays_to_device,
                                                                           trace_fullcolor)
    from oracle import OracleScene
    c = _config(5, 5, [0, 1, 2], 256)
    scene = Scene.from_geometry(c.geom, c.luts)
    rays = rays_to_device(c.rays, dev)
    rng = torch.from_numpy(c.fresh_rng().view(np.int32)).to(dev)
    eb = torch.zeros(c.eb_shape(), dtype=torch.float32, device=dev)
    sc = OracleScene.from_geometry(c.geom, c.luts)
    o_rng = c.fresh_rng()
    o_eb = np.zeros(c.eb_shape(), np.float32)
    for num_iter, run in ((3, 2), (3, 1), (1, 4), (2, 2), (5, 4), (1, 1), (4, 2), (5, 1), (5, 8)):
        _lib.set_fused_run(run)
        stats = new_stats(dev)
        trace_fullcolor(scene, rays, rng, eb, stats=stats, variant=7, num_iter=num_iter)
        torch.cuda.synchronize()
        tot = sum(sc.trace(c.rays, o_rng, o_eb)[0] for _ in range(num_iter))
        np.testing.assert_array_equal(rng.cpu().numpy().view(np.uint32), o_rng, err_msg=f"num_iter {num_iter} run {run}")
        np.testing.assert_array_equal(eb.cpu().numpy(), o_eb, err_msg=f"num_iter {num_iter} run {run}")
        assert int(stats[STAT.bounces]) == tot and int(stats[STAT.handoff_giveups]) == 0
    scene.close()


def test_handoff_bound(dev):
    """A hand-off bound of one tick with runs of two: the traces that would have waited are given up, counted, and
    ``check_stats`` raises; the default bound gives nothing up.  Under the automatic rule a call with a debug bound
    runs with a hand-off after every trace."""
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import WgrtError, check_stats
    c, want = _want("small9", SMALL, steps=STEPS)
    got = _fused(c, dev, 6, 2, debug=dict(handoff_wait_ticks=1))
    assert int(got["stats"][STAT.handoff_giveups]) > 0
    with pytest.raises(WgrtError, match="hand-off"):
        check_stats(torch.from_numpy(got["stats"]))
    got = _fused(c, dev, 6, 2)
    _assert_oracle(got, want[5])
    check_stats(torch.from_numpy(got["stats"]))
    _lib.set_fused_run(0)
    assert _lib.fused_run(8) == 2 and _lib.fused_run(8, handoff_bound=True) == 1
    got = _fused(c, dev, 8, 0, debug=dict(handoff_wait_ticks=1))
    assert int(got["stats"][STAT.handoff_giveups]) > 0


_table_oracle5 = {}


@pytest.mark.parametrize("amp", [False, True])
@pytest.mark.parametrize("single", [False, True])
@pytest.mark.parametrize("variant", [7, 9])
def test_single_wavelength_and_amp_kernels(dev, variant, single, amp):
    """The fused SINGLE and AMP instantiations of both cell widths with runs of four over five traces."""
    from oracle import OracleScene
    if (single, amp) not in _table_oracle5:
        c = _config(**_TABLE_CFG[(single, amp)])
        sc = OracleScene.from_geometry(c.geom, c.luts, wavelength=c.wavelength)
        rng, eb, total = c.fresh_rng(), np.zeros(c.eb_shape(), np.float32), 0
        for _ in range(5):
            total += sc.trace(c.rays, rng, eb)[0]
        _table_oracle5[(single, amp)] = (c, rng, eb, total)
    c, o_rng, o_eb, total = _table_oracle5[(single, amp)]
    _lib.set_fused_run(4)
    rng, eb, stats = _trace_fused(c, dev, 5, variant)
    np.testing.assert_array_equal(rng, o_rng)
    np.testing.assert_array_equal(eb, o_eb)
    assert int(stats[STAT.bounces]) == total
    assert int(stats[STAT.eyebox_hits]) == int(round(float(o_eb.sum())))
    assert int(stats[STAT.handoff_giveups]) == 0


def test_window_sink_without_a_grid(dev):
    """A window-table sink with ``matrix_EB=None``: five traces in runs of four leave the table five plain launches
    leave."""
    c, want = _want("small9", SMALL, steps=STEPS)
    _lib.set_fused_run(4)
    a, b = _Run(c, dev, windows=True), _Run(c, dev, windows=True)
    a.eb = None
    a.plain(1, num_iter=5)
    torch.cuda.synchronize()
    got = dict(rng=a.rng.cpu().numpy().view(np.uint32).copy(), stats=a.stats.cpu().numpy().copy(),
               table=a.table.cpu().numpy().copy())
    ref = b.plain(5).out()
    a.close()
    b.close()
    np.testing.assert_array_equal(got["rng"], want[4]["rng"])
    assert got["table"].sum() > 0
    np.testing.assert_array_equal(got["table"], ref["table"])
    np.testing.assert_array_equal(got["stats"], ref["stats"])


def test_gathered_chain_under_the_automatic_rule(dev):
    """Nine steps held and released as one fused launch of nine: the automatic rule's runs of two."""
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import TraceChain
    c, want = _want("small9", SMALL, steps=STEPS)
    assert _lib.fused_run(STEPS) == 2
    r = _Run(c, dev)
    with TraceChain(r.scene, r.rays, r.rng, r.eb, gather=True, hold=True, **r.kw) as ch:
        for _ in range(STEPS):
            ch.step()
        rep = ch.report()
    got = r.out()
    r.close()
    assert rep["launches"] == 0 and rep["pending"] == STEPS
    _assert_oracle(got, want[STEPS - 1])
