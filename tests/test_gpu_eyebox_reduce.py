"""``wgrt_eyebox_window_sums`` (csrc/wgrt_eyebox.hip) on the GPU against its float64 numpy statement
(``AR_system_evaluation_functions.eyebox_window_sums`` on a host array, tests/test_eyebox_reduce.py), the
driver's ``eyebox="device"`` mode against its host mode, and ``distributed.EyeboxReduce`` with the HIP
kernel in every rank (all ranks on cuda:0 over gloo, as tests/test_gpu_distributed.py).

Counts are integers, so every comparison of an integer-valued grid is bit for bit; only the test on
non-integer input has a tolerance (the summation order differs)."""
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from gpu_ray_tracing_for_waveguide_based_ar_display_amd import AR_system_evaluation_functions as E  # noqa: E402
from tests import _dist  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPE = (3, 2, 4, 80, 120)
INVALID_ARGUMENT = 1   # WGRT_ERR_INVALID_ARGUMENT (include/wgrt.h)
SLABS = np.array([5, 0, 23, 5, -1, 24, 7], dtype=np.int64)   # out of order, a duplicate, -1 and n_slabs


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _gpu(eb, **kw):
    """The kernel's result for host array ``eb`` (and keyword arguments of eyebox_window_sums), on the host."""
    out = E.eyebox_window_sums(torch.from_numpy(eb).to(_dev()), **kw)
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float64
    return out.cpu().numpy()


def _counts(seed, shape=SHAPE):
    return np.random.default_rng(seed).integers(0, 5, size=shape).astype(np.float32)


def _structured_bins():
    """Bins where an indexing slip of the window loop would show: see test_single_hits_at_edges."""
    m = E.pupil_mask()
    lo = [int(np.nonzero(r)[0][0]) for r in m]
    hi = [int(np.nonzero(r)[0][-1]) + 1 for r in m]
    bins = [(0, 0), (0, 119), (79, 0), (79, 119)]
    bins += [(y, x) for y in (77, 78) for x in (0, 60, 113, 114, 119)] + [(y, x) for y in (0, 40) for x in (113, 114)]
    for iy, ix in [(0, 0), (3, 4), (6, 7), (2, 5), (6, 0), (0, 7)]:
        y0, x0 = 8 * iy, 12 * ix
        bins += [(y0, x0 + 15), (y0 + 29, x0 + 15), (y0 + 15, x0), (y0 + 15, x0 + 29)]    # first / last row, column
        bins += [(y0, x0), (y0, x0 + 29), (y0 + 29, x0), (y0 + 29, x0 + 29)]              # mask corners (excluded)
        for r in (0, 1, 5, 14, 15, 28, 29):                                                # ends of the row runs
            bins += [(y0 + r, x0 + c) for c in (lo[r] - 1, lo[r], hi[r] - 1, hi[r]) if 0 <= x0 + c < 120]
    return sorted(set(bins))


@functools.lru_cache(maxsize=None)
def _structured():
    bins = _structured_bins()
    rng = np.random.default_rng(8)
    n = 256
    assert 180 <= len(bins) <= n
    bins = bins + [(int(rng.integers(80)), int(rng.integers(120))) for _ in range(n - len(bins))]
    eb = np.zeros((n, 80, 120), np.float32)
    for s, (y, x) in enumerate(bins):
        eb[s, y, x] = 1.0
    return eb, E.eyebox_window_sums(eb)


def test_random_counts_bit_for_bit():
    eb = _counts(0)
    got = _gpu(eb)
    assert got.shape == (24, 57)
    np.testing.assert_array_equal(got, E.eyebox_window_sums(eb))


def test_single_hits_at_edges():
    """256 slabs with a single 1.0 each: the grid's corners, rows 77 / 78 and columns 113 / 114 (the last
    bins any window covers and the first none does), the first and last row and column of several windows,
    the mask's corners (outside the pupil) and both ends of the pupil's row runs, one bin inside and one
    outside."""
    eb, want = _structured()
    got = _gpu(eb)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got[:, 0], 1.0)
    assert (got[:, 1:].sum(axis=1) == 0).any() and (got[:, 1:].sum(axis=1) > 1).any()


def test_slab_list_and_empty():
    eb = _counts(1)
    want = E.eyebox_window_sums(eb, slabs=SLABS)
    np.testing.assert_array_equal(_gpu(eb, slabs=SLABS), want)
    np.testing.assert_array_equal(_gpu(eb, slabs=torch.from_numpy(SLABS).to(_dev())), want)
    assert not want[4].any() and not want[5].any()
    assert _gpu(eb, slabs=np.zeros(0, np.int64)).shape == (0, 57)
    L = _lib().load()   # n == 0: WGRT_OK without a launch, whatever the pointers
    assert L.wgrt_eyebox_window_sums(None, 24, None, 0, None, 30, 8, 12, None, None) == 0


@pytest.mark.parametrize("ms,steps", [(80, (1, 1)), (1, (8, 12)), (5, (3, 7))])
def test_non_default_mask_and_steps(ms, steps):
    eb = _counts(2)
    if ms == 5:   # a general mask (non-unit weights, a zero inside a run, an empty row): the multiply path
        mask = np.array([[0, 1, 2, 0, 0], [.5, 0, 1, 1, 0], [1, 1, 1, 1, 1], [0, 0, 0, 0, 0], [0, 0, 0, 3, 1]], np.float32)
    else:
        mask = np.ones((ms, ms), np.float32)
    kw = dict(mask=mask, step_y=steps[0], step_x=steps[1])
    want = E.eyebox_window_sums(eb, **kw)
    assert want.shape[1] == {80: 42, 1: 101, 5: 443}[ms]
    np.testing.assert_array_equal(_gpu(eb, **kw), want)


def test_non_integer_input_and_determinism():
    """Uniform [0, 1) float32: the kernel and numpy add the same non-negative float64 terms (at most 900 per
    window) in different orders, each order within 899 * 2^-53 relative of the exact sum.  The slab total
    (9,600 terms) is held to the same 900 * 2^-53."""
    eb = np.random.default_rng(3).random(SHAPE, dtype=np.float32)
    want = E.eyebox_window_sums(eb)
    d = torch.from_numpy(eb).to(_dev())
    a = E.eyebox_window_sums(d).cpu().numpy()
    b = E.eyebox_window_sums(d).cpu().numpy()
    print(f"max relative difference {np.max(np.abs(a - want) / want):.3e}")
    np.testing.assert_allclose(a, want, rtol=900 * 2.0 ** -53, atol=0)
    assert a.tobytes() == b.tobytes()   # two calls: identical bits


def _lib():
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd import _lib
    return _lib


def _raw_call(eb, slabs, n, mask, ms, step_y, step_x, out_ptr):
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import _stream_handle
    return _lib().load().wgrt_eyebox_window_sums(eb.data_ptr(), eb.numel() // 9600,
                                                 slabs.data_ptr() if slabs is not None else None, n, mask.data_ptr(),
                                                 ms, step_y, step_x, out_ptr, _stream_handle(eb.device))


def test_neighbouring_memory_untouched():
    dev = _dev()
    eb = _counts(4)
    d, mask = torch.from_numpy(eb).to(dev), torch.from_numpy(E.pupil_mask()).to(dev)
    slabs = torch.from_numpy(SLABS).to(dev)
    n, W, pad = len(SLABS), 57, 64
    buf = torch.full((pad + n * W + pad,), -7.25, dtype=torch.float64, device=dev)
    assert _raw_call(d, slabs, n, mask, 30, 8, 12, buf.data_ptr() + 8 * pad) == 0
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert (h[:pad] == -7.25).all() and (h[pad + n * W:] == -7.25).all()
    np.testing.assert_array_equal(h[pad:pad + n * W].reshape(n, W), E.eyebox_window_sums(eb, slabs=SLABS))


def test_c3_shape_sparse_counts():
    """C3's grid (3 x 21 x 21 = 1323 slabs, 51 MB: more workgroups than the chip holds at once)."""
    rng = np.random.default_rng(6)
    shape = (3, 21, 21, 80, 120)
    eb = np.where(rng.random(shape, dtype=np.float32) < 0.02, rng.integers(1, 40, size=shape), 0).astype(np.float32)
    np.testing.assert_array_equal(_gpu(eb), E.eyebox_window_sums(eb))


def test_argument_validation():
    dev = _dev()
    d = torch.zeros(SHAPE, dtype=torch.float32, device=dev)
    mask = torch.ones((80, 80), dtype=torch.float32, device=dev)
    out = torch.full((24 * 57,), -1.0, dtype=torch.float64, device=dev)
    L = _lib().load()
    for ms, sy, sx, ptr in [(0, 8, 12, out.data_ptr()), (81, 8, 12, out.data_ptr()), (30, 0, 12, out.data_ptr()),
                            (30, 8, 0, out.data_ptr()), (30, 8, 12, None)]:
        assert _raw_call(d, None, 24, mask, ms, sy, sx, ptr) == INVALID_ARGUMENT
        assert L.wgrt_last_error()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -1.0).all()   # nothing was launched
    # the Python layer refuses device tensors the kernel cannot take (no silent fall-back)
    with pytest.raises(ValueError):
        E.eyebox_window_sums(d.double())
    with pytest.raises(ValueError):
        E.eyebox_window_sums(d.transpose(1, 2)[..., :80, :120])
    with pytest.raises(ValueError):
        E.eyebox_window_sums(d[..., :79, :])


# --- the driver -------------------------------------------------------------------------------------------

NX, NY, LAMBDAS, R, STEPS = 5, 4, [0, 1, 2], 256, 2


def _inputs():
    return _dist.small_job(NX, NY, R, lut_seed=3, point_seed=6, lut_profile="deep")


def test_driver_device_mode_equals_host_mode():
    _dev()
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.gpu_ray_tracing_pro_fullColor import run
    _, _, pts = _inputs()
    kw = dict(lut_seed=3, lut_profile="deep", points=pts, evaluate=True, verbose=False)
    host = run(NX, NY, R, STEPS, **kw)
    dev = run(NX, NY, R, STEPS, eyebox="device", **kw)
    assert "matrix_EB" not in dev and host["matrix_EB"].sum() > 0
    assert dev["A"].dtype == host["A"].dtype and dev["A"].tobytes() == host["A"].tobytes()
    assert dev["efficiency"] == host["efficiency"]
    np.testing.assert_array_equal(dev["rng_states"], host["rng_states"])
    sums = E.eyebox_window_sums(host["matrix_EB"])
    want = E.evaluation_from_perceive(E.perceive_from_window_sums(sums, host["matrix_EB"].shape, R * STEPS))
    assert (dev["delta_e"], dev["U_fov"], dev["U_EB"]) == tuple(float(v) for v in want[:3])
    np.testing.assert_array_equal(dev["output_image"], want[3])
    kept = run(NX, NY, R, STEPS, eyebox="device", keep_grid=True, **kw)
    np.testing.assert_array_equal(kept["matrix_EB"], host["matrix_EB"])
    with pytest.raises(ValueError):
        run(NX, NY, R, STEPS, eyebox="gpu", **kw)


# --- multi-rank: every rank traces its shard on cuda:0 and the window sums are sum-reduced over gloo --------

def _worker(rank, world, outdir):
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.distributed import EyeboxReduce, rank_blocks
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.gpu_ray_tracing_pro_fullColor import _set_up, _trace

    torch.cuda.set_device(torch.device("cuda", 0))
    nb = NX * NY * len(LAMBDAS)
    reduce = EyeboxReduce([rank_blocks(nb, world, r, "interleaved", len(LAMBDAS)) for r in range(world)],
                          NX, NY, LAMBDAS, len(LAMBDAS))
    # the driver's own set-up and trace stages: this rank's shard, STEPS separate launches, counters checked
    with _set_up(NX, NY, R, STEPS, LAMBDAS, None, 3, "deep", None, _inputs()[2], False) as job:
        _trace(job, 0, False)
        sums = reduce(job.eb)
        torch.cuda.synchronize()
    if rank == 0:
        assert sums.is_cuda
        np.save(os.path.join(outdir, "sums.npy"), sums.cpu().numpy())


@functools.lru_cache(maxsize=None)
def _oracle_sums():
    """Window sums of the oracle's grid after STEPS chained traces of the whole batch."""
    from oracle import OracleScene
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.distributed import shard_rays_host
    geom, luts, pts = _inputs()
    rays, rng = shard_rays_host(pts, NX, NY, LAMBDAS, R, np.arange(NX * NY * len(LAMBDAS)))
    sc = OracleScene.from_geometry(geom, luts)
    eb = np.zeros(sc.eb_shape(), np.float32)
    for _ in range(STEPS):
        sc.trace(rays, rng, eb, threads=8)
    assert eb.sum() > 0
    return E.eyebox_window_sums(eb)


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_reduce_equals_oracle_window_sums(tmp_path, world):
    _dev()
    _dist.spawn(_worker, world, str(tmp_path))
    got = np.load(tmp_path / "sums.npy")
    assert got.dtype == np.float64 and got.shape == (3 * NY * NX, 57)
    np.testing.assert_array_equal(got, _oracle_sums())
