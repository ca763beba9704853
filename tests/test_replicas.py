"""Monte-Carlo error bars without a GPU: the host fold of the replica window tables
(``wgrt_window_replicas_fold_host``), the jackknife estimators of ``AR_system_evaluation_functions`` and the
argument checks of ``run(error_bars=B)``.

Tolerances: none for the fold (fixed order of the additions: byte equality); 1e-12 relative where two algebraically
equal standard errors are compared, the float64 rounding of sums of at most 64 terms, not a measured number."""
import numpy as np
import pytest

from gpu_ray_tracing_for_waveguide_based_ar_display_amd import AR_system_evaluation_functions as E
from gpu_ray_tracing_for_waveguide_based_ar_display_amd import _lib
from tests._fixtures import GoldenCase

INVALID_ARGUMENT = 1   # WGRT_ERR_INVALID_ARGUMENT (include/wgrt.h)


def _fold_host(t):
    """``wgrt_window_replicas_fold_host`` on ``t [B, n]`` through ctypes: (status, out [1 + B, n])."""
    L = _lib.load()
    t = np.ascontiguousarray(t, dtype=np.float64)
    out = np.full((1 + t.shape[0], t.shape[1]), np.nan)
    st = L.wgrt_window_replicas_fold_host(t.ctypes.data, t.shape[0], t.shape[1], out.ctypes.data)
    return st, out


def _fold_loop(t):
    """The contract as an explicit loop over b: the sum in ascending b from 0.0, then sum - reps[b]."""
    B, n = t.shape
    out = np.empty((1 + B, n))
    s = np.zeros(n)
    for b in range(B):
        s = s + t[b]
    out[0] = s
    for b in range(B):
        out[1 + b] = s - t[b]
    return out


@pytest.mark.parametrize("B", [2, 5, 64])
def test_fold_host_integer_tables(B):
    n = 3 * 57 + 2   # not a multiple of 4
    t = np.random.default_rng(B).integers(0, 1 << 20, (B, n)).astype(np.float64)
    st, out = _fold_host(t)
    assert st == 0
    assert out.tobytes() == _fold_loop(t).tobytes()
    # integer counts come out as exact integers
    assert np.array_equal(out[0], t.astype(np.int64).sum(0)) and np.array_equal(out, np.rint(out))


def test_fold_host_fixed_order():
    """Non-integer entries of very different magnitude: any other order of the additions gives other bits."""
    rng = np.random.default_rng(7)
    t = rng.standard_normal((9, 57 + 3)) * 10.0 ** rng.integers(-8, 9, (9, 57 + 3))
    st, out = _fold_host(t)
    assert st == 0
    assert out.tobytes() == _fold_loop(t).tobytes()
    assert out[0].tobytes() != _fold_loop(t[::-1])[0].tobytes()   # (the case does tell the orders apart)


def test_fold_host_errors_and_empty():
    L = _lib.load()
    for B in (1, 65, 0, -3):
        t = np.zeros((max(B, 1), 8))
        out = np.zeros((max(B, 1) + 1, 8))
        assert L.wgrt_window_replicas_fold_host(t.ctypes.data, B, 8, out.ctypes.data) == INVALID_ARGUMENT
    assert L.wgrt_window_replicas_fold_host(None, 4, 0, None) == 0   # n == 0: nothing to do
    assert L.wgrt_window_replicas_fold_host(None, 4, -1, None) == INVALID_ARGUMENT
    # ... and the engine's wrapper on numpy arrays
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import fold_replicas
    t = np.random.default_rng(1).integers(0, 9, (4, 6, 57)).astype(np.float64)
    f = fold_replicas(t)
    assert f.shape == (5, 6, 57) and f.tobytes() == _fold_loop(t.reshape(4, -1)).tobytes()
    with pytest.raises(_lib.WgrtError):
        fold_replicas(t[:1])


def test_jackknife_se_of_a_linear_statistic():
    """For a mean the delete-a-group jackknife is the standard error of the replica means: the efficiency standard
    error of ``efficiency_error_bars`` against ``jackknife_se`` of the leave-one-out efficiencies computed from the
    folded rows."""
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import fold_replicas
    nl, ny, nx, R, num_iter = 3, 4, 5, 256, 2
    shape = (nl, ny, nx, 80, 120)
    num_rays = nl * ny * nx * R
    for B in (2, 8, 64):
        t = np.random.default_rng(B).integers(0, 40, (B, nl * ny * nx, 57)).astype(np.float64)
        bars = E.efficiency_error_bars(t, shape, num_rays, num_iter)
        assert bars["A_se"].shape == (nl, ny, nx) and bars["efficiency_se"].shape == (nl,)
        rows = fold_replicas(t)
        # a leave-one-out table holds (B - 1) / B of the rays
        loo_A = rows[1:, :, 0].reshape(B, nl, ny, nx) / (num_rays * (B - 1) / B) / num_iter
        loo_eff = 3.0 * loo_A.sum(axis=(2, 3))
        np.testing.assert_allclose(E.jackknife_se(loo_eff), bars["efficiency_se"], rtol=1e-12, atol=0)
        np.testing.assert_allclose(E.jackknife_se(loo_A), bars["A_se"], rtol=1e-12, atol=1e-300)
        # the replica estimates average to the job's figure
        A = rows[0][:, 0].reshape(nl, ny, nx) / num_rays / num_iter
        np.testing.assert_allclose(bars["A_reps"].mean(0), A, rtol=1e-12, atol=1e-300)
    with pytest.raises(ValueError):
        E.jackknife_se(np.zeros((1, 3)))
    # a textbook value: loo = (0, 2) -> sqrt(1/2 * (1 + 1)) = 1
    assert E.jackknife_se(np.array([0.0, 2.0])) == 1.0


def test_evaluation_error_bars_on_the_host():
    """Replica tables built from the fixture's grid: c1_rgb's grid after four launches dealt out bin by bin (the k-th
    occupied bin to replica k % 4), so the replicas are non-empty and add up to the table of ``eb_expected(4)``."""
    c = GoldenCase("c1_rgb")
    eb4 = c.eb_expected(4)
    idx = np.flatnonzero(eb4)
    incs = []
    for b in range(4):
        g = np.zeros_like(eb4)
        g.reshape(-1)[idx[b::4]] = eb4.reshape(-1)[idx[b::4]]
        incs.append(g)
    reps = np.stack([E.eyebox_window_sums(g) for g in incs])
    assert reps.shape == (4, 27, 57) and all(r[:, 0].sum() > 0 for r in reps)
    whole = E.eyebox_window_sums(eb4)
    assert reps.sum(0).tobytes() == whole.tobytes()
    shape, divisor = c.eb_shape(), c.R * 4
    got = E.evaluation_error_bars(reps, shape, divisor, evaluate_on="host")
    assert got["table"].tobytes() == whole.tobytes()
    want = E.evaluation_from_window_sums(whole, shape, divisor)
    for k, w in zip(("delta_e", "U_fov", "U_EB"), want[:3]):
        print(k, float(got[k]).hex(), float(w).hex())
        assert float(got[k]).hex() == float(w).hex(), k
    assert got["jackknife"].shape == (4, 3)
    for k in ("delta_e_se", "U_fov_se", "U_EB_se"):
        assert np.isfinite(got[k]) and got[k] >= 0, k
    np.testing.assert_array_equal(E.jackknife_se(got["jackknife"]),
                                  [got["delta_e_se"], got["U_fov_se"], got["U_EB_se"]])
    with pytest.raises(ValueError):
        E.evaluation_error_bars(reps, shape, divisor, evaluate_on="gpu")
    with pytest.raises(ValueError):
        E.evaluation_error_bars(reps[:1], shape, divisor)


@pytest.mark.parametrize("kw", [dict(eyebox="host"), dict(eyebox="windows", num_rays_per_FoV=20),
                                dict(eyebox="windows", budget=True), dict(eyebox="windows", error_bars=65)])
def test_run_refuses_before_any_gpu_work(kw, monkeypatch):
    """error_bars needs windows mode, B | R / 2 and no budget: each raises ValueError before a device is touched
    (torch.cuda is made to fail loudly if it is)."""
    torch = pytest.importorskip("torch")
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.gpu_ray_tracing_pro_fullColor import run

    def touched(*a, **k):
        raise AssertionError("the device was touched before the arguments were refused")
    for name in ("current_device", "synchronize", "is_available", "device_count", "set_device"):
        monkeypatch.setattr(torch.cuda, name, touched)
    args = dict(num_FOV_x=3, num_FOV_y=3, num_rays_per_FoV=64, num_iter=1, verbose=False, error_bars=4)
    args.update(kw)
    with pytest.raises(ValueError, match="error_bars"):
        run(**args)
