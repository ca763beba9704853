"""Window-sum tables for the tests of ``wgrt_eyebox_evaluate`` / ``_host`` (tests/test_eyebox_evaluate.py on
the CPU, tests/test_gpu_eyebox_evaluate.py on the device) and their numpy reference, computed once per case.

A table comes from seeded Poisson counts around 2048 as ``[3, NY, NX, npy, npx]``, laid out as
``eyebox_window_sums`` writes it (rows ``(lambda, FoV)``, column 0 the slab total -- filled with a value the
evaluation must ignore).  Planted in every table: one FoV at 30 x the mean (its sRGB clips).  Planted in the
``dark`` tables: one FoV dark at one eye position, one eye position dark at every FoV (``U_EB = 0``), one FoV
with a single dark wavelength.  The ``lit`` tables have no dark entry (``U_fov > 0``, ``U_EB > 0``)."""
import functools

import numpy as np

from gpu_ray_tracing_for_waveguide_based_ar_display_amd import AR_system_evaluation_functions as E

DIVISOR = 2048.0 * 20   # perceive ~ 0.05: the 30 x FoV reaches 1.5 and clips
# (NY, NX): 35 FoVs are three 16-FoV tiles of the kernel with a ragged last one, 63 and 441 ragged too
GRIDS = [(1, 1), (4, 5), (9, 7), (21, 21), (5, 7)]
# n_pos = 1, 56 (the reference's), 77
WINDOWS = {1: dict(ms=80, step_y=8, step_x=50), 56: dict(ms=30, step_y=8, step_x=12),
           77: dict(ms=20, step_y=10, step_x=10)}
CASES = [(ny, nx, n_pos, kind) for ny, nx in GRIDS for n_pos in WINDOWS for kind in ("dark", "lit")]
RTOL = 1e-12          # scalars and per-position U_EB (the issue's basis: < 100 rounded operations per pixel)
IMAGE_ATOL = 2.0 ** -20


def case_id(c):
    return f"{c[0]}x{c[1]}-p{c[2]}-{c[3]}"


def make_table(ny, nx, n_pos, kind):
    npy, npx = E.window_grid(**WINDOWS[n_pos])
    assert npy * npx == n_pos
    n_fov = ny * nx
    seed = 1000 * n_fov + 10 * n_pos + (kind == "dark")
    counts = np.random.default_rng(seed).poisson(2048, size=(3, n_fov, n_pos)).astype(np.float64)
    counts[:, n_fov - 1, :] *= 30                  # clips
    if kind == "dark":
        counts[:, 0, n_pos // 3] = 0               # one FoV dark at one eye position
        counts[:, :, n_pos - 1] = 0                # one eye position dark everywhere
        counts[1, n_fov // 2, :] = 0               # a single dark wavelength
    table = np.empty((3 * n_fov, 1 + n_pos))
    table[:, 0] = -12345.0                         # the slab total: ignored
    table[:, 1:] = counts.reshape(3 * n_fov, n_pos)
    return table, (3, ny, nx, 80, 120)


def hue_branch_margin(perceive):
    """The smallest ``| |h1p - h2p| - 180 |`` (= ``| |dh| - 180 |``) in degrees over the lit pixels, from the
    module's own functions: where CIEDE2000's hue-difference and mean-hue branches switch, a last-bit
    difference of atan2 could legitimately jump, so the fixed seeds must stay clear of it."""
    wl = np.linalg.inv(E.M_SENSOR) @ np.ones(3)
    lab2 = E.xyz_to_lab(E.XYZ_D65_ASTM / E.XYZ_D65_ASTM[1] * 100.0)
    adjusted = wl[:, None, None] * np.flip(np.transpose(perceive, (1, 2, 0, 3, 4)), axis=2)
    px = np.moveaxis(adjusted, 2, -1).reshape(-1, 3)
    xyz = (E.M_XYZ @ px.T).T
    Y = xyz[:, 1]
    lab = E.xyz_to_lab(xyz / np.maximum(Y, 1e-10)[:, None] * 100)[Y != 0]
    if len(lab) == 0:
        return np.inf
    a1, b1, a2, b2 = lab[:, 1], lab[:, 2], lab2[1], lab2[2]
    Cb7 = ((np.hypot(a1, b1) + np.hypot(a2, b2)) / 2) ** 7
    G = 0.5 * (1 - np.sqrt(Cb7 / (Cb7 + 25.0 ** 7)))
    h1p = np.degrees(np.arctan2(b1, (1 + G) * a1)) % 360
    h2p = np.degrees(np.arctan2(b2, (1 + G) * a2)) % 360
    return float(np.min(np.abs(np.abs(h1p - h2p) - 180)))


def per_position_ueb(perceive):
    """``U_EB[i, j]`` of EVAL:150-157 before the final min / max, flat ``[npy * npx]``."""
    wl = np.linalg.inv(E.M_SENSOR) @ np.ones(3)
    adjusted = wl[:, None, None] * np.flip(np.transpose(perceive, (1, 2, 0, 3, 4)), axis=2)
    n_epy, n_epx = adjusted.shape[3:]
    out = np.zeros(n_epy * n_epx)
    for i in range(n_epy):
        for j in range(n_epx):
            px = adjusted[:, :, :, i, j].reshape(-1, 3)
            y = (E.M_XYZ @ px.T).T[:, 1]
            out[i * n_epx + j] = 0.0 if np.any(y == 0) else np.mean(y)
    return out


@functools.lru_cache(maxsize=None)
def reference(case):
    """``(table, shape, window keywords, (delta_e, U_fov, U_EB, image), per-position U_EB)`` of a case: the
    numpy evaluation of the table, shared by every test of the case and left unchanged."""
    ny, nx, n_pos, kind = case
    table, shape = make_table(ny, nx, n_pos, kind)
    kw = WINDOWS[n_pos]
    perceive = E.perceive_from_window_sums(table, shape, DIVISOR, **kw)
    margin = hue_branch_margin(perceive)
    assert margin > 1e-6, f"{case_id(case)}: a lit pixel is {margin:.3e} degrees from a CIEDE2000 hue branch"
    want = E.evaluation_from_perceive(perceive)
    ueb = per_position_ueb(perceive)
    for a in (table, want[3], ueb):
        a.setflags(write=False)
    return table, shape, kw, want, ueb


def close(got, want, what):
    """Relative ``RTOL``, and exact equality where the reference is exactly 0."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    zero = want == 0
    assert np.array_equal(got[zero], want[zero]), f"{what}: not exactly 0 where the reference is"
    if (~zero).any():
        rel = np.max(np.abs(got[~zero] - want[~zero]) / np.abs(want[~zero]))
        print(f"{what}: max relative deviation {rel:.3e}")
        assert rel <= RTOL, f"{what}: {rel:.3e} > {RTOL}"


def image_close(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    diff = float(np.max(np.abs(got - want))) if got.size else 0.0
    same = int(np.count_nonzero(got == want))
    print(f"{what}: image max |diff| {diff:.3e}, {same} of {got.size} elements equal ({same / max(got.size, 1):.6f})")
    assert diff <= IMAGE_ATOL, f"{what}: image differs by {diff:.3e} > 2^-20"
    return diff, got.size - same
