"""System evaluation of the eyebox grid (reference ``AR_system_evaluation_functions.py``).

Restates ``evaluation(matrix_EB)`` (EVAL:45-163) without colour-science or OpenCV, which
are absent here.  Returns the same four outputs ``(delta_e, U_fov, U_EB, output_image)``:

* eye positions: the reference samples a 30-px circular pupil at every 8 px (y) and every
  12 px (x) of the 80 x 120 eyebox grid instead of convolving (EVAL:66-109);
* the pure-white sRGB image is mapped to per-wavelength weights with the inverse sensor
  matrix (EVAL:47-52, 112-118) and multiplied by the FoV-flipped pupil-integrated eyebox
  efficiency (EVAL:121);
* per eye position the image is mapped back to sRGB, gamma-encoded, brightness-normalised
  in HSV (EVAL:18-43, via cv2 in the reference), and converted to XYZ / CIELAB to take the
  mean CIEDE2000 difference to D65 white, the FoV uniformity min(Y)/max(Y), and the mean Y
  for the eyebox uniformity (EVAL:122-163).

Third-party pieces restated here (parity unpinned -- neither library is available to pin
against, and the reference has no tests):

* ``colour.XYZ_to_Lab``: the CIE 1976 formula with the CIE 1931 2-degree D65 white point
  xy = (0.3127, 0.3290), applied to XYZ as given (the reference feeds XYZ scaled to Y = 100
  for both the image and the white, which the formula then treats as 100x the white);
* ``colour.sd_to_XYZ(SDS_ILLUMINANTS['D65'])`` normalised to Y = 100: the ASTM E308 D65 /
  2-degree white point (95.047, 100, 108.883), since the spectral tables are not available;
* ``colour.delta_E(..., method='CIE 2000')``: CIEDE2000 after Sharma, Wu & Dalal (2005),
  k_L = k_C = k_H = 1;
* ``cv2.cvtColor`` RGB <-> HSV on float32: OpenCV's float HSV conversion (H in degrees).
"""
from __future__ import annotations

import numpy as np

M_SENSOR = np.array([
    [1.67430115, -0.76582385, -0.06172232],
    [-0.12551154, 1.47840695, -0.04124377],
    [-0.01826868, -0.13098157, 1.61444037],
])
M_XYZ = np.array([
    [6.424000e-01, 1.891400e-01, 2.511000e-01],
    [2.650000e-01, 8.849624e-01, 7.390000e-02],
    [4.999999e-05, 3.693564e-02, 1.528100e+00],
])
D65_XY = (0.3127, 0.3290)
XYZ_D65_ASTM = np.array([95.047, 100.0, 108.883])
_FLT_EPS = np.float32(np.finfo(np.float32).eps)


def linearize_srgb(image_srgb):
    """sRGB (0-1) -> linear RGB (EVAL:5-9)."""
    return np.where(image_srgb <= 0.04045, image_srgb / 12.92, ((image_srgb + 0.055) / 1.055) ** 2.4)


def apply_srgb_gamma(image_linear):
    """Linear RGB (0-1) -> sRGB (EVAL:11-15)."""
    return np.where(image_linear <= 0.0031308, image_linear * 12.92, 1.055 * (image_linear ** (1 / 2.4)) - 0.055)


def rgb_to_hsv_f32(img):
    """OpenCV float RGB -> HSV (H in [0, 360), S and V in [0, 1])."""
    img = img.astype(np.float32)
    r, g, b = img[..., 0], img[..., 1], img[..., 2]
    v = np.maximum(np.maximum(r, g), b)
    vmin = np.minimum(np.minimum(r, g), b)
    diff = v - vmin
    s = diff / (np.abs(v) + _FLT_EPS)
    k = np.float32(60.0) / (diff + _FLT_EPS)
    h = np.where(v == r, (g - b) * k, np.where(v == g, (b - r) * k + np.float32(120.0),
                                               (r - g) * k + np.float32(240.0)))
    h = np.where(h < 0, h + np.float32(360.0), h)
    return np.stack([h, s, v], axis=-1).astype(np.float32)


def hsv_to_rgb_f32(hsv):
    """OpenCV float HSV -> RGB."""
    h = hsv[..., 0].astype(np.float32) * np.float32(6.0 / 360.0)
    s = hsv[..., 1].astype(np.float32)
    v = hsv[..., 2].astype(np.float32)
    h = np.mod(h, np.float32(6.0))
    sector = np.floor(h).astype(np.int64)
    f = (h - sector).astype(np.float32)
    bad = (sector < 0) | (sector >= 6)
    sector = np.where(bad, 0, sector)
    f = np.where(bad, np.float32(0), f)
    tab = np.stack([v, v * (np.float32(1) - s), v * (np.float32(1) - s * f),
                    v * (np.float32(1) - s * (np.float32(1) - f))], axis=-1)
    # OpenCV sector table (b, g, r) indices into tab
    sector_data = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])
    idx = sector_data[sector]
    take = lambda j: np.take_along_axis(tab, idx[..., j:j + 1], axis=-1)[..., 0]
    bb, gg, rr = take(0), take(1), take(2)
    grey = s == 0
    rgb = np.stack([np.where(grey, v, rr), np.where(grey, v, gg), np.where(grey, v, bb)], axis=-1)
    return rgb.astype(np.float32)


def normalize_brightness_without_changing_color(img_srgb_float):
    """Scale the HSV value channel so its maximum is 1 (EVAL:18-43)."""
    hsv = rgb_to_hsv_f32(img_srgb_float)
    max_v = np.max(hsv[..., 2])
    if max_v > 0:
        hsv[..., 2] = hsv[..., 2] / max_v
    return hsv_to_rgb_f32(hsv)


def _lab_f(t):
    eps3 = (24 / 116) ** 3
    return np.where(t > eps3, np.cbrt(t), (841 / 108) * t + 16 / 116)


def xyz_to_lab(xyz, white_xy=D65_XY):
    """CIE 1976 L*a*b* (colour.XYZ_to_Lab with the CIE 1931 2-degree D65 white)."""
    x, y = white_xy
    Xn, Yn, Zn = x / y, 1.0, (1 - x - y) / y
    fx, fy, fz = _lab_f(xyz[..., 0] / Xn), _lab_f(xyz[..., 1] / Yn), _lab_f(xyz[..., 2] / Zn)
    return np.stack([116 * fy - 16, 500 * (fx - fy), 200 * (fy - fz)], axis=-1)


def delta_e_ciede2000(lab1, lab2):
    """CIEDE2000 colour difference (Sharma, Wu & Dalal 2005), k_L = k_C = k_H = 1."""
    lab1 = np.asarray(lab1, dtype=np.float64)
    lab2 = np.broadcast_to(np.asarray(lab2, dtype=np.float64), lab1.shape)
    L1, a1, b1 = lab1[..., 0], lab1[..., 1], lab1[..., 2]
    L2, a2, b2 = lab2[..., 0], lab2[..., 1], lab2[..., 2]
    C1, C2 = np.hypot(a1, b1), np.hypot(a2, b2)
    Cb7 = ((C1 + C2) / 2) ** 7
    G = 0.5 * (1 - np.sqrt(Cb7 / (Cb7 + 25.0 ** 7)))
    a1p, a2p = (1 + G) * a1, (1 + G) * a2
    C1p, C2p = np.hypot(a1p, b1), np.hypot(a2p, b2)
    h1p = np.where((a1p == 0) & (b1 == 0), 0.0, np.degrees(np.arctan2(b1, a1p)) % 360)
    h2p = np.where((a2p == 0) & (b2 == 0), 0.0, np.degrees(np.arctan2(b2, a2p)) % 360)
    dLp = L2 - L1
    dCp = C2p - C1p
    dh = h2p - h1p
    prod = C1p * C2p
    dhp = np.where(prod == 0, 0.0, np.where(dh > 180, dh - 360, np.where(dh < -180, dh + 360, dh)))
    dHp = 2 * np.sqrt(prod) * np.sin(np.radians(dhp / 2))
    Lbp = (L1 + L2) / 2
    Cbp = (C1p + C2p) / 2
    hsum = h1p + h2p
    hbp = np.where(prod == 0, hsum,
                   np.where(np.abs(h1p - h2p) <= 180, hsum / 2,
                            np.where(hsum < 360, (hsum + 360) / 2, (hsum - 360) / 2)))
    T = (1 - 0.17 * np.cos(np.radians(hbp - 30)) + 0.24 * np.cos(np.radians(2 * hbp))
         + 0.32 * np.cos(np.radians(3 * hbp + 6)) - 0.20 * np.cos(np.radians(4 * hbp - 63)))
    dtheta = 30 * np.exp(-(((hbp - 275) / 25) ** 2))
    Cbp7 = Cbp ** 7
    RC = 2 * np.sqrt(Cbp7 / (Cbp7 + 25.0 ** 7))
    SL = 1 + 0.015 * (Lbp - 50) ** 2 / np.sqrt(20 + (Lbp - 50) ** 2)
    SC = 1 + 0.045 * Cbp
    SH = 1 + 0.015 * Cbp * T
    RT = -np.sin(np.radians(2 * dtheta)) * RC
    return np.sqrt((dLp / SL) ** 2 + (dCp / SC) ** 2 + (dHp / SH) ** 2 + RT * (dCp / SC) * (dHp / SH))


def pupil_mask(size: int = 30) -> np.ndarray:
    """Circular eye-pupil mask (EVAL:66-73)."""
    radius = size / 2
    y, x = np.ogrid[:size, :size]
    c = radius - 0.5
    return (np.sqrt((x - c) ** 2 + (y - c) ** 2) <= radius).astype(np.float32)


def eye_perceive(matrix_EB, mask=None, step_y: int = 8, step_x: int = 12):
    """Pupil-integrated eyebox efficiency at the sampled eye positions (EVAL:89-109).

    Accepts a numpy array or a torch tensor (computed on its device) of shape
    [L, NY, NX, 80, 120]; returns an array of shape [L, NY, NX, n_epy, n_epx]."""
    mask = pupil_mask() if mask is None else mask
    ms = mask.shape[0]
    nl, ny, nx, neby, nebx = matrix_EB.shape
    y0s = np.arange(0, neby - ms + 1, step_y)
    x0s = np.arange(0, nebx - ms + 1, step_x)
    try:
        import torch
        is_torch = isinstance(matrix_EB, torch.Tensor)
    except ImportError:  # pragma: no cover
        is_torch = False
    if is_torch:
        m = torch.as_tensor(mask, dtype=matrix_EB.dtype, device=matrix_EB.device)
        out = torch.empty((nl, ny, nx, len(y0s), len(x0s)), dtype=matrix_EB.dtype, device=matrix_EB.device)
        for iy, y0 in enumerate(y0s):
            for ix, x0 in enumerate(x0s):
                out[..., iy, ix] = (matrix_EB[..., y0:y0 + ms, x0:x0 + ms] * m).sum(dim=(-1, -2))
        return out.cpu().numpy()
    out = np.zeros((nl, ny, nx, len(y0s), len(x0s)), dtype=matrix_EB.dtype)
    mb = mask[None, None, None]
    for iy, y0 in enumerate(y0s):
        for ix, x0 in enumerate(x0s):
            out[..., iy, ix] = np.sum(matrix_EB[..., y0:y0 + ms, x0:x0 + ms] * mb, axis=(-1, -2))
    return out


EB_ROWS, EB_COLS = 80, 120   # one (wavelength, FoV) slab of matrix_EB (MAIN:37)
_dev_masks = {}


def window_grid(ms: int = 30, step_y: int = 8, step_x: int = 12) -> tuple[int, int]:
    """``(npy, npx)``: the eye positions an ``ms``-px pupil takes on an 80 x 120 slab at the given steps
    (7 x 8 for the reference's 30 px at 8 / 12, EVAL:89-109)."""
    if not 1 <= ms <= EB_ROWS or step_y < 1 or step_x < 1:
        raise ValueError(f"need 1 <= ms <= {EB_ROWS} and steps >= 1, got ms={ms}, steps=({step_y}, {step_x})")
    return (EB_ROWS - ms) // step_y + 1, (EB_COLS - ms) // step_x + 1


def _square_mask(mask) -> np.ndarray:
    m = pupil_mask() if mask is None else np.asarray(mask.cpu() if hasattr(mask, "cpu") else mask)
    if m.ndim != 2 or m.shape[0] != m.shape[1]:
        raise ValueError(f"mask must be square, got shape {m.shape}")
    return np.ascontiguousarray(m, dtype=np.float32)


def _window_sums_host(eb: np.ndarray, slabs, mask: np.ndarray, step_y: int, step_x: int) -> np.ndarray:
    """The specification of ``eyebox_window_sums`` (include/wgrt.h wgrt_eyebox_window_sums) in float64 numpy."""
    ms = mask.shape[0]
    npy, npx = window_grid(ms, step_y, step_x)
    if eb.shape[-2:] != (EB_ROWS, EB_COLS):
        raise ValueError(f"the grid's last two axes must be ({EB_ROWS}, {EB_COLS}), got {eb.shape}")
    flat = eb.reshape(-1, EB_ROWS, EB_COLS)
    n_slabs = flat.shape[0]
    idx = np.arange(n_slabs, dtype=np.int64) if slabs is None else np.asarray(slabs, dtype=np.int64).reshape(-1)
    ok = (idx >= 0) & (idx < n_slabs)
    out = np.zeros((len(idx), 1 + npy * npx), dtype=np.float64)
    m64 = mask.astype(np.float64)[None]
    rows = np.nonzero(ok)[0]
    for lo in range(0, len(rows), 256):   # 256 slabs as float64: a 20 MB temporary
        rr = rows[lo:lo + 256]
        part = flat[idx[rr]].astype(np.float64)
        out[rr, 0] = part.sum(axis=(-1, -2))
        for iy in range(npy):
            for ix in range(npx):
                y0, x0 = iy * step_y, ix * step_x
                out[rr, 1 + iy * npx + ix] = (part[:, y0:y0 + ms, x0:x0 + ms] * m64).sum(axis=(-1, -2))
    return out


def _window_sums_device(eb, slabs, mask, step_y: int, step_x: int):
    """``wgrt_eyebox_window_sums`` on ``eb``'s device and torch's current stream there; no host sync."""
    import torch

    from ._lib import check, load
    from .engine import _stream_handle
    if eb.dtype != torch.float32 or not eb.is_contiguous():
        raise ValueError(f"a device grid must be contiguous float32, got {eb.dtype}"
                         f"{'' if eb.is_contiguous() else ', not contiguous'}")
    if tuple(eb.shape[-2:]) != (EB_ROWS, EB_COLS):
        raise ValueError(f"the grid's last two axes must be ({EB_ROWS}, {EB_COLS}), got {tuple(eb.shape)}")
    dev = eb.device
    if mask is None:   # the reference's pupil: uploaded once per device
        key = str(dev)
        if key not in _dev_masks:
            _dev_masks[key] = torch.from_numpy(pupil_mask()).to(dev)
        m = _dev_masks[key]
    elif isinstance(mask, torch.Tensor) and mask.device == dev:
        m = mask.to(torch.float32).contiguous()
    else:
        m = torch.from_numpy(_square_mask(mask)).to(dev)
    if m.dim() != 2 or m.shape[0] != m.shape[1]:
        raise ValueError(f"mask must be square, got shape {tuple(m.shape)}")
    ms = int(m.shape[0])
    npy, npx = window_grid(ms, step_y, step_x)
    n_slabs = eb.numel() // (EB_ROWS * EB_COLS)
    if slabs is None:
        idx, n = None, n_slabs
    else:
        idx = torch.as_tensor(slabs, dtype=torch.int64, device=dev).reshape(-1).contiguous()
        n = idx.numel()
    out = torch.empty((n, 1 + npy * npx), dtype=torch.float64, device=dev)
    check(load().wgrt_eyebox_window_sums(eb.data_ptr(), n_slabs, idx.data_ptr() if idx is not None else None, n,
                                         m.data_ptr(), ms, int(step_y), int(step_x), out.data_ptr(),
                                         _stream_handle(dev)), "wgrt_eyebox_window_sums")
    return out


def eyebox_window_sums(eb, slabs=None, mask=None, step_y: int = 8, step_x: int = 12):
    """What anyone reads from the eyebox grid, per 80 x 120 slab: float64 ``[n, W]`` with column 0 the slab's
    total (MAIN:186) and column ``1 + iy * npx + ix`` the sum over ``mask`` (default ``pupil_mask()``) placed at
    ``(iy * step_y, ix * step_x)`` -- ``eye_perceive`` of the slab (EVAL:89-109); W = 57 by default.

    ``eb``: ``[..., 80, 120]``, flattened to ``n_slabs`` slabs.  ``slabs``: the slab of each output row (any
    order, repeats allowed; an index outside ``[0, n_slabs)`` gives a zero row), default every slab in order.
    A contiguous float32 tensor on a HIP device is reduced there by ``wgrt_eyebox_window_sums`` (one pass over
    the grid, on torch's current stream, no host sync) and a torch tensor is returned; a device tensor of
    another dtype or layout raises ``ValueError``.  A numpy array or a host tensor takes the float64 numpy
    statement of the same formula and returns a numpy array.  Sums are float64: an integer-valued grid (the
    kernel adds exactly 1.0 per out-coupling, GRTF:154-165) gives the exact integers on both paths."""
    if getattr(eb, "is_cuda", False):
        return _window_sums_device(eb, slabs, mask, step_y, step_x)
    if hasattr(eb, "detach"):   # a host tensor
        eb = eb.detach().numpy()
    if hasattr(slabs, "detach"):
        slabs = slabs.detach().cpu().numpy()
    return _window_sums_host(np.asarray(eb), slabs, _square_mask(mask), step_y, step_x)


def check_window_plan(mask=None, step_y: int = 8, step_x: int = 12) -> None:
    """The argument check of the trace's window-table sink (``wgrt_window_plan_validate``; needs no GPU):
    raises ``WgrtError`` with the reason unless 1 <= ms <= 80, the steps are >= 1 and every tap of ``mask`` is
    exactly 0 or 1 (the sink adds exactly 1.0 per tap; ``eyebox_window_sums`` serves any other mask from a grid)."""
    from ._lib import check, load
    m = _square_mask(mask)
    check(load().wgrt_window_plan_validate(m.ctypes.data, int(m.shape[0]), int(step_y), int(step_x)),
          "wgrt_window_plan_validate")


def window_table_from_offsets(offsets, n_slabs: int, mask=None, step_y: int = 8, step_x: int = 12) -> np.ndarray:
    """The table the trace's window-table sink leaves for out-couplings at the flat grid ``offsets`` (int64; those
    outside ``[0, n_slabs * 9600)`` are dropped as the grid's guard drops them): float64 ``[n_slabs, W]``, on the
    host through the membership code the kernels compile (``wgrt_window_table_host``; needs no GPU).  Equal to
    ``eyebox_window_sums`` of the grid with one count per offset."""
    from ._lib import check, load
    m = _square_mask(mask)
    npy, npx = window_grid(int(m.shape[0]), step_y, step_x)
    off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    out = np.zeros((int(n_slabs), 1 + npy * npx), dtype=np.float64)
    check(load().wgrt_window_table_host(m.ctypes.data, int(m.shape[0]), int(step_y), int(step_x), off.ctypes.data,
                                        off.size, int(n_slabs), out.ctypes.data), "wgrt_window_table_host")
    return out


def perceive_from_window_sums(sums, shape, divisor, ms: int = 30, step_y: int = 8, step_x: int = 12) -> np.ndarray:
    """``eye_perceive(matrix_EB / R / num_iter)`` from the window sums of the raw grid: ``sums[:, 1:] / divisor``
    (``divisor = R * num_iter``) as float64 ``[L, NY, NX, npy, npx]``.  ``shape``: the grid's shape (its first
    three axes ``L, NY, NX`` are used).  The host path divides every bin in float32 and sums in float32; this
    divides the exact float64 sum once."""
    if hasattr(sums, "detach"):
        sums = sums.detach().cpu().numpy()
    sums = np.asarray(sums, dtype=np.float64)
    npy, npx = window_grid(ms, step_y, step_x)
    nl, ny, nx = (int(v) for v in tuple(shape)[:3])
    if sums.shape != (nl * ny * nx, 1 + npy * npx):
        raise ValueError(f"window sums of shape {sums.shape} do not match a {(nl, ny, nx)} grid with "
                         f"{npy} x {npx} eye positions")
    return (sums[:, 1:] / divisor).reshape(nl, ny, nx, npy, npx)


def evaluation_from_perceive(perceive):
    """``evaluation`` after its first step: everything EVAL:112-163 computes from the pupil-integrated eyebox
    efficiency ``perceive`` ``[L, NY, NX, n_epy, n_epx]`` (``eye_perceive``'s result)."""
    M_inv = np.linalg.inv(M_SENSOR)
    LAB_D65 = xyz_to_lab(XYZ_D65_ASTM / XYZ_D65_ASTM[1] * 100.0)
    n_lambda, n_FOVy, n_FOVx, n_epy, n_epx = perceive.shape
    white = linearize_srgb(np.zeros((n_FOVy, n_FOVx, 3)) + 1.0)
    wl = (M_inv @ white.reshape(-1, 3).T).T.reshape(n_FOVy, n_FOVx, 3)[..., None, None]
    adjusted = wl * np.flip(np.transpose(perceive, (1, 2, 0, 3, 4)), axis=2)
    output_image = np.empty_like(adjusted)
    delta_e = 0.0
    U_fov = 0.0
    U_EB = np.zeros((n_epy, n_epx))
    for i in range(n_epy):
        for j in range(n_epx):
            px = adjusted[:, :, :, i, j].reshape(-1, 3)
            rgb = np.clip((M_SENSOR @ px.T).T.reshape(n_FOVy, n_FOVx, 3), 0, 1)
            output_image[:, :, :, i, j] = normalize_brightness_without_changing_color(apply_srgb_gamma(rgb))
            xyz = (M_XYZ @ px.T).T.reshape(n_FOVy, n_FOVx, 3)
            Y = xyz[:, :, 1]
            xyz_norm = xyz / np.maximum(Y, 1e-10)[..., None] * 100
            lab = xyz_to_lab(xyz_norm)
            lab[Y == 0] = 0
            delta_e += np.mean(delta_e_ciede2000(lab, LAB_D65))
            if np.any(Y == 0):
                U_EB[i, j] = 0
            else:
                U_fov += np.min(Y) / np.max(Y)
                U_EB[i, j] = np.mean(Y)
    delta_e = delta_e / n_epx / n_epy
    U_fov = U_fov / n_epx / n_epy
    U_EB = 0 if np.max(U_EB) == 0 else np.min(U_EB) / np.max(U_EB)
    return delta_e, U_fov, U_EB, output_image


def evaluation(matrix_EB):
    """Drop-in for the reference's ``evaluation`` (EVAL:45-163)."""
    return evaluation_from_perceive(eye_perceive(matrix_EB))


_ev_consts = None
_ev_workspaces = {}   # (device, bytes) -> uint8 tensor, reused by every later call of that size


def _evaluate_consts():
    """``wl = inv(M_SENSOR) . white`` and ``LAB_D65`` as ``evaluation_from_perceive`` computes them (the
    linearised pure-white image is (1, 1, 1) at every FoV), float64 ``[3]`` each."""
    global _ev_consts
    if _ev_consts is None:
        white = linearize_srgb(np.zeros((1, 3)) + 1.0)
        wl = (np.linalg.inv(M_SENSOR) @ white.T).T[0]
        lab = xyz_to_lab(XYZ_D65_ASTM / XYZ_D65_ASTM[1] * 100.0)
        _ev_consts = (np.ascontiguousarray(wl, dtype=np.float64), np.ascontiguousarray(lab, dtype=np.float64))
    return _ev_consts


def evaluation_from_window_sums(sums, shape, divisor, ms: int = 30, step_y: int = 8, step_x: int = 12,
                                image="all"):
    """``evaluation_from_perceive(perceive_from_window_sums(sums, shape, divisor, ...))`` by the library's
    restatement of the same colour math (csrc/wgrt_colour.h): ``(delta_e, U_fov, U_EB, output_image)``.

    ``sums``: the ``[3 * NY * NX, 1 + npy * npx]`` float64 table of ``eyebox_window_sums``.  A tensor on a HIP
    device is evaluated there (``wgrt_eyebox_evaluate``, on torch's current stream; the workspace is cached
    per device and size, so calls of one size on different streams of a device must not overlap) and one small copy brings the scalars back -- and the image only when asked; a numpy
    array or a host tensor goes through the host replica of the same kernels (``wgrt_eyebox_evaluate_host``).
    ``image``: ``"all"`` gives ``output_image`` float64 ``[NY, NX, 3, npy, npx]`` as ``evaluation`` does,
    ``"center"`` only the position MAIN:199-203 exports (``i = 0``, ``j = npx - 1``) as ``[NY, NX, 3]``, ``None``
    no image (``output_image`` is ``None``).  The colour math needs the three wavelengths: ``L != 3`` raises
    ``ValueError``."""
    import ctypes

    from ._lib import check, load
    if image not in ("all", "center", None):
        raise ValueError(f"image must be 'all', 'center' or None, got {image!r}")
    npy, npx = window_grid(ms, step_y, step_x)
    nl, ny, nx = (int(v) for v in tuple(shape)[:3])
    if nl != 3:
        raise ValueError(f"the colour evaluation needs 3 wavelengths, got L = {nl}")
    n_fov, n_pos = ny * nx, npy * npx
    if tuple(sums.shape) != (nl * n_fov, 1 + n_pos):
        raise ValueError(f"window sums of shape {tuple(sums.shape)} do not match a {(nl, ny, nx)} grid with "
                         f"{npy} x {npx} eye positions")
    L = load()
    wl, lab = _evaluate_consts()
    vp = ctypes.c_void_p
    image_pos = -1 if image == "all" else npx - 1
    image_shape = None if image is None else ((n_fov, 3, n_pos) if image == "all" else (n_fov, 3))
    ws_bytes = int(L.wgrt_eyebox_evaluate_workspace_bytes(n_fov, n_pos))
    if ws_bytes < 0:
        raise ValueError(f"a table of {n_fov} FoVs x {n_pos} eye positions is beyond wgrt_eyebox_evaluate's limits")
    if getattr(sums, "is_cuda", False):
        import torch

        from .engine import _stream_handle
        if sums.dtype != torch.float64 or not sums.is_contiguous():
            raise ValueError("a device table must be contiguous float64")
        dev = sums.device
        key = (str(dev), ws_bytes)
        if key not in _ev_workspaces:
            _ev_workspaces[key] = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        ws = _ev_workspaces[key]
        out = torch.empty(3 + n_pos, dtype=torch.float64, device=dev)
        img = None if image is None else torch.empty(image_shape, dtype=torch.float32, device=dev)
        check(L.wgrt_eyebox_evaluate(sums.data_ptr(), n_fov, n_pos, float(divisor), wl.ctypes.data_as(vp),
                                     lab.ctypes.data_as(vp), out.data_ptr(),
                                     img.data_ptr() if img is not None else None, image_pos, ws.data_ptr(),
                                     _stream_handle(dev)), "wgrt_eyebox_evaluate")
        out = out.cpu().numpy()
        img = None if img is None else img.cpu().numpy()
    else:
        if hasattr(sums, "detach"):
            sums = sums.detach().numpy()
        sums = np.ascontiguousarray(sums, dtype=np.float64)
        ws = np.empty(ws_bytes // 8, dtype=np.float64)
        out = np.empty(3 + n_pos, dtype=np.float64)
        img = None if image is None else np.empty(image_shape, dtype=np.float32)
        check(L.wgrt_eyebox_evaluate_host(sums.ctypes.data_as(vp), n_fov, n_pos, float(divisor),
                                          wl.ctypes.data_as(vp), lab.ctypes.data_as(vp), out.ctypes.data_as(vp),
                                          img.ctypes.data_as(vp) if img is not None else None, image_pos,
                                          ws.ctypes.data_as(vp)), "wgrt_eyebox_evaluate_host")
    if img is not None:
        img = img.astype(np.float64).reshape((ny, nx, 3, npy, npx) if image == "all" else (ny, nx, 3))
    return float(out[0]), float(out[1]), float(out[2]), img


# ---- Monte-Carlo error bars from replica window tables (engine.trace_*(replicas=B), engine.fold_replicas) ----
def jackknife_se(loo) -> np.ndarray:
    """The delete-a-group jackknife standard error of a statistic from its ``B`` leave-one-out values ``loo``
    ``[B, ...]``: ``sqrt((B - 1) / B * sum_b (loo_b - mean_b loo)^2)``, over the first axis."""
    loo = np.asarray(loo, dtype=np.float64)
    B = loo.shape[0]
    if B < 2:
        raise ValueError("the jackknife needs at least two leave-one-out values")
    d = loo - loo.mean(axis=0)
    return np.sqrt((B - 1) / B * np.sum(d * d, axis=0))


def _replica_tables(reps_table, shape):
    """``reps_table`` checked against the grid ``shape``: ``(B, (L, NY, NX))``."""
    nl, ny, nx = (int(v) for v in tuple(shape)[:3])
    if len(reps_table.shape) != 3 or reps_table.shape[0] < 2 or reps_table.shape[1] != nl * ny * nx:
        raise ValueError(f"replica tables of shape {tuple(reps_table.shape)} do not match [B >= 2, {nl * ny * nx}, W]")
    return int(reps_table.shape[0]), (nl, ny, nx)


def evaluation_error_bars(reps_table, shape, divisor, evaluate_on: str = "host", ms: int = 30, step_y: int = 8,
                          step_x: int = 12, image="all") -> dict:
    """The evaluation of a job traced into ``B`` replica window tables, with jackknife error bars.

    ``reps_table``: ``[B, n_slabs, W]`` (a device tensor or a numpy array), replica ``b`` counted from the rays whose
    global id is ``b`` mod ``B``; ``shape``: the grid's shape (``L, NY, NX`` are used); ``divisor``: ``R * num_iter``, as
    for the one table.  The replicas are folded (``engine.fold_replicas``) into their sum -- the table a plain
    windows trace leaves, bit for bit -- and the ``B`` leave-one-out tables, each of ``(B - 1) / B`` of the rays and so
    evaluated with ``divisor * (B - 1) / B``.  Every row goes through ``evaluation_from_window_sums``, the library's one
    statement of the colour math: ``evaluate_on="device"`` where the tables live (a device tensor; ``wgrt_eyebox_evaluate``),
    ``"host"`` on their host copy (``wgrt_eyebox_evaluate_host``, no GPU needed), so row 0's figures are, bit for bit,
    what ``evaluation_from_window_sums`` gives for the summed table there.  (``evaluation_from_perceive``, numpy's
    restatement, differs from both in the last place; the jackknife does not see that.)  Only row 0's image is made
    (``image`` as ``evaluation_from_window_sums``).

    Returns ``delta_e``, ``U_fov``, ``U_EB`` (row 0's: what the one table gives), ``delta_e_se``, ``U_fov_se``,
    ``U_EB_se`` (``jackknife_se`` of the leave-one-out values), ``jackknife`` (those values, ``[B, 3]``), ``image`` and
    ``table`` (row 0).  The efficiencies are means over rays, for which the delete-a-group jackknife is the textbook
    estimator (``efficiency_error_bars`` gives the same number directly); ``delta_e`` is a smooth function of such
    means almost everywhere, for which it is a reasonable one.  ``U_fov`` and ``U_EB`` are min / max ratios: for such
    non-smooth statistics the jackknife is known to be unreliable, and their ``_se`` is an indication of scale only.
    With ``B | R / 2`` every tile gives every replica the same number of rays from disjoint subsets of the shared
    origins, which is what makes the replicas exchangeable (``run(error_bars=B)`` requires it)."""
    from .engine import fold_replicas
    if evaluate_on not in ("host", "device"):
        raise ValueError(f"evaluate_on must be 'host' or 'device', got {evaluate_on!r}")
    B, _ = _replica_tables(reps_table, shape)
    loo_div = divisor * (B - 1) / B
    if evaluate_on == "device":
        if not getattr(reps_table, "is_cuda", False):
            raise ValueError("evaluate_on='device' needs the replica tables as a device tensor")
        rows = fold_replicas(reps_table)
    else:
        rows = fold_replicas(reps_table.detach().cpu().numpy() if hasattr(reps_table, "detach") else reps_table)
    ev = lambda t, d, im: evaluation_from_window_sums(t, shape, d, ms, step_y, step_x, image=im)
    delta_e, U_fov, U_EB, img = ev(rows[0], divisor, image)
    loo = np.array([[float(v) for v in ev(rows[1 + b], loo_div, None)[:3]] for b in range(B)], dtype=np.float64)
    se = jackknife_se(loo)
    return dict(delta_e=float(delta_e), U_fov=float(U_fov), U_EB=float(U_EB), delta_e_se=float(se[0]),
                U_fov_se=float(se[1]), U_EB_se=float(se[2]), jackknife=loo, image=img, table=rows[0])


def evaluation_ensemble(tables, shape, divisor, evaluate_on: str = "host", ms: int = 30, step_y: int = 8,
                        step_x: int = 12) -> dict:
    """The three figures of every design of an ensemble: ``tables`` ``[K, n_slabs, W]`` (``VisitTable.reweight_many``'s;
    a device tensor or a numpy array), ``shape`` and ``divisor`` as for the one table.  One
    ``evaluation_from_window_sums(image=None)`` per design -- ``evaluate_on="device"`` where the tables live, ``"host"``
    on their host copy -- so row k is, bit for bit, what that call gives for ``tables[k]`` there.  Returns ``delta_e``,
    ``U_fov`` and ``U_EB``, float64 ``[K]`` each."""
    if evaluate_on not in ("host", "device"):
        raise ValueError(f"evaluate_on must be 'host' or 'device', got {evaluate_on!r}")
    if len(tables.shape) != 3 or tables.shape[0] < 1:
        raise ValueError(f"tables of shape {tuple(tables.shape)} are not [K >= 1, n_slabs, W]")
    K = int(tables.shape[0])
    if evaluate_on == "device":
        if not getattr(tables, "is_cuda", False):
            raise ValueError("evaluate_on='device' needs the tables as a device tensor")
    elif hasattr(tables, "detach"):
        tables = tables.detach().cpu().numpy()
    rows = np.array([[float(v) for v in evaluation_from_window_sums(tables[k], shape, divisor, ms, step_y, step_x,
                                                                    image=None)[:3]] for k in range(K)], dtype=np.float64)
    return dict(delta_e=rows[:, 0].copy(), U_fov=rows[:, 1].copy(), U_EB=rows[:, 2].copy())


def efficiency_error_bars(reps_table, shape, num_rays, num_iter) -> dict:
    """Standard errors of the efficiencies from the replica tables ``[B, n_slabs, W]``: replica ``b`` alone estimates
    ``A_b = B * table[b, :, 0] / num_rays / num_iter`` (it holds a ``B``-th of the rays), so the mean of the ``A_b`` is
    the job's ``A`` and ``A_se = std(A_b, ddof=1) / sqrt(B)``, ``[L, NY, NX]``; the same for each wavelength's
    ``3 * sum(A)``: ``efficiency_se`` ``[L]``.  Also returns the replica values (``A_reps`` ``[B, L, NY, NX]``,
    ``efficiency_reps`` ``[B, L]``).  Equal to ``jackknife_se`` of the leave-one-out efficiencies: for a mean the two
    are the same number."""
    B, (nl, ny, nx) = _replica_tables(reps_table, shape)
    tot = reps_table[:, :, 0]
    tot = tot.detach().cpu().numpy() if hasattr(tot, "detach") else np.asarray(tot)
    A = (B * tot.astype(np.float64) / num_rays / num_iter).reshape(B, nl, ny, nx)
    eff = 3.0 * A.sum(axis=(2, 3))
    return dict(A_se=A.std(axis=0, ddof=1) / np.sqrt(B), efficiency_se=eff.std(axis=0, ddof=1) / np.sqrt(B),
                A_reps=A, efficiency_reps=eff)


def evaluation_device(eb, divisor, evaluate_on: str = "host"):
    """``evaluation(eb / divisor)`` without the grid leaving the device: ``eb`` is the raw count grid
    ``[L, NY, NX, 80, 120]`` (``divisor = R * num_iter``), reduced to its window sums where it lives
    (``eyebox_window_sums``).  ``evaluate_on="host"``: only those ``[L * NY * NX, 57]`` numbers reach the host,
    where the colour math of ``evaluation_from_perceive`` runs; ``"device"``: the table stays on the device
    too and ``evaluation_from_window_sums`` evaluates it there, on the same stream.  Differs from the host path
    only by the float32 rounding of its per-bin division and summation (at most 902 * 2^-24 relative per eye
    position)."""
    if evaluate_on not in ("host", "device"):
        raise ValueError(f"evaluate_on must be 'host' or 'device', got {evaluate_on!r}")
    if len(eb.shape) != 5:
        raise ValueError(f"expected a [L, NY, NX, 80, 120] grid, got {tuple(eb.shape)}")
    sums = eyebox_window_sums(eb)
    if evaluate_on == "device":
        return evaluation_from_window_sums(sums, eb.shape, divisor)
    return evaluation_from_perceive(perceive_from_window_sums(sums, eb.shape, divisor))


# ---- polarisation of the delivered light: the Stokes window tables of wgrt_trace_stokes (csrc/wgrt_stokes.h) -------------
STOKES_QUANTUM = 2.0 ** -30   # a deposit is rint(s_k * 2^30) per normalised Stokes parameter s_k


def _f64(a):
    """``a`` as float64: a torch tensor stays one (on its device), anything else becomes a numpy array."""
    if hasattr(a, "detach"):
        import torch
        return a.detach().to(torch.float64)
    return np.asarray(a, dtype=np.float64)


def _stokes_pair(N, S):
    N, S = _f64(N), _f64(S)
    if S.ndim != 3 or S.shape[0] != 3 or tuple(S.shape[1:]) != tuple(N.shape):
        raise ValueError(f"Stokes tables of shape {tuple(S.shape)} do not lie beside a window table of shape "
                         f"{tuple(N.shape)}: expected [3, n_slabs, W] and [n_slabs, W]")
    return N, S


def polarisation_from_stokes(N, S) -> dict:
    """The polarisation state per (slab, window) entry from the window table ``N`` ``[n_slabs, W]`` and the Stokes tables
    ``S`` int64 ``[3, n_slabs, W]`` of the same launches (``engine.StokesTable``), as float64 numpy arrays: ``mean``
    ``[3, n_slabs, W]``, the mean normalised Stokes vector ``S_k * 2^-30 / N`` of the out-couplings the entry counts;
    ``dop`` its length, the degree of polarisation of their incoherent sum; ``orientation`` ``atan2(s2, s1) / 2``, the
    angle of the ellipse's major axis from the TE axis, in (-pi/2, pi/2]; ``ellipticity`` ``asin(s3 / dop) / 2`` in
    [-pi/4, pi/4] (0 where ``dop`` is 0).  All NaN where ``N == 0``.  The basis is each FoV's own TE / TM basis of its
    out-coupled order (``stokes_rotate`` turns it)."""
    N, S = _stokes_pair(N, S)
    if hasattr(N, "detach"):
        N, S = N.cpu().numpy(), S.cpu().numpy()
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(N > 0, S * STOKES_QUANTUM / N, np.nan)
        dop = np.sqrt((mean * mean).sum(axis=0))
        orientation = 0.5 * np.arctan2(mean[1], mean[0])
        ellipticity = np.where(dop > 0, 0.5 * np.arcsin(np.clip(mean[2] / np.where(dop > 0, dop, 1.0), -1.0, 1.0)),
                               np.where(N > 0, 0.0, np.nan))
    return dict(mean=mean, dop=dop, orientation=orientation, ellipticity=ellipticity)


def stokes_rotate(S, psi):
    """The Stokes tables ``S`` ``[3, n_slabs, W]`` in a basis turned by ``-psi``: every entry's orientation grows by
    ``psi`` (radians; a scalar or one angle per slab, ``[n_slabs]``), i.e. ``(S1, S2)`` turn by ``2 psi`` and ``S3``
    stays.  Float64, still in quanta, so the result feeds ``polarisation_from_stokes`` and ``analyser_table`` as the
    tables do.  A torch tensor is turned where it lives."""
    S = _f64(S)
    if S.ndim != 3 or S.shape[0] != 3:
        raise ValueError(f"expected Stokes tables [3, n_slabs, W], got {tuple(S.shape)}")
    if hasattr(S, "detach"):
        import torch
        a = 2.0 * torch.as_tensor(psi, dtype=torch.float64, device=S.device)
        c, s = torch.cos(a), torch.sin(a)
        stack = torch.stack
    else:
        a = 2.0 * np.asarray(psi, dtype=np.float64)
        c, s = np.cos(a), np.sin(a)
        stack = np.stack
    if a.ndim == 1:
        if a.shape[0] != S.shape[1]:
            raise ValueError(f"{a.shape[0]} angles for {S.shape[1]} slabs")
        c, s = c[:, None], s[:, None]
    elif a.ndim != 0:
        raise ValueError("psi must be a scalar or one angle per slab")
    return stack([c * S[0] - s * S[1], s * S[0] + c * S[1], S[2]])


def analyser_table(N, S, theta):
    """The window table seen through an ideal linear polariser whose axis lies at ``theta`` (radians) from the TE axis:
    ``(N + cos(2 theta) * S1 * 2^-30 + sin(2 theta) * S2 * 2^-30) / 2`` per entry (Malus's law summed over the
    out-couplings), float64 ``[n_slabs, W]`` -- a window table like ``N``, so it feeds ``evaluation_from_window_sums``,
    ``perceive_from_window_sums`` and the efficiencies (column 0) unchanged.  A torch tensor stays on its device."""
    import math
    N, S = _stokes_pair(N, S)
    c, s = math.cos(2.0 * float(theta)), math.sin(2.0 * float(theta))
    return 0.5 * (N + c * (S[0] * STOKES_QUANTUM) + s * (S[1] * STOKES_QUANTUM))
