"""The checker of the hit list (``wgrt_trace_hits``): ``tests/oracle_hits.c`` -- the CPU oracle with its hooks defined,
so that every trace that ends in an out-coupling records its last draw's position, its global id, its tile and the
reason -- built with the flags ``tests/_expected.py`` uses into a temporary directory and loaded through
``oracle._declare``; and the re-binning rule of ``wgrt_hits_grid`` stated in numpy (``grid_rule``), independent of the
product's header.  Test infrastructure only; needs gcc and no GPU."""
from __future__ import annotations

import atexit
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np

import oracle
from tests._expected import CFLAGS

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "oracle_hits.c")
# wgrt_hit (include/wgrt.h), stated here on its own
HIT_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("gid", "<i8"), ("tile", "<u4"), ("flags", "<u4")])
assert HIT_DTYPE.itemsize == 32

_lib = None


def lib():
    global _lib
    if _lib is None:
        tmp = tempfile.mkdtemp(prefix="wgrt_hits_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        out = os.path.join(tmp, "libwgrt_oracle_hits.so")
        cmd = [os.environ.get("CC", "gcc"), *CFLAGS, "-shared", "-o", out, SRC, "-lm"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"checker build failed ({' '.join(cmd)}):\n{r.stdout}{r.stderr}")
        L = oracle._declare(ctypes.CDLL(out))
        L.wgrt_oracle_hits_set.restype = None
        L.wgrt_oracle_hits_set.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
        L.wgrt_oracle_hits_recorded.restype = ctypes.c_int64
        L.wgrt_oracle_hits_recorded.argtypes = []
        _lib = L
    return _lib


def sort_records(rec: np.ndarray) -> np.ndarray:
    """By (tag, gid), which is unique per record."""
    return rec[np.lexsort((rec["gid"], rec["flags"] >> 16))]


def checker(sc: oracle.OracleScene, rays: dict, rng: np.ndarray, launches: int = 1, gid_offset: int = 0,
            eb: np.ndarray | None = None, tags=None):
    """``launches`` traces of ``rays`` from the states ``rng`` (updated in place) through the hooked oracle:
    ``(records HIT_DTYPE sorted by (tag, gid), rng, bounces uint32 of the last launch, counts per launch)``.  Launch k
    is tagged ``tags[k]`` (default k).  ``eb``: a float32 grid that takes the oracle's own hits."""
    L = lib()
    cols = {k: np.ascontiguousarray(rays[src], dtype=np.float32) for k, src in
            (("x", "x"), ("y", "y"), ("m", "m"), ("n", "n"), ("lmd", "lmd_num"), ("te", "te"), ("tm", "tm"),
             ("dph", "delta_phase")) if not (sc.single_lambda and k == "lmd")}
    N = cols["x"].shape[0]
    assert rng.dtype == np.uint32 and rng.flags.c_contiguous and rng.shape == (N,)
    r = oracle._Rays(*[oracle._p(cols[k], oracle._f32p) if k in cols else None
                       for k in ("x", "y", "m", "n", "lmd", "te", "tm", "dph")])
    eb = np.zeros(sc.eb_shape(), np.float32) if eb is None else eb
    bounces = np.zeros(N, np.uint32)
    fates = np.zeros(N, np.uint8)
    tags = list(range(launches)) if tags is None else list(tags)
    parts, counts = [], []
    for k in range(launches):
        xy = np.zeros((N, 2), np.float64)      # a trace out-couples at most once
        gt = np.zeros((N, 3), np.int64)
        L.wgrt_oracle_hits_set(xy.ctypes.data, gt.ctypes.data, N)
        L.wgrt_oracle_trace(ctypes.byref(sc._s), ctypes.byref(r), N, int(gid_offset), oracle._p(rng, oracle._u32p),
                            oracle._p(eb, oracle._f32p), oracle._p(bounces, oracle._u32p),
                            fates.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), 0)
        n = int(L.wgrt_oracle_hits_recorded())
        assert n <= N
        rec = np.zeros(n, HIT_DTYPE)
        rec["x"], rec["y"] = xy[:n, 0], xy[:n, 1]
        rec["gid"], rec["tile"] = gt[:n, 0], gt[:n, 1]
        rec["flags"] = gt[:n, 2].astype(np.uint32) | np.uint32(tags[k] << 16)
        parts.append(rec)
        counts.append(n)
    L.wgrt_oracle_hits_set(None, None, 0)
    return sort_records(np.concatenate(parts)), rng, bounces, counts


def rule_offsets(rec: np.ndarray, nx: int, ny: int, nl: int, scene_ranges, H: int, W: int, ranges=None):
    """The re-binning rule of ``wgrt_hits_grid`` in numpy: per record, its flat offset in a grid ``[nl, ny, nx, H, W]``,
    or -1 for a record that does not count or falls outside the buffer.  ``scene_ranges`` / ``ranges``: ``[nx, ny, 4]``
    (xmin, xmax, ymin, ymax)."""
    t = rec["tile"].astype(np.int64)
    ok = t < nl * nx * ny
    t = np.where(ok, t, 0)
    l, m, n = t // (nx * ny), t // ny % nx, t % ny
    x, y = rec["x"], rec["y"]
    if ranges is None:
        r = np.asarray(scene_ranges, np.float64).reshape(nx, ny, 4)[m, n]
        ok &= (rec["flags"] & 1).astype(bool)
    else:
        r = np.asarray(ranges, np.float64).reshape(nx, ny, 4)[m, n]
        ok &= (r[:, 0] <= x) & (x <= r[:, 1]) & (r[:, 2] <= y) & (y <= r[:, 3])
    with np.errstate(all="ignore"):
        dx = (r[:, 1] - r[:, 0]) / np.float64(W)
        dy = (r[:, 3] - r[:, 2]) / np.float64(H)
        fx, fy = np.floor((x - r[:, 0]) / dx), np.floor((y - r[:, 2]) / dy)
    ok &= np.isfinite(fx) & np.isfinite(fy)
    ix = np.where(ok, fx, 0).astype(np.int64)
    iy = np.where(ok, fy, 0).astype(np.int64)
    ix = np.where(ix < 0, ix + W, ix)
    iy = np.where(iy < 0, iy + H, iy)
    off = (((l * ny + n) * nx + m) * H + iy) * W + ix
    ok &= (off >= 0) & (off < nl * ny * nx * H * W)
    return np.where(ok, off, -1)


def grid_rule(rec, nx, ny, nl, scene_ranges, H, W, ranges=None) -> np.ndarray:
    """The float32 grid ``[nl, ny, nx, H, W]`` those offsets count into (integer counts: exact below 2^24)."""
    off = rule_offsets(rec, nx, ny, nl, scene_ranges, H, W, ranges)
    cnt = np.bincount(off[off >= 0], minlength=nl * ny * nx * H * W)
    return cnt.astype(np.float32).reshape(nl, ny, nx, H, W)
