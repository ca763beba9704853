"""The checker of the footprint maps (``wgrt_trace_footprint``): ``tests/oracle_footprint.c`` -- the CPU oracle with its
event hook defined, so that every Monte-Carlo draw of the bounce loop counts into an int64 plate map by the checker's
own statement of the binning rule -- built with the flags ``tests/_expected.py`` uses into a temporary directory and
loaded through ``oracle._declare``.  Test infrastructure only; needs gcc and no GPU."""
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
SRC = os.path.join(HERE, "oracle_footprint.c")
CHANNELS = 9

_lib = None


def lib():
    global _lib
    if _lib is None:
        tmp = tempfile.mkdtemp(prefix="wgrt_footprint_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        out = os.path.join(tmp, "libwgrt_oracle_footprint.so")
        cmd = [os.environ.get("CC", "gcc"), *CFLAGS, "-shared", "-o", out, SRC, "-lm"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"checker build failed ({' '.join(cmd)}):\n{r.stdout}{r.stderr}")
        L = oracle._declare(ctypes.CDLL(out))
        L.wgrt_oracle_footprint_set.restype = None
        L.wgrt_oracle_footprint_set.argtypes = [ctypes.c_double] * 4 + [ctypes.c_int64] * 2 + [ctypes.c_void_p] * 3 + \
                                               [ctypes.c_int64]
        L.wgrt_oracle_footprint_recorded.restype = ctypes.c_int64
        L.wgrt_oracle_footprint_recorded.argtypes = []
        _lib = L
    return _lib


def checker(sc: oracle.OracleScene, rays: dict, rng: np.ndarray, plan, launches: int = 1, gid_offset: int = 0,
            eb: np.ndarray | None = None, record: int = 0):
    """``launches`` traces of ``rays`` from the states ``rng`` (updated in place) through the hooked oracle into one
    map under ``plan`` (anything with ``x0, y0, cell_x, cell_y, nx_cells, ny_cells``):
    ``(map int64 [num_lmd, 9, ny_cells, nx_cells], rng, bounces uint32 of the last launch, fates uint8 of the last
    launch)``.  ``eb``: a float32 grid that takes the oracle's own hits.  ``record=n``: also, last, the counts of the
    LAST launch as ``(xy float64 [k, 2], lc int32 [k, 2])`` -- position, wavelength and channel of each, at most n."""
    L = lib()
    cols = {k: np.ascontiguousarray(rays[src], dtype=np.float32) for k, src in
            (("x", "x"), ("y", "y"), ("m", "m"), ("n", "n"), ("lmd", "lmd_num"), ("te", "te"), ("tm", "tm"),
             ("dph", "delta_phase")) if not (sc.single_lambda and k == "lmd")}
    N = cols["x"].shape[0]
    assert rng.dtype == np.uint32 and rng.flags.c_contiguous and rng.shape == (N,)
    r = oracle._Rays(*[oracle._p(cols[k], oracle._f32p) if k in cols else None
                       for k in ("x", "y", "m", "n", "lmd", "te", "tm", "dph")])
    fmap = np.zeros((sc.num_lmd, CHANNELS, int(plan.ny_cells), int(plan.nx_cells)), np.int64)
    eb = np.zeros(sc.eb_shape(), np.float32) if eb is None else eb
    bounces = np.zeros(N, np.uint32)
    fates = np.zeros(N, np.uint8)
    rec_xy = np.zeros((record, 2), np.float64) if record else None
    rec_lc = np.zeros((record, 2), np.int32) if record else None
    n_rec = 0
    for k in range(launches):
        last = record and k == launches - 1
        L.wgrt_oracle_footprint_set(float(plan.x0), float(plan.y0), float(plan.cell_x), float(plan.cell_y),
                                    int(plan.nx_cells), int(plan.ny_cells), fmap.ctypes.data,
                                    rec_xy.ctypes.data if last else None, rec_lc.ctypes.data if last else None,
                                    record if last else 0)
        L.wgrt_oracle_trace(ctypes.byref(sc._s), ctypes.byref(r), N, int(gid_offset), oracle._p(rng, oracle._u32p),
                            oracle._p(eb, oracle._f32p), oracle._p(bounces, oracle._u32p),
                            fates.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), 0)
        if last:
            n_rec = int(L.wgrt_oracle_footprint_recorded())
            assert n_rec <= record, f"the record holds {record} counts, the launch made {n_rec}"
    L.wgrt_oracle_footprint_set(0.0, 0.0, 1.0, 1.0, 1, 1, None, None, None, 0)
    out = (fmap, rng, bounces, fates)
    return out + ((rec_xy[:n_rec], rec_lc[:n_rec]),) if record else out
