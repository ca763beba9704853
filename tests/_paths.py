"""The checker of the path lists (``wgrt_trace_paths``): ``tests/oracle_paths.c`` -- the CPU oracle with its hooks
defined, so that every Monte-Carlo draw of the bounce loop of a selected ray, and the end of a trace that leaves the
plate or misses in R5, is appended as a 32-byte record by the checker's own statement of the packing -- built with the
flags ``tests/_expected.py`` uses into a temporary directory and loaded through ``oracle._declare``.  Test
infrastructure only; needs gcc and no GPU."""
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
SRC = os.path.join(HERE, "oracle_paths.c")
# the record, restated (include/wgrt.h wgrt_path_vertex)
DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("gid", "<i8"), ("step", "<u4"), ("flags", "<u4")])

_lib = None


def lib():
    global _lib
    if _lib is None:
        tmp = tempfile.mkdtemp(prefix="wgrt_paths_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        out = os.path.join(tmp, "libwgrt_oracle_paths.so")
        cmd = [os.environ.get("CC", "gcc"), *CFLAGS, "-shared", "-o", out, SRC, "-lm"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"checker build failed ({' '.join(cmd)}):\n{r.stdout}{r.stderr}")
        L = oracle._declare(ctypes.CDLL(out))
        L.wgrt_oracle_paths_set.restype = None
        L.wgrt_oracle_paths_set.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
                                            ctypes.c_uint32]
        L.wgrt_oracle_paths_recorded.restype = ctypes.c_int64
        L.wgrt_oracle_paths_recorded.argtypes = []
        _lib = L
    return _lib


def state(rec):
    return (rec["flags"] & 7).astype(np.int64)


def kind(rec):
    return (rec["flags"] >> 4 & 15).astype(np.int64)


def lmd(rec):
    return (rec["flags"] >> 8 & 255).astype(np.int64)


def tag(rec):
    return (rec["flags"] >> 16).astype(np.int64)


def sort(rec):
    return rec[np.lexsort((rec["step"], rec["gid"], tag(rec)))]


def checker(sc: oracle.OracleScene, rays: dict, rng: np.ndarray, launches: int = 1, gid_offset: int = 0,
            eb: np.ndarray | None = None, select=None, capacity: int | None = None, first_tag: int = 0):
    """``launches`` traces of ``rays`` from the states ``rng`` (updated in place) through the hooked oracle, launch k
    tagged ``first_tag + k``, the rays ``select`` names (uint8 ``[N]``, nonzero; None: all; a list: one mask per
    launch) recorded: ``(records sorted by (tag, gid, step), rng, bounces uint32 of the last launch, fates uint8 [launches,
    N])``.  ``eb``: a float32 grid that takes the oracle's own hits.  ``capacity``: records of room per launch
    (default: 64 per ray, asserted to suffice)."""
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
    fates = np.zeros((launches, N), np.uint8)
    cap = 64 * N if capacity is None else int(capacity)
    parts = []
    for k in range(launches):
        sel = select[k] if isinstance(select, (list, tuple)) else select
        sel = None if sel is None else np.ascontiguousarray(sel, dtype=np.uint8)
        assert sel is None or sel.shape == (N,)
        buf = np.zeros(cap, DTYPE)
        L.wgrt_oracle_paths_set(buf.ctypes.data, cap, int(gid_offset), sel.ctypes.data if sel is not None else None,
                                first_tag + k)
        L.wgrt_oracle_trace(ctypes.byref(sc._s), ctypes.byref(r), N, int(gid_offset), oracle._p(rng, oracle._u32p),
                            oracle._p(eb, oracle._f32p), oracle._p(bounces, oracle._u32p),
                            fates[k].ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), 0)
        n = int(L.wgrt_oracle_paths_recorded())
        assert n <= cap, f"the buffer holds {cap} records, the launch made {n}"
        parts.append(buf[:n])
    L.wgrt_oracle_paths_set(None, 0, 0, None, 0)
    return sort(np.concatenate(parts)), rng, bounces, fates
