#!/usr/bin/env python3
"""Which cache lines of the locator grid a launch's cell gathers touch, per layout of the grid, and how an LRU
cache the size of one XCD's L2 share serves them (analysis tool, CPU only: the prediction the byte locator was
built on).

Builds tools/locator_lines.c (the CPU oracle with a position hook, gcc + OpenMP) into tools/bin/, traces one launch
of a BASELINE workload and keeps the cell of every position the Jones-vector lane would gather, indexed as the
kernels index it (the scene's host hook gives the grid).  Then, per layout -- 4-B cells row-major (the 32-bit word
grid), 1-B row-major (the byte grid), 1-B in 16 x 8 tiles, 2-B in 8 x 8 tiles -- the distinct 128-B lines touched,
and the miss rate of an LRU cache of --l2-mb megabytes over the gathers one XCD sees: the (wavelength, FoV) tiles
x, x + 8, ... (the work queue stripes tiles over the 8 XCDs), --resident of them in flight at a time, their gathers
merged in order of bounce index.  A model: real waves drift apart, and the L2 also holds ray columns and LUT tiles.

    python tools/locator_lines.py --config C3 --out profiles/locator_lines_C3.json
    python tools/locator_lines.py --check c1_rgb h6_edge_rgb     # EDGE / clamped gathers of golden fixtures
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

LINE = 128


def build() -> str:
    out = os.path.join(HERE, "bin", "liblocator_lines.so")
    src = os.path.join(HERE, "locator_lines.c")
    deps = [src, os.path.join(REPO, "oracle", "wgrt_oracle.c")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(map(os.path.getmtime, deps)):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.run(["gcc", "-O2", "-fPIC", "-fopenmp", "-ffp-contract=off", "-std=gnu11", "-shared",
                        "-I", os.path.join(REPO, "oracle"), "-o", out, src, "-lm"], check=True)
    return out


def gathers(geom, luts, rays, wavelength, grid, threads):
    """One oracle launch of ``rays``: (ray, bounce index, ix, iy, clamped) of every gather, and the bounce total."""
    import oracle
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.rays import rng_seeds
    single = wavelength is not None
    sc = oracle.OracleScene.from_geometry(geom, luts, wavelength=wavelength)
    if single:
        rays = dict(rays)
        rays["lmd_num"] = np.zeros_like(rays["x"])
    n = rays["x"].shape[0]
    cols = {k: np.ascontiguousarray(rays[src], dtype=np.float32) for k, src in
            (("x", "x"), ("y", "y"), ("m", "m"), ("n", "n"), ("lmd", "lmd_num"), ("te", "te"),
             ("tm", "tm"), ("dph", "delta_phase"))}
    rr = oracle._Rays(*[cols[k].ctypes.data_as(oracle._f32p) if not (single and k == "lmd") else None
                        for k in ("x", "y", "m", "n", "lmd", "te", "tm", "dph")])
    L = ctypes.CDLL(build())
    L.ll_trace.restype = ctypes.c_int64
    cap = 16 * n
    while True:
        rng, eb = rng_seeds(n, 0), np.zeros(sc.eb_shape(), np.float32)
        o_ray, o_k = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        o_ix, o_iy, o_fl = np.zeros(cap, np.int16), np.zeros(cap, np.int16), np.zeros(cap, np.uint8)
        bounces = ctypes.c_int64()
        p = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))
        got = L.ll_trace(ctypes.byref(sc._s), ctypes.byref(rr), ctypes.c_int64(n), ctypes.c_int64(0),
                         rng.ctypes.data_as(oracle._u32p), eb.ctypes.data_as(oracle._f32p),
                         ctypes.c_double(grid["x0"]), ctypes.c_double(grid["y0"]), ctypes.c_double(1.0 / grid["h"]),
                         ctypes.c_int(grid["ncx"]), ctypes.c_int(grid["ncy"]), p(o_ray, ctypes.c_int32),
                         p(o_k, ctypes.c_int32), p(o_ix, ctypes.c_int16), p(o_iy, ctypes.c_int16),
                         p(o_fl, ctypes.c_uint8), ctypes.c_int64(cap), ctypes.byref(bounces), ctypes.c_int(threads))
        if got < 0:
            raise MemoryError("ll_trace")
        if got <= cap:
            break
        cap = int(got)
    s = slice(0, int(got))
    return o_ray[s], o_k[s], o_ix[s].astype(np.int64), o_iy[s].astype(np.int64), o_fl[s], int(bounces.value)


def layouts(ix, iy, ncx, ncy):
    """Layout name -> (line id of every gather, lines of the whole grid)."""
    lin = iy * ncx + ix
    cdiv = lambda a, b: -(-a // b)
    return {
        "4B_row_major": (lin * 4 // LINE, cdiv(ncx * ncy * 4, LINE)),
        "1B_row_major": (lin // LINE, cdiv(ncx * ncy, LINE)),
        "1B_tiled_16x8": ((iy // 8) * cdiv(ncx, 16) + ix // 16, cdiv(ncx, 16) * cdiv(ncy, 8)),
        "2B_tiled_8x8": ((iy // 8) * cdiv(ncx, 8) + ix // 8, cdiv(ncx, 8) * cdiv(ncy, 8)),
    }


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--cell-mm", type=float, default=1.0 / 128, help="the scene's default cell size")
    ap.add_argument("--l2-mb", type=float, nargs="+", default=[2.0, 3.0, 4.0], help="L2 share given to cells")
    ap.add_argument("--xcd", type=int, default=0)
    ap.add_argument("--resident", type=int, default=32, help="tiles in flight on the XCD at a time")
    ap.add_argument("--threads", type=int, default=min(os.cpu_count() or 1, 16))
    ap.add_argument("--out", default=None)
    ap.add_argument("--check", nargs="+", metavar="FIXTURE", default=None,
                    help="instead: the EDGE-cell and clamped gathers of one launch of golden fixtures (tests/golden)")
    a = ap.parse_args(argv)
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd import _lib

    if a.check:
        from tests._fixtures import GoldenCase
        for name in a.check:
            c = GoldenCase(name)
            t = _lib.locator_palette_host(c.geom, c.luts, cell_mm=a.cell_mm)
            _, _, ix, iy, fl, bounces = gathers(c.geom, c.luts, c.rays, c.wavelength, t, a.threads)
            w = t["cells"][iy, ix]
            edge = ((w >> np.uint64(1)) & ~w & np.uint64(0x5555555555555555)) != 0
            print(json.dumps({"fixture": name, "rays": int(c.N), "bounces": bounces, "gathers": int(ix.size),
                              "edge_cell_gathers": int(edge.sum()), "clamped_gathers": int(fl.sum()),
                              "distinct_words": t["count"]}), flush=True)
        return

    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.configs import CONFIGS, build_inputs
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.rays import build_rays
    w = CONFIGS[a.config]
    geom, luts, points = build_inputs(w)
    single = len(w.lambdas) == 1
    grid = _lib.locator_palette_host(geom, luts, cell_mm=a.cell_mm, tables=False)
    rays = build_rays(points, w.nx, w.ny, list(w.lambdas), w.R, blocks=(0, w.n_blocks))
    ray, k, ix, iy, fl, bounces = gathers(geom, luts, rays, w.lambdas[0] if single else None, grid, a.threads)
    ncx, ncy = grid["ncx"], grid["ncy"]
    lay = layouts(ix, iy, ncx, ncy)
    out = {"config": a.config, "cell_mm": grid["h"], "grid_cells": [ncx, ncy], "distinct_words": grid["count"],
           "rays": int(rays["x"].shape[0]), "bounces": bounces, "gathers": int(ix.size),
           "clamped_gathers": int(fl.sum()),
           "distinct_lines": {n: {"lines": int(np.unique(l).size), "mb": round(np.unique(l).size * LINE / 1e6, 2)}
                              for n, (l, _) in lay.items()}}
    # one XCD's gathers: its tiles in groups of --resident, each group's gathers by bounce index
    tile = ray // w.R
    mine = tile % 8 == a.xcd
    group = (tile // 8) // a.resident
    order = np.lexsort((ray[mine], k[mine], group[mine]))
    L = ctypes.CDLL(build())
    L.ll_lru.restype = ctypes.c_int64
    out["lru"] = {"xcd": a.xcd, "resident_tiles": a.resident, "gathers": int(mine.sum()), "miss_rate": {}}
    for mb in a.l2_mb:
        capl = int(mb * (1 << 20)) // LINE
        row = {}
        for n, (l, nl) in lay.items():
            seq = np.ascontiguousarray(l[mine][order], dtype=np.int32)
            m = L.ll_lru(seq.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.c_int64(seq.size),
                         ctypes.c_int32(int(nl)), ctypes.c_int64(capl))
            row[n] = round(m / max(seq.size, 1), 4)
        out["lru"]["miss_rate"][f"{mb:g}MB"] = row
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
