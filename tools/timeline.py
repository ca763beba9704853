#!/usr/bin/env python3
"""Wave timeline of one Jones-vector launch (wgrt_debug_opts.timeline): where a launch's time goes.

Runs the bench workload (C3 by default), records per wave: start, queue-exhausted and end
times, passes and lane-passes, and prints a summary: launch span, when the work queue ran dry,
the drain (tail) after it, lane occupancy before and after, per-XCD end times.
Usage: python tools/timeline.py [--config C3] [--num-iter 1] [--variant 0] [--shard N] [--run S] [--taper T] [--out FILE]
--run S: the run length of a fused launch (wgrt_debug_set_fused_run; default: the library's rule).
--taper T: the first tail length of a fused launch (wgrt_debug_set_fused_taper; 0: none; default: the library's rule).
--shard N: rank 0's interleaved FoV x wavelength shard of N (distributed.make_shard), i.e. what one GPU
of the N-GPU strong-scaling run traces.  Single traces use the product's grid rule (wgrt_launch_opts
grid_sqrt_k: ceil(6.5 sqrt(work items)) workgroups), like the launches the bench times.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--num-iter", type=int, default=1)
    ap.add_argument("--variant", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--raw", default=None, help="also save the per-wave records (npz)")
    ap.add_argument("--order", default="none", choices=["none", "lifetime"],
                    help="chunk issue order: ascending, or long-lived tiles first (from a previous launch)")
    ap.add_argument("--shard", type=int, default=1, help="trace rank 0's interleaved shard of N ranks")
    ap.add_argument("--run", type=int, default=None, help="run length of fused launches (wgrt_debug_set_fused_run)")
    ap.add_argument("--taper", type=int, default=None, help="first tail length (wgrt_debug_set_fused_taper; 0: none)")
    a = ap.parse_args()
    import torch
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.configs import CONFIGS, build_inputs
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.distributed import hip_shard_builder, make_shard
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import Scene, schedule_by_lifetime, trace_fullcolor

    dev = torch.device("cuda", 0)
    w = CONFIGS[a.config]
    nx, ny, lam, R = w.nx, w.ny, list(w.lambdas), w.R
    geom, luts, pts = build_inputs(w)
    if a.run is not None:
        from gpu_ray_tracing_for_waveguide_based_ar_display_amd import _lib
        _lib.set_fused_run(a.run)
    if a.taper is not None:
        from gpu_ray_tracing_for_waveguide_based_ar_display_amd import _lib
        _lib.set_fused_taper(a.taper)
    scene = Scene.from_geometry(geom, luts)
    shard = make_shard(nx, ny, len(lam), R, a.shard, 0)
    rays, rng = hip_shard_builder(pts, nx, ny, lam, R, dev)(shard)
    gkw = {} if a.shard == 1 else dict(gid_blocks=torch.as_tensor(shard.gid.block_gid, dtype=torch.int64, device=dev),
                                       gid_block_rays=R)
    eb = torch.zeros(scene.eb_shape(), dtype=torch.float32, device=dev)
    nw = 256 * 8 * 4 * 2
    buf = torch.zeros(8 * nw, dtype=torch.int64, device=dev)
    order = None
    if a.order == "lifetime":
        per = torch.zeros(rng.numel(), dtype=torch.int32, device=dev)
        trace_fullcolor(scene, rays, rng, eb, variant=a.variant, per_ray_bounces=per, **gkw)
        tile = ((rays["lmd_num"].long() * nx + rays["m"].long()) * ny + rays["n"].long())
        order = schedule_by_lifetime(per, tile, len(lam) * nx * ny)
    kw = dict(chunk_order=order) if order is not None else {}
    kw.update(gkw)
    for _ in range(2):
        trace_fullcolor(scene, rays, rng, eb, variant=a.variant, num_iter=a.num_iter, **kw)
    res = []
    for rep in range(a.reps):
        buf.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        trace_fullcolor(scene, rays, rng, eb, variant=a.variant, num_iter=a.num_iter, debug=dict(timeline=buf), **kw)
        e1.record()
        torch.cuda.synchronize()
        t = buf.cpu().numpy().reshape(-1, 8)
        t = t[t[:, 0] > 0]
        start, exh, end, passes, lanes, xcc, p_exh, l_exh = (t[:, k].astype(np.float64) for k in range(8))
        t0 = start.min()
        us = lambda v: (v - t0) / 100.0   # 100 MHz ticks -> us
        r = {"event_ms": e0.elapsed_time(e1), "waves": int(len(t)),
             "start_us": [float(np.percentile(us(start), q)) for q in (0, 50, 100)],
             "exhausted_us": [float(np.percentile(us(exh), q)) for q in (0, 10, 50, 90, 100)],
             "end_us": [float(np.percentile(us(end), q)) for q in (0, 10, 50, 90, 99, 100)],
             # the launch's end: how long the last wave ends after the median wave's queue ran dry
             "end_after_median_dry_us": float(us(end).max() - np.percentile(us(exh), 50)),
             "passes_per_wave": [float(np.percentile(passes, q)) for q in (0, 50, 100)],
             "mean_active_lanes_per_pass": float(lanes.sum() / max(passes.sum(), 1)),
             "bulk_us_per_pass": float(np.median(us(exh) / np.maximum(p_exh, 1))),
             "drain_us_per_pass": float(np.median((end - exh) / 100.0 / np.maximum(passes - p_exh, 1))),
             "drain_passes": [float(np.percentile(passes - p_exh, q)) for q in (0, 50, 100)],
             "drain_lanes_per_pass": float((lanes - l_exh).sum() / max((passes - p_exh).sum(), 1)),
             "bulk_lanes_per_pass": float(l_exh.sum() / max(p_exh.sum(), 1)),
             # the waves that end the launch: their drain passes' mean duration (the critical chain)
             "last1pct_drain_us_per_pass": float(np.median(((end - exh) / 100.0 / np.maximum(passes - p_exh, 1))[
                 us(end) >= np.percentile(us(end), 99)])),
             "last1pct_drain_passes": float(np.median((passes - p_exh)[us(end) >= np.percentile(us(end), 99)])),
             "waves_alive_at_us": {int(tt): int(((us(start) <= tt) & (us(end) > tt)).sum())
                                   for tt in (100, 200, 250, 300, 350, 400)},
             "end_by_xcd_us": {int(x): float(us(end[xcc == x]).max()) for x in np.unique(xcc)},
             "exhausted_by_xcd_us": {int(x): float(us(exh[xcc == x]).max()) for x in np.unique(xcc)}}
        if a.raw:
            np.savez_compressed(f"{a.raw}.{rep}.npz", start=start, exh=exh, end=end, passes=passes, lanes=lanes,
                                xcc=xcc, p_exh=p_exh, l_exh=l_exh)
        r["order"] = a.order
        r["workgroups"] = int(len(t)) // 4
        r["rays"] = int(rng.numel())
        res.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            import hashlib
            from gpu_ray_tracing_for_waveguide_based_ar_display_amd._lib import loaded_path
            with open(loaded_path(), "rb") as lf:
                sha = hashlib.sha256(lf.read()).hexdigest()[:16]
            json.dump({"config": a.config, "num_iter": a.num_iter, "shard_of": a.shard, "fused_run": a.run, "fused_taper": a.taper, "lib_sha16": sha,
                       "runs": res}, f, indent=1)


if __name__ == "__main__":
    main()
