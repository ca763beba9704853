#!/usr/bin/env python3
"""Same-binary sweep of the fused launches' taper (wgrt_debug_set_fused_taper): one process,
one scene and batch, fused calls of --fused traces each timed with HIP events under no taper, t0 = S/2 and t0 = S/4
(S the automatic run length), the settings interleaved round by round so that drift hits all alike.  Prints one JSON
line per (config, shard, traces): the per-setting medians in ms per trace and each taper's gain over none.

    python tools/taper_sweep.py [--config C3] [--shard 1] [--fused 4,8,20,39,64,200] [--rounds 5]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--shard", type=int, default=1, help="time rank 0's interleaved shard of N instead of the batch")
    ap.add_argument("--fused", default="4,8,20,39,64,200")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd import _lib
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.configs import CONFIGS, build_inputs
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.distributed import hip_shard_builder, make_shard
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import Scene, new_stats, reserve, trace_fullcolor

    dev = torch.device("cuda", 0)
    w = CONFIGS[a.config]
    nx, ny, lam, R = w.nx, w.ny, list(w.lambdas), w.R
    geom, luts, pts = build_inputs(w)
    scene = Scene.from_geometry(geom, luts)
    shard = make_shard(nx, ny, len(lam), R, a.shard, 0)
    rays, rng = hip_shard_builder(pts, nx, ny, lam, R, dev)(shard)
    kw = {} if a.shard == 1 else dict(gid_blocks=torch.as_tensor(shard.gid.block_gid, dtype=torch.int64, device=dev),
                                      gid_block_rays=R)
    eb = torch.zeros(scene.eb_shape(), dtype=torch.float32, device=dev)
    stats = new_stats(dev)
    fused = [int(v) for v in a.fused.split(",")]
    reserve(scene, rays["x"].numel(), max(fused))
    for _ in range(3):
        trace_fullcolor(scene, rays, rng, eb, **kw)
    for n in fused:
        _lib.set_fused_taper(-1)
        run = _lib.fused_run(n)
        settings = sorted({0, run // 2, run // 4})
        ms = {t: [] for t in settings}
        trace_fullcolor(scene, rays, rng, eb, num_iter=n, stats=stats, **kw)
        for _ in range(a.rounds):
            for t in settings:
                _lib.set_fused_taper(t)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                trace_fullcolor(scene, rays, rng, eb, num_iter=n, stats=stats, **kw)
                e1.record()
                torch.cuda.synchronize()
                ms[t].append(e0.elapsed_time(e1) / n)
        med = {t: float(np.median(v)) for t, v in ms.items()}
        print(json.dumps({"config": a.config, "shard_of": a.shard, "traces": n, "run": run,
                          "ms_per_trace": {str(t): round(med[t], 5) for t in settings},
                          "spread_pct": {str(t): round(100 * (max(ms[t]) - min(ms[t])) / med[t], 2) for t in settings},
                          "gain_pct": {str(t): round(100 * (1 - med[t] / med[0]), 2) for t in settings if t}}),
              flush=True)
    _lib.set_fused_taper(-1)
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import check_stats
    check_stats(stats)
    scene.close()


if __name__ == "__main__":
    main()
