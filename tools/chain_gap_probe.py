#!/usr/bin/env python3
"""What a gathering chain costs a caller that does host work between its steps (GPU box; analysis tool).

A chain of ``--steps`` traces of one batch whose caller spends ``gap`` ms on the host after every step (a busy
wait: the caller's own work), as the plain two-queue chain and as a gathering chain (``TraceChain(gather=True)``),
each closed by a device synchronize: wall ms per step, the median of ``--rounds`` rounds, the two modes alternating.
With gap = 0 the steps are called back to back (``run_steps``); with a gap shorter than a launch a gathering chain
holds steps that the plain chain has already enqueued, and the GPU idles until the next call finds it so; with a
gap longer than a launch every step of either chain meets an idle stream.

    python tools/chain_gap_probe.py --config C3 --steps 20 --gaps 0,0.05,0.1,0.2,0.4 --out probe.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--gaps", default="0,0.05,0.1,0.2,0.4", help="host ms after every step, comma-separated")
    ap.add_argument("--out", default=None, help="also write the record to this file")
    a = ap.parse_args(argv)

    import torch
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.configs import CONFIGS, build_inputs
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.distributed import hip_shard_builder, make_shard
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import Scene, TraceChain, check_stats, new_stats

    w = CONFIGS[a.config]
    dev = torch.device("cuda", 0)
    geom, luts, points = build_inputs(w)
    scene = Scene.from_geometry(geom, luts)
    shard = make_shard(w.nx, w.ny, len(w.lambdas), w.R, 1, 0)
    rays, rng = hip_shard_builder(points, w.nx, w.ny, list(w.lambdas), w.R, dev)(shard)
    eb = torch.zeros(scene.eb_shape(), dtype=torch.float32, device=dev)
    stats = new_stats(dev)

    def run(gather: bool, gap_ms: float):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with TraceChain(scene, rays, rng, eb, gid_offset=shard.gid.offset, stats=stats, gather=gather) as ch:
            for _ in range(a.steps):
                ch.step()
                if gap_ms:
                    t = time.perf_counter() + gap_ms * 1e-3
                    while time.perf_counter() < t:
                        pass
            rep = ch.report()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.steps * 1e3, rep["launches"] + (1 if rep["pending"] else 0)

    for g in (False, True):   # untimed: the scene's learning launches, both chains' scratch
        for _ in range(3):
            run(g, 0.0)
    out = []
    for gap in [float(v) for v in a.gaps.split(",")]:
        t = {False: [], True: []}
        launches = []
        for _ in range(a.rounds):
            for g in (False, True):
                ms, n = run(g, gap)
                t[g].append(ms)
                if g:
                    launches.append(n)
        out.append({"host_gap_ms": gap, "two_queue_ms_per_step": round(float(np.median(t[False])), 4),
                    "gathering_ms_per_step": round(float(np.median(t[True])), 4),
                    "two_queue_spread": round(max(t[False]) - min(t[False]), 4),
                    "gathering_spread": round(max(t[True]) - min(t[True]), 4),
                    "gathering_launches_median": float(np.median(launches))})
    check_stats(stats)
    rec = {"config": a.config, "steps": a.steps, "rounds": a.rounds, "rays_per_trace": shard.n_rays, "gaps": out,
           "note": "wall ms per step of a chain whose caller busy-waits host_gap_ms after every step, then one "
                   "synchronize; medians over the rounds, the two modes alternating; spread = max - min"}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    scene.close()


if __name__ == "__main__":
    main()
