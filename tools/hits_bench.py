#!/usr/bin/env python3
"""The hits launch against the plain windows launch, and the re-binning of its list, timed on the GPU box (analysis tool).

(a) launches  On a bench configuration (default C3), after --warmup launches of each kind, --rounds rounds that
              alternate, in one session, single launches of: the plain windows launch (what the parent runs) and the
              hits launch (wgrt_trace_hits) into a list sized for every ray.  Every timed launch starts from the same RNG
              states, so all of them time the same walk, and the list's counter is zeroed before each.  HIP events;
              median / min / max ms per kind, the plain launch's own run-to-run spread, the hits launch's ratio to
              plain, and the out-couplings one launch appends (inside / beside the eyebox).
(b) grid      wgrt_hits_grid of one launch's list, at 80 x 120 and at 160 x 240 over the scene's ranges, --rounds times
              each into a zeroed grid: median / min / max ms, and that the 80 x 120 grid equals the matrix_EB a launch
              with a grid leaves.

One JSON line per part.    python tools/hits_bench.py --out profiles/hits_bench.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def _summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def _setup(config):
    import torch
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.configs import CONFIGS, build_inputs
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.distributed import hip_shard_builder, make_shard
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import HitList, Scene, WindowPlan, reserve
    w = CONFIGS[config]
    nx, ny, lam, R = w.nx, w.ny, list(w.lambdas), w.R
    dev = torch.device("cuda", 0)
    geom, luts, pts = build_inputs(w)
    scene = Scene.from_geometry(geom, luts)
    rays, rng0 = hip_shard_builder(pts, nx, ny, lam, R, dev)(make_shard(nx, ny, len(lam), R, 1, 0))
    plan = WindowPlan()
    reserve(scene, rng0.numel(), 1)
    return dev, scene, rays, rng0, plan, HitList(rng0.numel(), dev)


def _timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def launches(a, ctx) -> dict:
    import torch
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import hit_inside, trace_fullcolor
    dev, scene, rays, rng0, plan, hl = ctx
    table = plan.new_table(scene)
    rng = rng0.clone()
    kinds = ("plain", "hits")

    def launch(kind):
        trace_fullcolor(scene, rays, rng, None, windows=(plan, table), hits=(hl, 0) if kind == "hits" else None)

    for _ in range(a.warmup):   # (the first plain launches learn the automatic issue order: another kernel)
        for k in kinds:
            rng.copy_(rng0)
            launch(k)
    torch.cuda.synchronize()
    ms = {k: [] for k in kinds}
    for _ in range(a.rounds):   # alternating: every kind once per round
        for k in kinds:
            rng.copy_(rng0)
            hl.clear()
            ms[k].append(_timed(lambda: launch(k)))
    rec_ = hl.records()
    rec = {"tool": "hits_bench", "part": "launches", "config": a.config, "rays": int(rng0.numel()),
           "device": torch.cuda.get_device_name(0), "warmup": a.warmup, "rounds": a.rounds,
           "out_couplings_per_launch": hl.count(), "inside": int(hit_inside(rec_).sum()),
           "beside": int((~hit_inside(rec_)).sum()), "list_bytes": int(hl.buffer.numel())}
    for k in kinds:
        rec[k] = _summary(ms[k])
    p = rec["plain"]
    rec["plain_spread"] = round((p["max_ms"] - p["min_ms"]) / p["median_ms"], 4)
    rec["hits_over_plain"] = round(rec["hits"]["median_ms"] / p["median_ms"], 4)
    return rec


def grid(a, ctx) -> dict:
    import torch
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import trace_fullcolor
    dev, scene, rays, rng0, plan, hl = ctx
    rng = rng0.clone()
    hl.clear()
    eb = torch.zeros(scene.eb_shape(), dtype=torch.float32, device=dev)
    trace_fullcolor(scene, rays, rng, eb, hits=(hl, 0))
    torch.cuda.synchronize()
    rec = {"tool": "hits_bench", "part": "grid", "config": a.config, "records": hl.stored(), "rounds": a.rounds}
    for H, W in ((80, 120), (160, 240)):
        g = torch.zeros(tuple(scene.eb_shape()[:-2]) + (H, W), dtype=torch.float32, device=dev)
        hl.grid(scene, H, W, out=g)   # warm-up
        ms = []
        for _ in range(a.rounds):
            g.zero_()
            ms.append(_timed(lambda: hl.grid(scene, H, W, out=g)))
        rec[f"{H}x{W}"] = dict(_summary(ms), grid_bytes=int(g.numel()) * 4, counted=int(g.sum().item()))
        if (H, W) == (80, 120):
            rec["equals_matrix_EB"] = bool(torch.equal(g, eb))
        del g
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("hits_bench.py needs a HIP device")
    ctx = _setup(a.config)
    for part in (launches, grid):
        line = json.dumps(part(a, ctx))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    ctx[4].close()
    ctx[1].close()


if __name__ == "__main__":
    main()
