#!/usr/bin/env python3
"""What per-ray fates cost, timed on the GPU box (analysis tool; a record, not a gate).

On a bench configuration (default C3) and for one kernel variant (default 0, auto), after --warmup launches of each
kind, HIP events around each of --launches (>= 20) launches of
  plain   a single launch without fates (the kernels every launch ran before fates existed),
  fate    the same launch storing every ray's fate code (wgrt_trace_fate),
  census  the census kernel over the fate buffer the last fate launch left (wgrt_fate_census),
the plain and fate launches alternating, in one session, from the same RNG start states -- so both time the same
traces; the census calls queued behind a backlog of trace launches, so that their events bracket the kernel and not
the host's enqueue.  Median / min / max ms of each, fate over plain, the census table's total against the ray
count, and the loss budget the census gives.  The scene's learning launches are spent in the warm-up (a fate launch
never learns).

One JSON line.    python tools/fate_bench.py --out profiles/fate_bench.jsonl
"""
from __future__ import annotations

import argparse
import datetime
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def _summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def measure(a) -> dict:
    import torch
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.configs import CONFIGS, build_inputs
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.distributed import hip_shard_builder, make_shard
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import (Scene, fate_census, loss_budget, reserve,
                                                                           trace_fullcolor)
    w = CONFIGS[a.config]
    nx, ny, lam, R = w.nx, w.ny, list(w.lambdas), w.R
    dev = torch.device("cuda", 0)
    geom, luts, pts = build_inputs(w)
    scene = Scene.from_geometry(geom, luts)
    rays, rng0 = hip_shard_builder(pts, nx, ny, lam, R, dev)(make_shard(nx, ny, len(lam), R, 1, 0))
    n = int(rng0.numel())
    reserve(scene, n, 1)
    eb = torch.zeros(scene.eb_shape(), dtype=torch.float32, device=dev)
    fate = torch.zeros(n, dtype=torch.uint8, device=dev)
    rng = {k: rng0.clone() for k in ("plain", "fate")}
    kw = {"plain": {}, "fate": {"fate": fate}}
    for _ in range(a.warmup):
        for k in ("plain", "fate"):
            trace_fullcolor(scene, rays, rng[k], eb, variant=a.variant, **kw[k])
    torch.cuda.synchronize()
    for k in rng:   # both kinds time the same traces
        rng[k].copy_(rng0)
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.launches)]
          for k in ("plain", "fate", "census")}
    for j in range(a.launches):   # alternating
        for k in ("plain", "fate"):
            ev[k][j][0].record()
            trace_fullcolor(scene, rays, rng[k], eb, variant=a.variant, **kw[k])
            ev[k][j][1].record()
    torch.cuda.synchronize()
    same = bool(torch.equal(rng["plain"], rng["fate"]))
    table = fate_census(scene, rays, fate)   # warm-up, and the table that is reported
    torch.cuda.synchronize()
    scratch = torch.zeros_like(table)
    # the census kernel is shorter than the host's call that enqueues it, so events around a lone call would time
    # the host: the timed calls are queued behind a backlog of trace launches, where the events bracket the kernel
    for _ in range(2 * a.launches):
        trace_fullcolor(scene, rays, rng["plain"], eb, variant=a.variant)
    for j in range(a.launches):
        ev["census"][j][0].record()
        fate_census(scene, rays, fate, table=scratch)
        ev["census"][j][1].record()
    torch.cuda.synchronize()
    rec = {"tool": "fate_bench", "date": datetime.date.today().isoformat(), "config": a.config, "variant": a.variant,
           "rays": n, "device": torch.cuda.get_device_name(0), "warmup": a.warmup, "launches": a.launches}
    for k in ev:
        rec[k] = _summary([e0.elapsed_time(e1) for e0, e1 in ev[k]])
    rec["fate_over_plain"] = round(rec["fate"]["median_ms"] / rec["plain"]["median_ms"], 4)
    rec["census_over_plain"] = round(rec["census"]["median_ms"] / rec["plain"]["median_ms"], 4)
    rec["same_rng_states"] = same
    rec["census_total"] = int(table.sum())
    rec["census_repeatable"] = bool(torch.equal(scratch, table * a.launches))
    b = loss_budget(table, scene)
    rec["loss_budget"] = {k: round(v, 6) for k, v in b["total"]["fractions"].items()}
    rec["loss_budget_per_wavelength"] = [{k: round(v, 6) for k, v in w_["fractions"].items()} for w_ in b["per_wavelength"]]
    scene.close()
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--variant", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args(argv)
    if a.launches < 20:
        raise SystemExit("--launches must be at least 20")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fate_bench.py needs a HIP device")
    line = json.dumps(measure(a))
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
