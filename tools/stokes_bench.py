#!/usr/bin/env python3
"""The Stokes launch against the plain windows launch, timed on the GPU box (analysis tool).

On a bench configuration (default C3), after --warmup launches of each kind, --rounds rounds that alternate, in one
session, single launches of: the plain windows launch (what the parent runs) and the Stokes launch (wgrt_trace_stokes)
into the window table and no grid.  Every timed launch starts from the same RNG states, so all of them time the same
walk, and the tables are zeroed before each.  HIP events; median / min / max ms per kind, the plain launch's own
run-to-run spread (max - min over median), the Stokes launch's ratio to plain, the deposits one launch makes, the table
entries it touches, and the mean Stokes vector and degree of polarisation of the delivered light per wavelength.

One JSON line.    python tools/stokes_bench.py --out profiles/stokes_bench.jsonl
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
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import Scene, StokesTable, WindowPlan, reserve
    w = CONFIGS[config]
    nx, ny, lam, R = w.nx, w.ny, list(w.lambdas), w.R
    dev = torch.device("cuda", 0)
    geom, luts, pts = build_inputs(w)
    scene = Scene.from_geometry(geom, luts)
    rays, rng0 = hip_shard_builder(pts, nx, ny, lam, R, dev)(make_shard(nx, ny, len(lam), R, 1, 0))
    plan = WindowPlan()
    reserve(scene, rng0.numel(), 1)
    return dev, scene, rays, rng0, plan, StokesTable(scene, plan, dev)


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
    import numpy as np
    import torch
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.AR_system_evaluation_functions import polarisation_from_stokes
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import trace_fullcolor
    dev, scene, rays, rng0, plan, st = ctx
    table = plan.new_table(scene)
    rng = rng0.clone()
    kinds = ("plain", "stokes")

    def launch(kind):
        trace_fullcolor(scene, rays, rng, None, windows=(plan, table), stokes=st if kind == "stokes" else None)

    for _ in range(a.warmup):   # (the first plain launches learn the automatic issue order: another kernel)
        for k in kinds:
            rng.copy_(rng0)
            launch(k)
    torch.cuda.synchronize()
    ms = {k: [] for k in kinds}
    tables = {}
    for _ in range(a.rounds):   # alternating: every kind once per round
        for k in kinds:
            rng.copy_(rng0)
            table.zero_()
            st.clear()
            ms[k].append(_timed(lambda: launch(k)))
            tables[k] = table.clone()
    N, S = tables["stokes"].cpu().numpy(), st.host()
    nl = scene.num_lmd
    whole = polarisation_from_stokes(N[:, 0].reshape(nl, -1).sum(1)[:, None], S[:, :, 0].reshape(3, nl, -1).sum(2)[:, :, None])
    rec = {"tool": "stokes_bench", "config": a.config, "rays": int(rng0.numel()),
           "device": torch.cuda.get_device_name(0), "warmup": a.warmup, "rounds": a.rounds,
           "deposits_per_launch": int(N[:, 0].sum()), "entries_touched": int((N > 0).sum()),
           "window_adds_per_launch": int(N.sum()), "stokes_atomics_per_launch": int((np.abs(S) > 0).sum()),
           "table_equals_plain": bool(torch.equal(tables["stokes"], tables["plain"])),
           "stokes_bytes": int(st.tables.numel()) * 8,
           "mean_stokes": [[round(float(v), 6) for v in whole["mean"][:, l, 0]] for l in range(nl)],
           "dop": [round(float(v), 6) for v in whole["dop"][:, 0]]}
    for k in kinds:
        rec[k] = _summary(ms[k])
    p = rec["plain"]
    rec["plain_spread"] = round((p["max_ms"] - p["min_ms"]) / p["median_ms"], 4)
    rec["stokes_over_plain"] = round(rec["stokes"]["median_ms"] / p["median_ms"], 4)
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("stokes_bench.py needs a HIP device")
    ctx = _setup(a.config)
    line = json.dumps(launches(a, ctx))
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    ctx[4].close()
    ctx[1].close()


if __name__ == "__main__":
    main()
