#!/usr/bin/env python3
"""What replica window tables cost, timed on the GPU box (analysis tool; a record, not a gate).

On a bench configuration (default C3) and for one kernel variant (default 0, auto), after --warmup launches of each
kind, HIP events around each of --launches (>= 20) launches of
  windows      a single launch into the one window table (wgrt_trace_windows; no grid),
  replicas_B   the same launch into B replica tables (wgrt_trace_replicas), for every B of --replicas (default 8, 16),
the kinds alternating, in one session, from the same RNG start states -- so all time the same traces; then, queued
behind a backlog of trace launches so that their events bracket the kernels and not the host's enqueue,
  fold_B       wgrt_window_replicas_fold of the B tables,
  evaluate_B   the B + 1 device evaluations of the folded rows (wgrt_eyebox_evaluate, no image).
Median / min / max ms of each, replicas over windows, whether the replica tables add up to the one table bit for
bit, and the figures with their jackknife standard errors at the largest B.  The scene's learning launches are spent
in the warm-up (a replica launch never learns).

One JSON line.    python tools/replica_bench.py --out profiles/replica_bench.jsonl
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
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd import AR_system_evaluation_functions as E
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.configs import CONFIGS, build_inputs
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.distributed import hip_shard_builder, make_shard
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import (Scene, WindowPlan, fold_replicas, reserve,
                                                                           trace_fullcolor)
    w = CONFIGS[a.config]
    nx, ny, lam, R = w.nx, w.ny, list(w.lambdas), w.R
    dev = torch.device("cuda", 0)
    geom, luts, pts = build_inputs(w)
    scene = Scene.from_geometry(geom, luts)
    plan = WindowPlan()
    rays, rng0 = hip_shard_builder(pts, nx, ny, lam, R, dev)(make_shard(nx, ny, len(lam), R, 1, 0))
    n = int(rng0.numel())
    reserve(scene, n, 1)
    kinds = ["windows"] + [f"replicas_{B}" for B in a.replicas]
    reps = dict(zip(kinds, [0] + list(a.replicas)))
    table = {k: plan.new_table(scene, replicas=reps[k]) for k in kinds}
    rng = {k: rng0.clone() for k in kinds}
    go = lambda k: trace_fullcolor(scene, rays, rng[k], None, variant=a.variant, windows=(plan, table[k]),
                                   replicas=reps[k])
    for _ in range(a.warmup):
        for k in kinds:
            go(k)
    torch.cuda.synchronize()
    for k in kinds:   # every kind times the same traces, into zeroed tables
        rng[k].copy_(rng0)
        table[k].zero_()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.launches)]
          for k in kinds + [f"{p}_{B}" for B in a.replicas for p in ("fold", "evaluate")]}
    for j in range(a.launches):   # alternating
        for k in kinds:
            ev[k][j][0].record()
            go(k)
            ev[k][j][1].record()
    torch.cuda.synchronize()
    same_rng = all(bool(torch.equal(rng["windows"], rng[k])) for k in kinds)
    adds_up = all(bool(torch.equal(table[k].sum(0), table["windows"])) for k in kinds[1:])
    shape, traces = scene.eb_shape(), a.launches
    for B in a.replicas:
        k = f"replicas_{B}"
        rows = fold_replicas(table[k])   # warm-up
        for r in range(1 + B):
            E.evaluation_from_window_sums(rows[r], shape, R * traces, image=None)
        torch.cuda.synchronize()
        # both are shorter than the host's calls that enqueue them: timed behind a backlog of trace launches
        for _ in range(2 * a.launches):
            go("windows")
        for j in range(a.launches):
            ev[f"fold_{B}"][j][0].record()
            rows = fold_replicas(table[k])
            ev[f"fold_{B}"][j][1].record()
        torch.cuda.synchronize()
        # (an evaluation reads its scalars back, so each synchronises: the B + 1 of them between two events)
        for j in range(a.launches):
            ev[f"evaluate_{B}"][j][0].record()
            for r in range(1 + B):
                E.evaluation_from_window_sums(rows[r], shape, R * traces * (1.0 if r == 0 else (B - 1) / B), image=None)
            ev[f"evaluate_{B}"][j][1].record()
        torch.cuda.synchronize()
    rec = {"tool": "replica_bench", "date": datetime.date.today().isoformat(), "config": a.config, "variant": a.variant,
           "rays": n, "device": torch.cuda.get_device_name(0), "warmup": a.warmup, "launches": a.launches,
           "replicas": list(a.replicas)}
    for k in ev:
        rec[k] = _summary([e0.elapsed_time(e1) for e0, e1 in ev[k]])
    for B in a.replicas:
        rec[f"replicas_{B}_over_windows"] = round(rec[f"replicas_{B}"]["median_ms"] / rec["windows"]["median_ms"], 4)
    rec["same_rng_states"] = same_rng
    rec["replicas_add_up"] = adds_up
    B = max(a.replicas)
    if R // 2 % B == 0 and scene.num_lmd == 3:
        bars = E.evaluation_error_bars(table[f"replicas_{B}"], shape, R * traces, "device", image=None)
        eff = E.efficiency_error_bars(table[f"replicas_{B}"], shape, n, traces)
        rec["error_bars"] = {"B": B, "traces": traces,
                             **{k: bars[k] for k in ("delta_e", "delta_e_se", "U_fov", "U_fov_se", "U_EB", "U_EB_se")},
                             "efficiency": [float(v) for v in eff["efficiency_reps"].mean(0)],
                             "efficiency_se": [float(v) for v in eff["efficiency_se"]]}
    plan.close()
    scene.close()
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--variant", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--replicas", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args(argv)
    if a.launches < 20:
        raise SystemExit("--launches must be at least 20")
    if any(not 2 <= B <= 64 for B in a.replicas):
        raise SystemExit("--replicas must lie in 2 .. 64")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("replica_bench.py needs a HIP device")
    line = json.dumps(measure(a))
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
