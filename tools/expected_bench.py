#!/usr/bin/env python3
"""What the expected-value eyebox estimator costs and buys, measured on the GPU box (analysis tool; a record, not a gate).

On a bench configuration (default C3) and for one kernel variant (default 0, auto), after --warmup launches of each
kind, HIP events around each of --launches (>= 20) launches of
  windows    a single launch into the one window table (wgrt_trace_windows; no grid),
  expected   the same launch scoring every out-coupler visit (wgrt_trace_expected),
the kinds alternating, in one session, from the same RNG start states -- so both time the same walks.  Then the same
--launches traces again, from the same start states, into B = --replicas (default 16) replica tables of each kind:
delta_e, U_fov, U_EB and the three efficiencies, each with its jackknife standard error, for both estimators.
Recorded besides: the analog hits per launch (wgrt_trace_stats.eyebox_hits, the same for both kinds), the sum of the
deposited weights per launch, and -- with --count-deposits, from the CPU checker (tests/oracle_expected.c) on the
first launch's rays, which also says how many table entries differ from the reference arithmetic's -- the deposits
of one launch.  The scene's learning launches are spent in the warm-up (an expected-value launch never learns).
--no-deposits zeroes the out-coupling channels of lut_oc1 / lut_oc2 first: the rays that would out-couple are lost at
the same bounce, so the walks keep their lengths, but no visit has a weight and nothing is pushed, binned or added --
what is left of the expected-value launch's extra time is the rectangle test and the double-precision evaluation.

One JSON line.    python tools/expected_bench.py --out profiles/expected_bench.jsonl
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
    import numpy as np
    import torch
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd import AR_system_evaluation_functions as E
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.configs import CONFIGS, build_inputs
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.distributed import hip_shard_builder, make_shard
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import (STAT, Scene, WindowPlan, new_stats, reserve,
                                                                           trace_fullcolor)
    w = CONFIGS[a.config]
    nx, ny, lam, R = w.nx, w.ny, list(w.lambdas), w.R
    dev = torch.device("cuda", 0)
    geom, luts, pts = build_inputs(w)
    if a.no_deposits:   # e3 = 0 at every out-coupler visit (the out-coupling channels of GRTF:1186-1200)
        luts = {k: np.array(v, copy=True) for k, v in luts.items()}
        luts["lut_oc1"][..., [13, 18, 33, 38]] = 0.0
        luts["lut_oc2"][..., [15, 20, 35, 40]] = 0.0
    scene = Scene.from_geometry(geom, luts)
    plan = WindowPlan()
    rays, rng0 = hip_shard_builder(pts, nx, ny, lam, R, dev)(make_shard(nx, ny, len(lam), R, 1, 0))
    n = int(rng0.numel())
    reserve(scene, n, 1)
    kinds = ["windows", "expected"]
    table = {k: plan.new_table(scene) for k in kinds}
    rng = {k: rng0.clone() for k in kinds}
    stats = {k: new_stats(dev) for k in kinds}

    def go(k, tab, B=0):
        trace_fullcolor(scene, rays, rng[k], None, stats=stats[k], variant=a.variant, windows=(plan, tab), replicas=B,
                        expected=k == "expected")
    for _ in range(a.warmup):
        for k in kinds:
            go(k, table[k])
    torch.cuda.synchronize()
    for k in kinds:   # both kinds time the same traces, into zeroed tables
        rng[k].copy_(rng0)
        table[k].zero_()
        stats[k].zero_()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.launches)]
          for k in kinds}
    for j in range(a.launches):   # alternating
        for k in kinds:
            ev[k][j][0].record()
            go(k, table[k])
            ev[k][j][1].record()
    torch.cuda.synchronize()
    rec = {"tool": "expected_bench", "date": datetime.date.today().isoformat(), "config": a.config, "variant": a.variant,
           "rays": n, "device": torch.cuda.get_device_name(0), "warmup": a.warmup, "launches": a.launches,
           "no_deposits": bool(a.no_deposits)}
    for k in kinds:
        rec[k] = _summary([e0.elapsed_time(e1) for e0, e1 in ev[k]])
    rec["expected_over_windows"] = round(rec["expected"]["median_ms"] / rec["windows"]["median_ms"], 4)
    rec["same_rng_states"] = bool(torch.equal(rng["windows"], rng["expected"]))
    rec["same_stats"] = bool(torch.equal(stats["windows"], stats["expected"]))
    rec["hits_per_launch"] = int(stats["windows"][STAT.eyebox_hits]) / a.launches
    rec["bounces_per_launch"] = int(stats["windows"][STAT.bounces]) / a.launches
    rec["weight_per_launch"] = float(table["expected"][:, 0].sum()) / a.launches
    rec["nonzero_entries"] = {k: int((table[k] != 0).sum()) for k in kinds}

    # the same traces into B replica tables of each kind: the figures and their jackknife standard errors
    B = a.replicas
    if R // 2 % B == 0 and scene.num_lmd == 3:
        shape = scene.eb_shape()
        rec["figures"] = {"B": B, "traces": a.launches}
        for k in kinds:
            reps = plan.new_table(scene, replicas=B)
            rng[k].copy_(rng0)
            for _ in range(a.launches):
                go(k, reps, B)
            torch.cuda.synchronize()
            assert torch.equal(reps.sum(0), table[k]), "the replica tables do not add up to the one table"
            bars = E.evaluation_error_bars(reps, shape, R * a.launches, "device", image=None)
            eff = E.efficiency_error_bars(reps, shape, n, a.launches)
            rec["figures"][k] = {**{f: bars[f] for f in ("delta_e", "delta_e_se", "U_fov", "U_fov_se", "U_EB", "U_EB_se")},
                                 "efficiency": [float(v) for v in eff["efficiency_reps"].mean(0)],
                                 "efficiency_se": [float(v) for v in eff["efficiency_se"]]}
            del reps

    if a.count_deposits:   # one launch through the CPU checker: its deposits, and the table against the reference's
        from oracle import OracleScene
        from tests import _expected as X
        host = {k: v.cpu().numpy() for k, v in rays.items()}
        wgt, cnt, orng, _ = X.checker(OracleScene.from_geometry(geom, luts), host, rng0.cpu().numpy().view(np.uint32).copy())
        want, D = X.tables(wgt, cnt)
        one = plan.new_table(scene)
        rng["expected"].copy_(rng0)
        go("expected", one)
        torch.cuda.synchronize()
        ok, differ, worst = X.within_bound(one.cpu().numpy(), want, D)
        rec["checker"] = {"deposits": int(cnt.sum()), "deposits_over_bounces": round(int(cnt.sum()) / rec["bounces_per_launch"], 5),
                          "scored_entries": int((D > 0).sum()), "entries_differing": differ, "worst_quanta": worst,
                          "within_bound": ok,
                          "same_rng_states": bool(np.array_equal(orng, rng["expected"].cpu().numpy().view(np.uint32)))}
    plan.close()
    scene.close()
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--variant", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--replicas", type=int, default=16)
    ap.add_argument("--count-deposits", action="store_true", help="also trace one launch with the CPU checker")
    ap.add_argument("--no-deposits", action="store_true", help="zero the out-coupling channels: no visit deposits")
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args(argv)
    if a.launches < 20:
        raise SystemExit("--launches must be at least 20")
    if not 2 <= a.replicas <= 64:
        raise SystemExit("--replicas must lie in 2 .. 64")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("expected_bench.py needs a HIP device")
    line = json.dumps(measure(a))
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
