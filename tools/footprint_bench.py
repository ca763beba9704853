#!/usr/bin/env python3
"""The footprint launch against the plain windows launch, timed on the GPU box (analysis tool).

(a) launches  On a bench configuration (default C3), after --warmup launches of each kind, --rounds rounds that
              alternate, in one session, single launches of: the plain windows launch (what the parent runs), the
              footprint launch with the naive sink (one atomic per lane and count,
              wgrt_debug_set_footprint_aggregate(0)) and with the aggregated sink (1), each into a 256 x 256 map
              and into a 1 x 1 map (every add of a channel on one address: the contention ceiling).  Every timed launch
              starts from the same RNG states, so all of them time the same walk.  HIP events; median / min / max ms
              per kind, the plain launch's own run-to-run spread, each kind's ratio to plain, whether both sinks left
              the same map, and which form wins at 256 x 256 by more than that spread.
(b) pmc       With --pmc: one `rocprofv3 --pmc TCC_EA0_ATOMIC_sum` run of its own per form (this script as the
              profiled child, --child FORM: plain launches of that form only), the counter summed over the footprint
              kernel's dispatches and divided by the interactions they counted: atomic requests leaving L2 per
              interaction (the plain launch's own atomics -- eyebox hits, statistics, dequeues -- are reported from a
              third run, to subtract).
(c) driver    With --driver NX NY R K: run(eyebox="windows", evaluate_on="device") with and without
              footprint=(256, 256), alternating, each in a child process: gpu_seconds, and that everything else
              returned agrees.

One JSON line per part.    python tools/footprint_bench.py --pmc --driver 100 75 5000 4 --out profiles/footprint_bench.jsonl
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

KINDS = (("plain", None, None), ("naive_256", 0, "map"), ("aggregated_256", 1, "map"), ("naive_1x1", 0, "one"),
         ("aggregated_1x1", 1, "one"))


def _summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def _setup(config, cells):
    import torch
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.configs import CONFIGS, build_inputs
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.distributed import hip_shard_builder, make_shard
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import FootprintPlan, Scene, WindowPlan, reserve
    w = CONFIGS[config]
    nx, ny, lam, R = w.nx, w.ny, list(w.lambdas), w.R
    dev = torch.device("cuda", 0)
    geom, luts, pts = build_inputs(w)
    scene = Scene.from_geometry(geom, luts)
    rays, rng0 = hip_shard_builder(pts, nx, ny, lam, R, dev)(make_shard(nx, ny, len(lam), R, 1, 0))
    plan = WindowPlan()
    reserve(scene, rng0.numel(), 1)
    fp = FootprintPlan.for_scene(geom, cells=(cells, cells))
    one = FootprintPlan(fp.x0, fp.y0, fp.cell_x * fp.nx_cells, fp.cell_y * fp.ny_cells, 1, 1)
    return dev, scene, rays, rng0, plan, {"map": fp, "one": one}


def launches(a) -> dict:
    import torch
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd import _lib
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import STAT, new_stats, trace_fullcolor
    dev, scene, rays, rng0, plan, fps = _setup(a.config, a.cells)
    table = plan.new_table(scene)
    maps = {name: fps[which].new_map(scene) for name, _, which in KINDS if which}
    rng = rng0.clone()

    def launch(name, agg, which, stats=None):
        rng.copy_(rng0)
        if agg is not None:
            _lib.set_footprint_aggregate(bool(agg))
        trace_fullcolor(scene, rays, rng, None, windows=(plan, table), stats=stats,
                        footprint=(fps[which], maps[name]) if which else None)

    for _ in range(a.warmup):   # (the first plain launches learn the automatic issue order: another kernel)
        for k in KINDS:
            launch(*k)
    torch.cuda.synchronize()
    for m in maps.values():
        m.zero_()
    ms = {name: [] for name, _, _ in KINDS}
    st = new_stats(dev)
    for r in range(a.rounds):   # alternating: every kind once per round
        for name, agg, which in KINDS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            rng.copy_(rng0)
            if agg is not None:
                _lib.set_footprint_aggregate(bool(agg))
            e0.record()
            trace_fullcolor(scene, rays, rng, None, windows=(plan, table), stats=st if name == "plain" else None,
                            footprint=(fps[which], maps[name]) if which else None)
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    _lib.set_footprint_aggregate(True)
    inter = int(st[STAT.interactions]) // a.rounds
    rec = {"tool": "footprint_bench", "part": "launches", "config": a.config, "rays": int(rng0.numel()),
           "device": torch.cuda.get_device_name(0), "warmup": a.warmup, "rounds": a.rounds, "cells": a.cells,
           "interactions_per_launch": inter, "map_bytes": int(maps["naive_256"].numel()) * 8}
    for name, _, _ in KINDS:
        rec[name] = _summary(ms[name])
    p = rec["plain"]
    rec["plain_spread"] = round((p["max_ms"] - p["min_ms"]) / p["median_ms"], 4)
    for name, _, _ in KINDS[1:]:
        rec[name + "_over_plain"] = round(rec[name]["median_ms"] / p["median_ms"], 4)
    rec["maps_equal"] = bool(torch.equal(maps["naive_256"], maps["aggregated_256"]) and
                             torch.equal(maps["naive_1x1"], maps["aggregated_1x1"]))
    rec["map_counts_interactions"] = int(maps["aggregated_256"][:, 0:6].sum()) == inter * a.rounds
    n, g = rec["naive_256"]["median_ms"], rec["aggregated_256"]["median_ms"]
    spread_ms = p["max_ms"] - p["min_ms"]
    rec["winner_256"] = "aggregated" if n - g > spread_ms else "naive" if g - n > spread_ms else "tie (within the plain launch's spread)"
    plan.close()
    scene.close()
    return rec


def child(a) -> None:
    """The profiled workload of a counter pass: single launches of one form only."""
    import torch
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd import _lib
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import STAT, new_stats, trace_fullcolor
    dev, scene, rays, rng0, plan, fps = _setup(a.config, a.cells)
    table = plan.new_table(scene)
    fmap = fps["map"].new_map(scene)
    if a.child != "plain":
        _lib.set_footprint_aggregate(a.child == "aggregated")
    foot = (fps["map"], fmap) if a.child != "plain" else None
    st = new_stats(dev)
    for k in range(a.warmup + a.rounds):
        rng = rng0.clone()
        trace_fullcolor(scene, rays, rng, None, windows=(plan, table), stats=st if k >= a.warmup else None, footprint=foot)
    torch.cuda.synchronize()
    print(json.dumps({"form": a.child, "launches": a.rounds, "interactions": int(st[STAT.interactions]),
                      "eyebox_hits": int(st[STAT.eyebox_hits])}), flush=True)
    plan.close()
    scene.close()


def pmc(a) -> dict:
    counter = "TCC_EA0_ATOMIC_sum"
    rec = {"tool": "footprint_bench", "part": "pmc", "config": a.config, "cells": a.cells, "counter": counter,
           "note": "one rocprofv3 --pmc run per form; the counter summed over the dispatches of the trace kernel the "
                   "form runs (the last `launches` of them) / the interactions those launches counted"}
    for form in ("plain", "naive", "aggregated"):
        d = tempfile.mkdtemp(prefix="fp_pmc_")
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "run", "--pmc", counter, "--",
               sys.executable, os.path.abspath(__file__), "--child", form, "--config", a.config, "--cells", str(a.cells),
               "--warmup", "2", "--rounds", str(a.pmc_launches)]
        r = subprocess.run(cmd, cwd=d, capture_output=True, text=True, timeout=500)
        if r.returncode != 0:
            print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
            raise SystemExit(r.returncode)
        line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        # (the footprint kernels: trace_jones_mode_kernel<..., (wgrt::TraceMode)7, ...>, TraceMode::kFp)
        want = "trace_jones" if form == "plain" else "TraceMode)7"
        per = {}
        for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                if want in row["Kernel_Name"] and "learn" not in row["Kernel_Name"] and row["Counter_Name"] == counter:
                    k = int(row["Dispatch_Id"])
                    per[k] = per.get(k, 0.0) + float(row["Counter_Value"])
        last = [per[k] for k in sorted(per)[-line["launches"]:]]
        rec[form] = {"dispatches": len(last), "atomic_requests": sum(last), "interactions": line["interactions"],
                     "requests_per_interaction": round(sum(last) / max(line["interactions"], 1), 4)}
    return rec


DRIVER_CHILD = r'''
import hashlib, json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import torch
from gpu_ray_tracing_for_waveguide_based_ar_display_amd.gpu_ray_tracing_pro_fullColor import run
nx, ny, R, K = (int(v) for v in sys.argv[3:7])
foot = (256, 256) if sys.argv[2] == "footprint" else None
run(5, 4, 256, 2, lut_seed=0, point_seed=1, verbose=False, eyebox="windows", evaluate_on="device", footprint=foot)   # warm-up
torch.cuda.synchronize()
res = run(nx, ny, R, K, lut_seed=0, point_seed=1, verbose=False, eyebox="windows", evaluate_on="device", footprint=foot,
          fuse=False)
print(json.dumps({"gpu_seconds": res["gpu_seconds"], "bounces": res["bounces"], "eyebox_hits": res["eyebox_hits"],
                  "A_sha": hashlib.sha256(res["A"].tobytes()).hexdigest(),
                  "rng_sha": hashlib.sha256(res["rng_states"].tobytes()).hexdigest(),
                  "figures": [float(res[k]).hex() for k in ("delta_e", "U_fov", "U_EB")],
                  "footprint_interactions": int(res["footprint"][:, 0:6].sum()) if foot else None}))
'''


def driver(a) -> dict:
    rec = {"tool": "footprint_bench", "part": "driver", "job": a.driver, "runs": a.driver_runs,
           "note": "both modes as separate launches (fuse=False): the footprint job's launches are plain single ones"}
    for mode in ("plain", "footprint"):
        rec[mode] = []
    for _ in range(a.driver_runs):   # alternating
        for mode in ("plain", "footprint"):
            p = subprocess.run([sys.executable, "-c", DRIVER_CHILD, REPO, mode] + [str(v) for v in a.driver],
                               capture_output=True, text=True, timeout=900)
            if p.returncode:
                print(p.stderr[-3000:], file=sys.stderr)
                raise SystemExit(p.returncode)
            rec[mode].append(json.loads(p.stdout.strip().splitlines()[-1]))
    d = rec["plain"][0]
    rec["same_results"] = all(all(r[k] == d[k] for k in ("A_sha", "rng_sha", "figures", "bounces", "eyebox_hits"))
                              for r in rec["plain"] + rec["footprint"])
    med = lambda mode: statistics.median(r["gpu_seconds"] for r in rec[mode])
    rec["gpu_seconds_median"] = {m: round(med(m), 5) for m in ("plain", "footprint")}
    rec["gpu_seconds_footprint_over_plain"] = round(med("footprint") / med("plain"), 4)
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--cells", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--no-launches", action="store_true")
    ap.add_argument("--pmc", action="store_true")
    ap.add_argument("--pmc-launches", type=int, default=3)
    ap.add_argument("--child", choices=["plain", "naive", "aggregated"], default=None, help=argparse.SUPPRESS)
    ap.add_argument("--driver", nargs=4, type=int, metavar=("NX", "NY", "R", "K"), default=None)
    ap.add_argument("--driver-runs", type=int, default=2)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("footprint_bench.py needs a HIP device")
    if a.child:
        return child(a)
    for part in ([] if a.no_launches else [launches]) + ([pmc] if a.pmc else []) + ([driver] if a.driver else []):
        line = json.dumps(part(a))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
