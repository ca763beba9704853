#!/usr/bin/env python3
"""The visits launch against the plain windows launch, and the two reductions of its rows, timed on the GPU box
(analysis tool).

(a) launches    On a bench configuration (default C3), after --warmup launches of each kind, --rounds rounds that
                alternate, in one session, single launches of: the plain windows launch (the parent's kernel), the fate
                launch (the first pass that chooses the rows; like every launch here it fills the window table and no
                grid, so its ratio is to the plain windows launch), the visits launch with the eyebox class
                selected (one row per delivered ray), and the visits launch with every ray counted (row i for ray i).
                Every timed launch starts from the same RNG states, so all of them time the same walk; the rows are
                zeroed before each, outside the timed region.  HIP events; median / min / max ms per kind, the plain
                launch's own run-to-run spread, each kind's ratio to plain, the rows and the counts one launch adds.
(b) reductions  wgrt_visits_sensitivity and wgrt_visits_reweight over the eyebox rows and over every ray's rows, --rounds
                times each into a zeroed table: median / min / max ms; that the re-weighted table with every scale 1 is the
                launch's window table; and the device memory of the sensitivity tables here and at the default job.

(c) pmc         With --pmc: one `rocprofv3 --pmc TCC_EA0_ATOMIC_sum` run of its own per form (this script as the child
                process; plain, eyebox rows, every ray): the atomic requests that leave L2 during the trace kernel's
                dispatches, per counted branch -- whether the every-ray form is bound by the count of its atomic adds,
                as the footprint launch is (about 21 G requests / s).

One JSON line per part.    python tools/visits_bench.py --pmc --out profiles/visits_bench.jsonl
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


def _summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def _setup(config):
    import torch
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.configs import CONFIGS, build_inputs
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.distributed import hip_shard_builder, make_shard
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import Scene, WindowPlan, reserve
    w = CONFIGS[config]
    nx, ny, lam, R = w.nx, w.ny, list(w.lambdas), w.R
    dev = torch.device("cuda", 0)
    geom, luts, pts = build_inputs(w)
    scene = Scene.from_geometry(geom, luts)
    rays, rng0 = hip_shard_builder(pts, nx, ny, lam, R, dev)(make_shard(nx, ny, len(lam), R, 1, 0))
    plan = WindowPlan()
    reserve(scene, rng0.numel(), 1)
    return dev, scene, rays, rng0, plan


def _timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def _rows(ctx):
    """The eyebox class of one launch from the start states: ``(mask int32, slot int32, n)``."""
    import torch
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import select_by_fate, trace_fullcolor
    dev, scene, rays, rng0, plan = ctx
    fate = torch.zeros(rng0.numel(), dtype=torch.uint8, device=dev)
    trace_fullcolor(scene, rays, rng0.clone(), None, windows=(plan, plan.new_table(scene)), fate=fate)
    mask = select_by_fate(fate, "eyebox").to(torch.int32)
    slot = torch.where(mask != 0, torch.cumsum(mask, 0, dtype=torch.int32) - mask, torch.full_like(mask, -1))
    return fate, slot, int(mask.sum().item())


def launches(a, ctx) -> dict:
    import torch
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import VisitTable, trace_fullcolor
    dev, scene, rays, rng0, plan = ctx
    table = plan.new_table(scene)
    fate, slot, n = _rows(ctx)
    vt_eye, vt_all = VisitTable(scene, n, dev), VisitTable(scene, rng0.numel(), dev)
    rng = rng0.clone()
    kinds = ("plain", "fate", "visits_eyebox", "visits_all")

    def launch(kind):
        kw = {"fate": dict(fate=fate), "visits_eyebox": dict(visits=(vt_eye, slot)),
              "visits_all": dict(visits=(vt_all, None))}.get(kind, {})
        trace_fullcolor(scene, rays, rng, None, windows=(plan, table), **kw)

    for _ in range(a.warmup):   # (the first plain launches learn the automatic issue order: another kernel)
        for k in kinds:
            rng.copy_(rng0)
            launch(k)
    torch.cuda.synchronize()
    ms = {k: [] for k in kinds}
    added = {}
    for _ in range(a.rounds):   # alternating: every kind once per round
        for k in kinds:
            rng.copy_(rng0)
            vt_eye.clear()
            vt_all.clear()
            ms[k].append(_timed(lambda: launch(k)))
            if k.startswith("visits"):   # what one launch adds to its zeroed rows
                added[k] = int((vt_eye if k == "visits_eyebox" else vt_all).counts.sum().item())
    rec = {"tool": "visits_bench", "part": "launches", "config": a.config, "rays": int(rng0.numel()),
           "device": torch.cuda.get_device_name(0), "warmup": a.warmup, "rounds": a.rounds, "channels": vt_all.n_channels,
           "rows_eyebox": n, "counts_eyebox": added["visits_eyebox"], "counts_all": added["visits_all"],
           "rows_bytes_eyebox": int(vt_eye.counts.numel() * 4 + vt_eye.ends.numel()),
           "rows_bytes_all": int(vt_all.counts.numel() * 4 + vt_all.ends.numel())}
    for k in kinds:
        rec[k] = _summary(ms[k])
    p = rec["plain"]["median_ms"]
    rec["plain_spread"] = round((rec["plain"]["max_ms"] - rec["plain"]["min_ms"]) / p, 4)
    for k in kinds[1:]:
        rec[f"{k}_over_plain"] = round(rec[k]["median_ms"] / p, 4)
    rec["fate_plus_visits_eyebox_over_plain"] = round((rec["fate"]["median_ms"] + rec["visits_eyebox"]["median_ms"]) / p, 4)
    return rec


def reductions(a, ctx) -> dict:
    import torch
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import VisitTable, trace_fullcolor
    dev, scene, rays, rng0, plan = ctx
    _, slot, n = _rows(ctx)
    rec = {"tool": "visits_bench", "part": "reductions", "config": a.config, "rounds": a.rounds}
    for name, vt, sl in (("eyebox", VisitTable(scene, n, dev), slot), ("all", VisitTable(scene, rng0.numel(), dev), None)):
        table = plan.new_table(scene)
        trace_fullcolor(scene, rays, rng0.clone(), None, windows=(plan, table), visits=(vt, sl))
        sens = vt.sensitivity(plan)   # warm-up
        ones = torch.ones(vt.n_channels, dtype=torch.float64)
        out = vt.reweight(plan, ones)
        torch.cuda.synchronize()
        same = bool(torch.equal(out, table))
        ms_s, ms_r = [], []
        for _ in range(a.rounds):
            sens.zero_()
            ms_s.append(_timed(lambda: vt.sensitivity(plan, out=sens)))
            out.zero_()
            ms_r.append(_timed(lambda: vt.reweight(plan, ones, out=out)))
        rec[name] = {"rows": vt.n_rows, "sensitivity": _summary(ms_s), "reweight": _summary(ms_r),
                     "reweight_ones_equals_table": same}
        rec["sens_bytes"] = int(sens.numel() * 8)
    # the default job (100 x 75 FoVs x 3 wavelengths = 22,500 slabs): C x 22,500 x 57 x 8 B
    rec["sens_bytes_default_job"] = int(rec["sens_bytes"] // (scene.num_lmd * scene.nx * scene.ny) * 22500)
    return rec


def child(a):
    """One form's launches, for a counter run: --warmup then --rounds launches from the same RNG states."""
    import torch
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import VisitTable, trace_fullcolor
    ctx = _setup(a.config)
    dev, scene, rays, rng0, plan = ctx
    table = plan.new_table(scene)
    kw, vt = {}, None
    if a.child == "visits_eyebox":
        _, slot, n = _rows(ctx)
        vt = VisitTable(scene, n, dev)
        kw = dict(visits=(vt, slot))
    elif a.child == "visits_all":
        vt = VisitTable(scene, rng0.numel(), dev)
        kw = dict(visits=(vt, None))
    for k in range(a.warmup + a.rounds):
        if k == a.warmup and vt is not None:
            vt.clear()
        trace_fullcolor(scene, rays, rng0.clone(), None, windows=(plan, table), **kw)
    torch.cuda.synchronize()
    print(json.dumps({"form": a.child, "launches": a.rounds,
                      "counts": int(vt.counts.sum().item()) if vt is not None else 0}), flush=True)
    plan.close()
    scene.close()


def pmc(a, ctx=None) -> dict:
    counter = "TCC_EA0_ATOMIC_sum"
    rec = {"tool": "visits_bench", "part": "pmc", "config": a.config, "counter": counter,
           "note": "one rocprofv3 --pmc run per form; the counter summed over the dispatches of the trace kernel the "
                   "form runs (the last `launches` of them); counts: the branches those launches counted"}
    for form in ("plain", "visits_eyebox", "visits_all"):
        d = tempfile.mkdtemp(prefix="visits_pmc_")
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "run", "--pmc", counter, "--",
               sys.executable, os.path.abspath(__file__), "--child", form, "--config", a.config,
               "--warmup", "2", "--rounds", str(a.pmc_launches)]
        r = subprocess.run(cmd, cwd=d, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
            raise SystemExit(r.returncode)
        line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        # (the visits kernels: trace_jones_mode_kernel<..., (wgrt::TraceMode)10, ...>, TraceMode::kVisits; the fate pass
        # that chooses the eyebox rows is TraceMode 4 and is not counted)
        want = "trace_jones" if form == "plain" else "TraceMode)10"
        per = {}
        for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                if want in row["Kernel_Name"] and "learn" not in row["Kernel_Name"] and row["Counter_Name"] == counter:
                    k = int(row["Dispatch_Id"])
                    per[k] = per.get(k, 0.0) + float(row["Counter_Value"])
        last = [per[k] for k in sorted(per)[-line["launches"]:]]
        rec[form] = {"dispatches": len(last), "atomic_requests": sum(last), "counts": line["counts"],
                     "requests_per_launch": round(sum(last) / max(len(last), 1), 1)}
    base = rec["plain"]["requests_per_launch"]
    for form in ("visits_eyebox", "visits_all"):
        n = rec[form]["counts"] / max(rec[form]["dispatches"], 1)
        rec[form]["added_requests_per_count"] = round((rec[form]["requests_per_launch"] - base) / max(n, 1), 4)
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--pmc", action="store_true")
    ap.add_argument("--pmc-launches", type=int, default=3)
    ap.add_argument("--child", choices=["plain", "visits_eyebox", "visits_all"], default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("visits_bench.py needs a HIP device")
    if a.child:
        return child(a)
    ctx = _setup(a.config)
    for part in (launches, reductions) + ((pmc,) if a.pmc else ()):
        line = json.dumps(part(a, ctx))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    ctx[4].close()
    ctx[1].close()


if __name__ == "__main__":
    main()
