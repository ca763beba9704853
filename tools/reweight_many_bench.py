#!/usr/bin/env python3
"""K what-if tables from one visits launch: the batched reduction against the loop it replaces, timed on the GPU box
(analysis tool).

On a bench configuration (default C3) one visits launch fills the rows of the delivered rays.  Then, for K in --designs
(default 1, 16, 64, 256) tolerance designs (sigma 0.05), --rounds rounds alternate, in one session, after one warm-up of
each:
  many_interleaved   wgrt_visits_reweight_many with its deposits through the scratch interleaved over a chunk's designs,
                     the operator called with the log-scales already on the device (device time of the kernels);
  many_direct        the same with the deposits straight into out [K, n_slabs, W];
  many_call          VisitTable.reweight_many as the driver calls it (the shipped form; with the host's preparation of
                     the log-scales);
  loop               K VisitTable.reweight calls plus K VisitTable.weight_sums calls: what a caller had before;
  loop_kernels       the K single kernels alone, log-scales already on the device, no weight sums: the loop's floor;
  evaluate           evaluation_ensemble of the K tables on the device.
HIP events around each; per kind the median, min and max ms and the spread (max - min) / median.  Every table of every
batched form is compared with the loop's (equal bytes).  One time limit (--time-limit seconds) covers the whole run and
nothing is started after a failure: any exception ends the run.

One JSON line per K.    python tools/reweight_many_bench.py --out profiles/reweight_many_bench.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import signal
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def _summary(ms):
    med = statistics.median(ms)
    return {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "spread": round((max(ms) - min(ms)) / med, 4)}


def _timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--designs", default="1,16,64,256")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--time-limit", type=int, default=480, help="seconds for the whole run")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("reweight_many_bench.py needs a HIP device")
    signal.alarm(a.time_limit)   # the one limit: SIGALRM ends the process

    from gpu_ray_tracing_for_waveguide_based_ar_display_amd import _lib
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.AR_system_evaluation_functions import evaluation_ensemble
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import (VisitTable, _lnscale_many, _stream_handle,
                                                                           tolerance_scales, trace_fullcolor)
    from tools.visits_bench import _rows, _setup
    ctx = _setup(a.config)
    dev, scene, rays, rng0, plan = ctx
    _, slot, n = _rows(ctx)
    vt = VisitTable(scene, n, dev)
    table = plan.new_table(scene)
    trace_fullcolor(scene, rays, rng0.clone(), None, windows=(plan, table), visits=(vt, slot))
    torch.cuda.synchronize()
    n_slabs, W = table.shape
    nonzero = float((vt.counts != 0).sum().item()) / max(n, 1)
    shape, divisor = scene.eb_shape(), 1
    handle = lambda: _stream_handle(dev, None)
    for K in (int(v) for v in a.designs.split(",")):
        scales = tolerance_scales(vt.channels, 0.05, max(K, 2))[:K]
        ln = _lnscale_many(vt.channels, scales).to(dev)
        out = torch.zeros((K, n_slabs, W), dtype=torch.float64, device=dev)
        sums = torch.zeros((K, 2, scene.num_lmd), dtype=torch.int64, device=dev)
        loop_out = torch.zeros_like(out)

        def many_op():
            _lib.check(_lib.ops().visits_reweight_many(scene.handle.value, plan.handle.value, vt.counts, vt.ends, vt.n_rows,
                                                       ln, out, sums, handle()), "wgrt_visits_reweight_many")

        def loop():
            for k in range(K):
                vt.reweight(plan, scales[k], out=loop_out[k])
                vt.weight_sums(scales[k])

        def loop_kernels():
            for k in range(K):
                _lib.check(_lib.ops().visits_reduce(scene.handle.value, plan.handle.value, vt.counts, vt.ends, vt.n_rows,
                                                    ln[k], loop_out[k], handle()), "wgrt_visits_reweight")

        kinds = {"many_interleaved": (True, many_op), "many_direct": (False, many_op),
                 "many_call": (True, lambda: vt.reweight_many(plan, scales, out=out, sums=sums)),
                 "loop": (None, loop), "loop_kernels": (None, loop_kernels),
                 "evaluate": (None, lambda: evaluation_ensemble(out, shape, divisor, "device"))}
        loop()   # the reference tables, and the loop's warm-up
        torch.cuda.synchronize()
        want = loop_out.clone()
        equal = {}
        for name, (layout, fn) in kinds.items():   # warm-up, and every batched form against the loop
            if layout is not None:
                _lib.set_reweight_layout(layout)
                out.zero_()
            fn()
            torch.cuda.synchronize()
            if layout is not None:
                equal[name] = bool(torch.equal(out, want))
        ms = {name: [] for name in kinds}
        for _ in range(a.rounds):   # alternating: every kind once per round
            for name, (layout, fn) in kinds.items():
                if layout is not None:
                    _lib.set_reweight_layout(layout)
                    out.zero_()
                    sums.zero_()
                elif name != "evaluate":
                    loop_out.zero_()
                if name == "evaluate" and not out.any():
                    out.copy_(want)
                ms[name].append(_timed(fn))
        _lib.set_reweight_layout(True)
        rec = {"tool": "reweight_many_bench", "config": a.config, "device": torch.cuda.get_device_name(0), "K": K,
               "rows": n, "channels": vt.n_channels, "nonzero_counts_per_row": round(nonzero, 2),
               "table_entries": int(n_slabs * W), "tables_bytes": int(out.numel() * 8), "rounds": a.rounds,
               "equal_to_loop": equal}
        for name in kinds:
            rec[name] = _summary(ms[name])
        rec["loop_over_many_interleaved"] = round(rec["loop"]["median_ms"] / rec["many_interleaved"]["median_ms"], 2)
        rec["loop_over_many_direct"] = round(rec["loop"]["median_ms"] / rec["many_direct"]["median_ms"], 2)
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        del out, loop_out, want
    signal.alarm(0)
    plan.close()
    scene.close()


if __name__ == "__main__":
    main()
