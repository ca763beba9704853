#!/usr/bin/env python3
"""Do two independent single-trace launches overlap when they sit on two streams? (GPU box; analysis tool)

Two traces of one batch, each with its own RNG states, eyebox grid and counters, in pairs (the ray columns,
which a trace only reads, are one set of tensors: a stream caches its automatic issue order by the columns'
addresses, and two sets alternating on one stream would make the serial mode rebuild it, a 0.24-ms
order_kernel, before every launch):
``serial`` issues both traces of a pair on one non-blocking stream, ``two_stream`` issues one on each of
two non-blocking streams of this process (the launch scratch is keyed by stream, so the launches share
nothing but the scene).  A round is ``--pairs`` pairs issued back to back with one device synchronize at
the end (wall clock); rounds of the two modes alternate, the serial mode first and last, so the serial
rounds among themselves give the probe's own A/A spread.  ``overlaps`` is true when the two-stream median
lies below the serial median by more than that spread: then the runtime runs kernels of two streams of
one process at the same time, and a launch's drain can be covered by the next launch's bulk.

    python tools/overlap_probe.py --config C3 --pairs 50 --rounds 5 --out probe.json   (profiles/chain_probe.json)
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
    ap.add_argument("--pairs", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5, help="two-stream rounds (the serial mode runs one more)")
    ap.add_argument("--out", default=None, help="also write the record to this file")
    a = ap.parse_args(argv)

    import torch
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.configs import CONFIGS, build_inputs
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.distributed import hip_shard_builder, make_shard
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import (STAT, Scene, check_stats, new_stats, reserve,
                                                                           trace_fullcolor)

    w = CONFIGS[a.config]
    dev = torch.device("cuda", 0)
    geom, luts, points = build_inputs(w)
    scene = Scene.from_geometry(geom, luts)
    shard = make_shard(w.nx, w.ny, len(w.lambdas), w.R, 1, 0)
    build = hip_shard_builder(points, w.nx, w.ny, list(w.lambdas), w.R, dev)
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]   # torch's streams are non-blocking ones
    rays, rng0 = build(shard)
    batches = [(rays, rng0.clone(), torch.zeros(scene.eb_shape(), dtype=torch.float32, device=dev), new_stats(dev))
               for _ in range(2)]
    torch.cuda.synchronize()

    def launch(b, s):
        rays, rng, eb, st = batches[b]
        trace_fullcolor(scene, rays, rng, eb, gid_offset=shard.gid.offset, stats=st, stream=s)

    # warm-up, one stream at a time: the scene's first launches learn the tile table (one writer at a time),
    # and each stream allocates its launch scratch on its first launch
    for s in streams:
        reserve(scene, shard.n_rays, 1, stream=s)
        for b in range(2):
            for _ in range(3):
                launch(b, s)
        torch.cuda.synchronize()

    def one_round(two: bool) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.pairs):
            launch(0, streams[0])
            launch(1, streams[1] if two else streams[0])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.pairs * 1e3

    for two in (False, True):   # one untimed round of each mode
        one_round(two)
    serial, twos = [one_round(False)], []
    for _ in range(a.rounds):
        twos.append(one_round(True))
        serial.append(one_round(False))
    for b in range(2):
        check_stats(batches[b][3])
    bounces = int(batches[0][3][STAT.bounces]) + int(batches[1][3][STAT.bounces])
    s_med, t_med = float(np.median(serial)), float(np.median(twos))
    spread = (max(serial) - min(serial)) / s_med
    rec = {"config": a.config, "rays_per_trace": shard.n_rays, "pairs_per_round": a.pairs,
           "hw_queues_env": os.environ.get("GPU_MAX_HW_QUEUES"),
           "serial_ms_per_pair": [round(v, 4) for v in serial], "two_stream_ms_per_pair": [round(v, 4) for v in twos],
           "serial_median_ms": round(s_med, 4), "two_stream_median_ms": round(t_med, 4),
           "serial_aa_spread": round(spread, 4), "two_stream_gain": round(1.0 - t_med / s_med, 4),
           "overlaps": bool(max(twos) < min(serial) and 1.0 - t_med / s_med > spread),
           "bounces_total": bounces,
           "note": "wall ms per pair of independent single traces: both on one stream (serial) against one on each "
                   "of two non-blocking streams; rounds alternate, serial_aa_spread = (max - min) / median of the "
                   "serial rounds; overlaps: every two-stream round below every serial round and the median gain "
                   "above that spread"}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    scene.close()


if __name__ == "__main__":
    main()
