#!/usr/bin/env python3
"""What the driver does with the eyebox grid after the trace, timed on the GPU box (analysis tool).

On a synthetic integer-valued grid at 2 % occupancy, filled on the device, at the reference's default job
(3 x 75 x 100 slabs, 864 MB) and at C3 (3 x 21 x 21, 51 MB), one JSON line per shape with

  (a) window_sums   wgrt_eyebox_window_sums over the whole grid (eyebox_window_sums);
  (b) torch_perceive the torch branch of eye_perceive on the same tensor (56 masked multiply-and-sum passes);
  (c) sum_floor     eb.sum(dim=(-1, -2)): a read of the same bytes, the floor (a) is held against;
  (d) host_post     wall time of the driver's host mode after the trace: eb.cpu(), the slab sums, the scaling
                    and evaluation() (MAIN:186-198);
      device_post   the same quantities in device mode: (a), its 57 doubles per slab copied back, and
                    evaluation_from_perceive;
      device_eval_post  the same in device mode with --evaluate device: (a), (e) with the centre image, and the
                    slab totals, three figures and centre image copied back;
  (e) evaluate      wgrt_eyebox_evaluate on the table of (a) (evaluation_from_window_sums' device path, through
                    the raw call so that no copy is timed): with the full image, the centre image, no image;
      host_colour_s wall time of the host colour math (e) replaces, evaluation_from_perceive on the copied-back
                    table, in this process.

(a)-(c), (e): HIP events around each of --repeats calls after --warmup calls, all in this process; median, min
and max in ms.  (d): wall clock around --post-repeats runs (seconds each; the host evaluation of the default
grid takes several seconds).  The kernel's result is compared with (b)'s once per shape (integer counts: equal
after the cast to float32), (e)'s with the host colour math.

    python tools/eval_bench.py --out profiles/eval_bench.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = {"default": (3, 75, 100), "C3": (3, 21, 21)}


def fill_grid(shape, device, occupancy=0.02, seed=0):
    """Counts 1..39 on ``occupancy`` of the bins, zero elsewhere, generated on the device slab row by row."""
    import torch
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    eb = torch.empty(shape + (80, 120), dtype=torch.float32, device=device)
    for part in eb:   # one wavelength at a time: the temporaries stay a third of the grid
        hit = torch.rand(part.shape, generator=g, device=device) < occupancy
        cnt = torch.randint(1, 40, part.shape, generator=g, device=device).to(torch.float32)
        part.copy_(torch.where(hit, cnt, torch.zeros_like(cnt)))
    return eb


def event_times(fn, warmup, repeats):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def raw_evaluate(E, sums, shape, divisor):
    """``form -> callable`` launching wgrt_eyebox_evaluate on the device table ``sums`` into buffers allocated
    here once (what evaluation_from_window_sums does, without its copies back), and the buffers."""
    import ctypes

    import torch
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd._lib import check, load
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import _stream_handle
    L = load()
    dev = sums.device
    npy, npx = E.window_grid()
    n_fov, n_pos = shape[1] * shape[2], npy * npx
    wl, lab = E._evaluate_consts()
    vp = ctypes.c_void_p
    ws = torch.empty(int(L.wgrt_eyebox_evaluate_workspace_bytes(n_fov, n_pos)), dtype=torch.uint8, device=dev)
    out = torch.empty(3 + n_pos, dtype=torch.float64, device=dev)
    img = {"all": torch.empty((n_fov, 3, n_pos), dtype=torch.float32, device=dev),
           "center": torch.empty((n_fov, 3), dtype=torch.float32, device=dev), "none": None}
    pos = {"all": -1, "center": npx - 1, "none": -1}

    def call(form):
        check(L.wgrt_eyebox_evaluate(sums.data_ptr(), n_fov, n_pos, float(divisor), wl.ctypes.data_as(vp),
                                     lab.ctypes.data_as(vp), out.data_ptr(),
                                     img[form].data_ptr() if img[form] is not None else None, pos[form],
                                     ws.data_ptr(), _stream_handle(dev)), "wgrt_eyebox_evaluate")
    return call, out, img, ws


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", nargs="+", default=["default", "C3"], choices=sorted(SHAPES))
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--post-repeats", type=int, default=3)
    ap.add_argument("--rays-per-fov", type=int, default=5000)
    ap.add_argument("--num-iter", type=int, default=4)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args(argv)

    import torch
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd import AR_system_evaluation_functions as E
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench.py needs a HIP device")
    dev = torch.device("cuda", 0)
    R, K = a.rays_per_fov, a.num_iter
    for name in a.shapes:
        shape = SHAPES[name]
        eb = fill_grid(shape, dev)
        n_slabs = shape[0] * shape[1] * shape[2]
        num_rays = n_slabs * R
        rec = {"tool": "eval_bench", "shape": name, "grid": list(shape) + [80, 120], "grid_bytes": eb.numel() * 4,
               "occupancy": round(float((eb != 0).float().mean()), 5), "device": torch.cuda.get_device_name(0),
               "warmup": a.warmup, "repeats": a.repeats}
        # the kernel's result against the torch branch (integer counts: exact in float32 and float64)
        sums = E.eyebox_window_sums(eb)
        ref = E.eye_perceive(eb)
        got = sums[:, 1:].cpu().numpy().reshape(ref.shape)
        rec["matches_torch_perceive"] = bool(np.array_equal(got.astype(np.float32), ref))
        rec["matches_sum"] = bool(torch.equal(sums[:, 0].to(torch.float32), eb.sum(dim=(-1, -2)).reshape(-1)))
        rec["window_sums"] = event_times(lambda: E.eyebox_window_sums(eb), a.warmup, a.repeats)
        rec["sum_floor"] = event_times(lambda: eb.sum(dim=(-1, -2)), a.warmup, a.repeats)
        rec["torch_perceive"] = event_times(lambda: E.eye_perceive(eb), a.warmup, a.repeats)
        rec["window_sums_over_sum_floor"] = round(rec["window_sums"]["median_ms"] / rec["sum_floor"]["median_ms"], 3)
        rec["window_sums_GBps"] = round(rec["grid_bytes"] / rec["window_sums"]["median_ms"] / 1e6, 1)
        rec["sum_floor_GBps"] = round(rec["grid_bytes"] / rec["sum_floor"]["median_ms"] / 1e6, 1)
        # (e): the evaluation of the table on the device
        call, ev_out, ev_img, ev_ws = raw_evaluate(E, sums, shape, R * K)
        rec["table_bytes"] = sums.numel() * 8
        rec["image_bytes"] = ev_img["all"].numel() * 4
        rec["workspace_bytes"] = ev_ws.numel()
        for form in ("all", "center", "none"):
            rec[f"evaluate_{form}"] = event_times(lambda: call(form), a.warmup, a.repeats)
        host, d2h, device, device_eval, colour = [], [], [], [], []
        for _ in range(a.post_repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m = eb.cpu().numpy()
            t1 = time.perf_counter()
            A = np.sum(m, axis=(-2, -1)) / num_rays / K
            ev = E.evaluation(m / R / K)
            host.append(time.perf_counter() - t0)
            d2h.append(t1 - t0)
            del m
            t0 = time.perf_counter()
            s = E.eyebox_window_sums(eb).cpu().numpy()
            A_d = s[:, 0].reshape(shape).astype(np.float32) / num_rays / K
            t1 = time.perf_counter()
            ev_d = E.evaluation_from_perceive(E.perceive_from_window_sums(s, shape, R * K))
            device.append(time.perf_counter() - t0)
            colour.append(time.perf_counter() - t1)
            t0 = time.perf_counter()
            sd = E.eyebox_window_sums(eb)
            A_e = sd[:, 0].cpu().numpy().reshape(shape).astype(np.float32) / num_rays / K
            ev_e = E.evaluation_from_window_sums(sd, shape + (80, 120), R * K, image="center")
            device_eval.append(time.perf_counter() - t0)
        rec["A_bit_identical"] = bool(A.tobytes() == A_d.tobytes())
        rec["evaluation_diff"] = [float(ev_d[k] - ev[k]) for k in range(3)]
        rec["host_post_s"] = [round(v, 4) for v in host]
        rec["host_post_d2h_s"] = [round(v, 4) for v in d2h]
        rec["device_post_s"] = [round(v, 4) for v in device]
        rec["host_colour_s"] = [round(v, 4) for v in colour]
        rec["device_eval_post_s"] = [round(v, 4) for v in device_eval]
        rec["device_eval_A_bit_identical"] = bool(A_e.tobytes() == A_d.tobytes())
        rec["device_eval_rel_diff"] = [float(abs(ev_e[k] - ev_d[k]) / abs(ev_d[k])) if ev_d[k] else float(abs(ev_e[k]))
                                       for k in range(3)]
        n_epx = ev_d[3].shape[4]
        rec["device_eval_center_max_diff"] = float(np.max(np.abs(ev_e[3] - ev_d[3][:, :, :, 0, n_epx - 1])))
        rec["host_colour_over_evaluate_center"] = round(
            statistics.median(colour) * 1e3 / rec["evaluate_center"]["median_ms"], 1)
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        del eb
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
