// wgrt_items.h -- the work items of a Jones-vector launch, stated once for the device AND the host: which
// (run, chunk) position q of head x's queue stands for.  The wave loop (jones_body, wgrt_trace.hip) decodes
// every dequeue through item_decode; the host hook (wgrt_debug_fused_items_host) runs the same code, so the
// mapping is checked without a GPU (tests/test_fused_items.py), as wgrt_order.h and wgrt_window.h are shared.
//
// Head x hands out the stripes s = x, x + 8, ... of kStripe consecutive chunks, in order.  A fused launch
// (n_iter chained traces of every ray) repeats that list once per RUN of `run` consecutive traces
// [k0, min(k0 + run, n_iter)), k0 = 0, run, 2 run, ..., run-major: every item of run r precedes every item of
// run r + 1 on its head, which is what the hand-off's forward-progress argument rests on (wgrt_trace.hip,
// kHandoffTicksPerIter).  run = 1 is one item per (trace, chunk); a single launch is n_iter = run = 1.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define WGRT_ITEMS_HD __host__ __device__ __forceinline__
#else
#define WGRT_ITEMS_HD inline
#endif

namespace wgrt {

constexpr int kItemHeads = 8;
#ifndef WGRT_STRIPE
#define WGRT_STRIPE 16
#endif
constexpr int64_t kItemStripe = WGRT_STRIPE;   // chunks per stripe of the work queue (1024 rays: one C3 tile)
constexpr int kMaxFusedRun = 64;               // the longest run (wgrt_debug_set_fused_run)

// The traces of a fused launch after trace k that belong to k's run end before run_end(k): run is a power of
// two, so a lane derives its run's end from the trace it is at and holds no register for it.
WGRT_ITEMS_HD uint32_t run_end(uint32_t k, uint32_t run, uint32_t n_iter) {
    const uint32_t e = (k | (run - 1u)) + 1u;
    return e < n_iter ? e : n_iter;
}

// Position q of head x's queue -> chunk c and first trace k0 of the item; false past the head's last item.
// ns stripes, the last of `last` chunks (n_chunks = (ns - 1) * kItemStripe + last); n_runs = ceil(n_iter / run).
template <bool FUSED>
WGRT_ITEMS_HD bool item_decode(int64_t ns, int64_t last, int64_t n_runs, uint32_t run, int x, int64_t q, int64_t &c,
                               uint32_t &k0) {
    if (x >= ns) return false;
    int64_t cx = ((ns - x + kItemHeads - 1) / kItemHeads) * kItemStripe;
    if ((ns - 1) % kItemHeads == x) cx -= kItemStripe - last;
    if (q >= cx * n_runs) return false;
    // the item's run: 0 for a single trace; else q / cx (< 256) from a double quotient,
    // corrected -- no 64-bit integer division on the dequeue path
    int64_t kk = 0;
    if (FUSED) {
        kk = (int64_t)((double)q / (double)cx);
        kk -= kk * cx > q;
        kk += (kk + 1) * cx <= q;
    }
    k0 = (uint32_t)kk * (FUSED ? run : 1u);
    const int64_t r = q - kk * cx;
    c = ((r / kItemStripe) * kItemHeads + x) * kItemStripe + r % kItemStripe;
    return true;
}

}  // namespace wgrt
