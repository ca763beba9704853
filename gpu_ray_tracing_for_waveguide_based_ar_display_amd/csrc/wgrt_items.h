// wgrt_items.h -- the work items of a Jones-vector launch, stated once for the device AND the host: which
// (run, chunk) position q of head x's queue stands for.  The wave loop (jones_body, wgrt_trace.hip) decodes
// every dequeue through item_decode; the host hooks (wgrt_debug_fused_items_host, wgrt_debug_fused_partition_host)
// run the same code, so the mapping is checked without a GPU (tests/test_fused_items.py,
// tests/test_fused_partition.py), as wgrt_order.h and wgrt_window.h are shared.
//
// Head x hands out the stripes s = x, x + 8, ... of kStripe consecutive chunks, in order.  A fused launch
// (n_iter chained traces of every ray) repeats that list once per RUN of consecutive traces, run-major: every
// item of run r precedes every item of run r + 1 on its head, which is what the hand-off's forward-progress
// argument rests on (wgrt_trace.hip, kHandoffTicksPerIter).  The runs are a partition of [0, n_iter) fixed by
// (n_iter, S, t0) -- the functions below; S = 1 is one item per (trace, chunk); a single launch is n_iter = S = 1.
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

// The runs of a fused launch: a partition of its traces [0, n) into consecutive runs, fixed by n, the main run S
// (a power of two) and the first tail length t0 (a power of two below S, or 0).
//   t0 = 0   runs of S aligned at multiples of S from 0; the short run, if any, is the last.
//   t0 > 0   the TAPER: the last 2 t0 - 1 traces are the runs of t0, t0 / 2, ..., 2, 1 traces, so each level's
//            drain lies under the next level's bulk and only a one-trace run drains with nothing behind it.  The
//            traces before T = n - (2 t0 - 1) are runs of S aligned from T backwards; the short run, if any, is
//            the first, [0, T mod S): its drain lies under the whole launch.  A launch shorter than the tail keeps
//            the tail's last runs, the first of them clipped at 0.
// Both are one form: the head [0, T) holds runs of S whose first traces are = a (mod S), clipped to [0, n), with
// (T, a) = (n, 0) without the taper and (max(n - (2 t0 - 1), 0), T mod S) with it; a trace d = n - k before the end
// of the tail lies in the run of length p = 2^floor(log2 d), which ends p - 1 traces before n.  Everything is
// closed-form in 32 bits, so a lane derives its run from the trace it is at and holds no register for it, and the
// publisher of a run's last trace and the waiter for the next run's first trace read one boundary.
WGRT_ITEMS_HD uint32_t part_log2(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }   // floor(log2 v), v > 0
WGRT_ITEMS_HD uint32_t part_tail(uint32_t n, uint32_t t0) {   // T: the first trace of the tail (n: no tail)
    const uint32_t lt = t0 ? 2u * t0 - 1u : 0u;
    return n > lt ? n - lt : 0u;
}
WGRT_ITEMS_HD uint32_t part_align(uint32_t n, uint32_t S, uint32_t t0) {   // a: the head's runs start at a (mod S)
    return t0 ? part_tail(n, t0) & (S - 1u) : 0u;
}
WGRT_ITEMS_HD uint32_t part_head_runs(uint32_t n, uint32_t S, uint32_t t0) {
    return (part_tail(n, t0) + S - 1u) >> part_log2(S);
}
// the number of runs
WGRT_ITEMS_HD uint32_t part_runs(uint32_t n, uint32_t S, uint32_t t0) {
    uint32_t tail = 0u;
    if (t0) {
        const uint32_t a = part_log2(t0), b = part_log2(n);
        tail = (a < b ? a : b) + 1u;
    }
    return part_head_runs(n, S, t0) + tail;
}
// the first trace of run r (r < part_runs)
WGRT_ITEMS_HD uint32_t part_run_first(uint32_t r, uint32_t n, uint32_t S, uint32_t t0) {
    const uint32_t h = part_head_runs(n, S, t0);
    int32_t f;
    if (r < h) {
        const uint32_t a = part_align(n, S, t0);
        f = (int32_t)a + ((int32_t)r - (a ? 1 : 0)) * (int32_t)S;
    } else {
        const uint32_t j = part_runs(n, S, t0) - 1u - r;   // the run of 2^j traces
        f = (int32_t)n - (int32_t)((2u << j) - 1u);
    }
    return f > 0 ? (uint32_t)f : 0u;
}
// the first and the end trace of the run that holds trace k (k < n)
WGRT_ITEMS_HD void part_span(uint32_t k, uint32_t n, uint32_t S, uint32_t t0, uint32_t &first, uint32_t &end) {
    int32_t f;
    if (k < part_tail(n, t0)) {
        f = (int32_t)k - (int32_t)((k - part_align(n, S, t0)) & (S - 1u));
        const uint32_t e = (uint32_t)(f + (int32_t)S);
        end = e < n ? e : n;
    } else {
        const uint32_t p = 1u << part_log2(n - k);
        f = (int32_t)n - (int32_t)(2u * p - 1u);
        end = n - (p - 1u);
    }
    first = f > 0 ? (uint32_t)f : 0u;
}
WGRT_ITEMS_HD uint32_t run_first(uint32_t k, uint32_t n, uint32_t S, uint32_t t0) {
    uint32_t f, e;
    part_span(k, n, S, t0, f, e);
    return f;
}
WGRT_ITEMS_HD uint32_t run_end(uint32_t k, uint32_t n, uint32_t S, uint32_t t0) {
    uint32_t f, e;
    part_span(k, n, S, t0, f, e);
    return e;
}

// The RUN WORD a lane of a fused launch carries in the 32 bits of its trace number: the trace it is at in the low
// byte, and the first and the end trace of the run that holds it in the next two (a launch has at most 255 traces).
// The dequeue makes it from the partition, wave-uniform, for the item's first trace; a restart inside the run adds 1.
// So a lane asks the partition nothing where its registers are scarcest -- where a trace ends -- and the publisher of
// a run's last trace and the waiter for the next run's first read the one boundary item_decode derived.
WGRT_ITEMS_HD uint32_t run_word(uint32_t k0, uint32_t end) { return k0 | k0 << 8 | end << 16; }
WGRT_ITEMS_HD uint32_t word_trace(uint32_t w) { return w & 0xffu; }
WGRT_ITEMS_HD uint32_t word_first(uint32_t w) { return (w >> 8) & 0xffu; }
WGRT_ITEMS_HD uint32_t word_end(uint32_t w) { return w >> 16; }

// Position q of head x's queue -> chunk c and first trace k0 of the item; false past the head's last item.
// ns stripes, the last of `last` chunks (n_chunks = (ns - 1) * kItemStripe + last); n_runs = part_runs(n_iter, run,
// t0): item q of the head is run q / cx of chunk q % cx of the head's list, and k0 that run's first trace.
template <bool FUSED>
WGRT_ITEMS_HD bool item_decode(int64_t ns, int64_t last, int64_t n_runs, uint32_t n_iter, uint32_t run, uint32_t t0, int x,
                               int64_t q, int64_t &c, uint32_t &k0) {
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
    k0 = FUSED ? part_run_first((uint32_t)kk, n_iter, run, t0) : 0u;
    const int64_t r = q - kk * cx;
    c = ((r / kItemStripe) * kItemHeads + x) * kItemStripe + r % kItemStripe;
    return true;
}

}  // namespace wgrt
