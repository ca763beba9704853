// wgrt_order.h -- the arithmetic of the work queue's automatic issue order, shared by the device kernel
// that builds it (wgrt_trace.hip: order_kernel) and the host entry point that runs the same code for a CPU
// test (wgrt_debug_order_host), as wgrt_pack.h is shared.
//
// A launch's 64-ray chunks are issued in descending classes of their tile's tail count (the rays of that
// (wavelength, FoV) tile that lived longer than kLongBounces bounces in the learning launches), so the
// chains that end a launch start early.  The sort is a stable two-pass radix sort of the class keys over
// kOrderThreads workers, each owning a contiguous range of positions: chunks of one class keep their
// natural order, so a tile's 16 consecutive chunks stay adjacent (one stripe of the work queue).
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WGRT_ORDER_HD __host__ __device__ inline
#else
#define WGRT_ORDER_HD inline
#endif

namespace wgrt {

// A trace with more bounces than this counts into its tile's tail.  C3 measured the same with 24 and 30
// (profiles/order_ab_C3.log); 24 keeps ten times the counts, so one 1024-ray launch ranks the tiles.
constexpr uint32_t kLongBounces = 24;
// A scene learns until this many rays per tile have been traced by learning launches.
constexpr int64_t kLearnRaysPerTile = 1024;
// Classes of the order.  Few classes lose the gain: on C3 8 linear classes measured nothing, 16 half of
// the exact order's -2.5 % (profiles/order_ab_C3.log); 256 is the exact order up to a count of 255.
constexpr int kOrderClasses = 256;
constexpr int kOrderDigitBits = 4, kOrderDigits = 1 << kOrderDigitBits, kOrderPasses = 2;
static_assert(kOrderDigits * kOrderDigits == kOrderClasses, "two digits make a class key");
constexpr int kOrderThreads = 256;

// The sort key of a chunk whose tile has `count` of the table's largest count `max_count`: 0 first.
// A chunk of no tile (out-of-range FoV / wavelength index) passes count 0: the lowest class.
WGRT_ORDER_HD uint32_t order_key(uint32_t count, uint32_t max_count) {
    if (max_count == 0u) return (uint32_t)kOrderClasses - 1u;
    uint64_t cls = (uint64_t)count * (uint64_t)(kOrderClasses - 1) / (uint64_t)max_count;
    if (cls > (uint64_t)(kOrderClasses - 1)) cls = (uint64_t)(kOrderClasses - 1);   // a count read past the max
    return (uint32_t)(kOrderClasses - 1) - (uint32_t)cls;
}

WGRT_ORDER_HD uint32_t order_digit(uint32_t key, int pass) {
    return (key >> (pass * kOrderDigitBits)) & (uint32_t)(kOrderDigits - 1);
}

// Worker t's positions [lo, hi) of n.
WGRT_ORDER_HD void order_range(int t, int64_t n, int64_t &lo, int64_t &hi) {
    const int64_t per = (n + kOrderThreads - 1) / kOrderThreads;
    lo = (int64_t)t * per < n ? (int64_t)t * per : n;
    hi = lo + per < n ? lo + per : n;
}

// The chunk at position p going into `pass`: pass 0 reads the natural order.
WGRT_ORDER_HD int32_t order_src(const int32_t *src, int pass, int64_t p) {
    return pass == 0 ? (int32_t)p : src[p];
}

// Step 1 of a pass: worker t counts its positions' digits into hist[digit * kOrderThreads + t].
template <class Hist>
WGRT_ORDER_HD void order_count(int t, int pass, int64_t n, const uint32_t *keys, const int32_t *src, Hist hist) {
    int64_t lo, hi;
    order_range(t, n, lo, hi);
    for (int d = 0; d < kOrderDigits; ++d) hist[d * kOrderThreads + t] = 0;
    for (int64_t p = lo; p < hi; ++p) hist[order_digit(keys[order_src(src, pass, p)], pass) * kOrderThreads + t] += 1;
}
// Step 2 (between the two, by the caller): hist becomes its exclusive prefix sum in index order, so
// hist[d * kOrderThreads + t] is where worker t's first chunk of digit d goes.
// Step 3: worker t places its chunks, in order.
template <class Hist>
WGRT_ORDER_HD void order_place(int t, int pass, int64_t n, const uint32_t *keys, const int32_t *src, Hist hist,
                               int32_t *dst) {
    int64_t lo, hi;
    order_range(t, n, lo, hi);
    for (int64_t p = lo; p < hi; ++p) {
        const int32_t c = order_src(src, pass, p);
        const uint32_t slot = order_digit(keys[c], pass) * kOrderThreads + t;
        dst[hist[slot]] = c;
        hist[slot] += 1;
    }
}

}  // namespace wgrt
