// wgrt_window.h -- window membership of an eyebox bin, stated once for the device AND the host: which
// entries of the pupil-window table [n_slabs, W] (the layout wgrt_eyebox_window_sums writes, include/wgrt.h)
// one out-coupling into flat grid offset `off` counts into.  The trace kernels' second sink (eyebox_add,
// wgrt_exact_lane.h; wgrt_trace_windows) and the host hook (wgrt_window_table_host, wgrt_eyebox_host.cpp)
// both go through window_visit, so a table accumulated hit by hit equals the window sums of the grid the
// same hits would have left: the counts are integers and the sums linear in the grid.
//
// `off` is the offset eyebox_add computes: after the negative-index wrap, with ix == 120 aliased into the
// next row and iy == 80 into the next slab (compiled-numba addressing, GRTF:164), and inside [0, total).
// The slab comes from `off`, not from the ray's tile, so the aliased hits land where the grid's would.
#pragma once

#include "wgrt_common.h"

namespace wgrt {

constexpr int kWinMaxMs = kEbNy;          // 1 <= ms <= 80 (as wgrt_eyebox_window_sums)
constexpr int kWinRowWords = 3;           // bit words per mask row (96 >= 80 taps)
constexpr int64_t kEbSlabCells = (int64_t)kEbNy * kEbNx;

// A plan as the sink reads it (the device copy lives in global memory behind wgrt_window_plan): the window
// grid and the mask as one bit per tap, bit c of row r at bits[r * kWinRowWords + c / 32] >> (c % 32).
struct WindowPlanView {
    int32_t ms, step_y, step_x, npy, npx, W;
    int32_t pad_[2];
    uint32_t bits[kWinMaxMs * kWinRowWords];
};

// Builds the view of plan (mask [ms * ms], step_y, step_x); returns NULL, or why the plan is refused.  The
// sink adds exactly 1.0 per tap, so every tap must be exactly 0 or 1 (wgrt_eyebox_window_sums serves any
// other mask from a grid).
inline const char *window_plan_view(const float *mask, int32_t ms, int32_t step_y, int32_t step_x,
                                    WindowPlanView &v) {
    if (ms < 1 || ms > kWinMaxMs) return "need 1 <= ms <= 80";
    if (step_y < 1 || step_x < 1) return "need step_y >= 1 and step_x >= 1";
    if (!mask) return "NULL mask";
    v = WindowPlanView{};
    v.ms = ms;
    v.step_y = step_y;
    v.step_x = step_x;
    v.npy = (kEbNy - ms) / step_y + 1;
    v.npx = (kEbNx - ms) / step_x + 1;
    v.W = 1 + v.npy * v.npx;
    for (int r = 0; r < ms; ++r)
        for (int c = 0; c < ms; ++c) {
            const float m = mask[r * ms + c];
            if (m == 1.0f) v.bits[r * kWinRowWords + (c >> 5)] |= 1u << (c & 31);
            else if (!(m == 0.0f)) return "the window sink takes a binary mask: every tap exactly 0.0 or 1.0";
        }
    return nullptr;
}

// add(k) for every table entry k that a hit at grid offset off counts into: the slab's total, then every
// window (wy, wx) with wy*step_y <= r < wy*step_y + ms, wx*step_x <= c < wx*step_x + ms and the tap
// mask[r - wy*step_y, c - wx*step_x] set, (r, c) the bin's row and column in its slab.  off >= 0.
template <class F>
WGRT_HD void window_visit(const WindowPlanView &P, int64_t off, F add) {
    const int64_t s = off / kEbSlabCells;
    const int cell = (int)(off - s * kEbSlabCells);
    const int r = cell / kEbNx, c = cell - r * kEbNx;
    const int ms = P.ms, sy = P.step_y, sx = P.step_x, npx = P.npx;
    const int64_t row = s * P.W;
    add(row);
    // wy * sy <= r  and  r - wy * sy <= ms - 1
    int wy_hi = r / sy, wx_hi = c / sx;
    if (wy_hi > P.npy - 1) wy_hi = P.npy - 1;
    if (wx_hi > npx - 1) wx_hi = npx - 1;
    const int wy_lo = r >= ms ? (r - ms) / sy + 1 : 0;
    const int wx_lo = c >= ms ? (c - ms) / sx + 1 : 0;
    for (int wy = wy_lo; wy <= wy_hi; ++wy) {
        const uint32_t *bits = P.bits + (r - wy * sy) * kWinRowWords;
        for (int wx = wx_lo; wx <= wx_hi; ++wx) {
            const int tc = c - wx * sx;
            if ((bits[tc >> 5] >> (tc & 31)) & 1u) add(row + 1 + wy * npx + wx);
        }
    }
}

}  // namespace wgrt

// The plan behind the opaque handle of include/wgrt.h: the view on the host and its copy on `device`.
struct wgrt_window_plan {
    int device = 0;
    wgrt::WindowPlanView host;
    wgrt::WindowPlanView *d_view = nullptr;
};
