// wgrt_hits.h -- the hit list: one record per out-coupling of a launch (wgrt_trace_hits), and the rule that bins such
// a list into an eyebox grid of any resolution (wgrt_hits_grid), stated once for the device kernel and its host twin
// wgrt_hits_grid_host.
//
// A record is the out-coupling's position (the ray's at its last draw: the doubles both lanes hand to eyebox_add), the
// ray's global id, its tile index (lambda * nx + m) * ny + n, and flags: bit 0 the result of the FoV's eyebox rectangle
// test (eyebox_inside: fate reason 3 set, 4 clear), bits 16..31 the call's tag.  Two 16-byte halves, so a lane writes a
// record with two 16-byte stores.
//
// The re-binning rule is eyebox_offset (wgrt_exact_lane.h) with kEbNy, kEbNx replaced by H, W, operation by operation:
//     dx = (xmax - xmin) / W,   ix = (int64_t)floor((x - xmin) / dx)     (and the same in y with H),
// a negative index wraps once, an index equal to the axis length aliases through the flat offset
//     off = ((((l * ny + n) * nx + m) * H + iy) * W + ix,
// and the offset is kept iff 0 <= off < num_lmd * ny * nx * H * W.  A subtraction, two IEEE divisions and a floor:
// nothing a compiler could contract, so the device, the twin, numpy and the test-side checker give the same integer for
// the same doubles.  At H = 80, W = 120 over the scene's own ranges it is eyebox_offset itself.
//
// Which records count: over the scene's ranges (ranges == NULL) those whose flag bit 0 is set -- the rectangle test
// the trace made; over caller ranges those with xmin <= x <= xmax && ymin <= y <= ymax, the flag ignored.
#pragma once

#include <cstdint>

#include "../../include/wgrt.h"
#include "wgrt_common.h"

namespace wgrt {

static_assert(sizeof(wgrt_hit) == 32 && alignof(wgrt_hit) == 16, "a record is two 16-byte halves");

constexpr uint32_t kHitInside = 1u;    // flags bit 0
constexpr int kHitTagShift = 16;       // flags bits 16..31
constexpr uint32_t kHitMaxTag = 65535u;
constexpr int kHitsMaxAxis = 4096;     // H, W

WGRT_HD uint32_t hit_flags(bool inside, uint32_t tag) { return (inside ? kHitInside : 0u) | tag << kHitTagShift; }

// NULL, or why the grid's shape is refused (n_slabs = num_lmd * ny * nx).
inline const char *hits_grid_shape_error(int64_t n_slabs, int32_t H, int32_t W) {
    if (H < 1 || H > kHitsMaxAxis || W < 1 || W > kHitsMaxAxis) return "the grid's H and W must be 1 .. 4096";
    if (n_slabs < 1) return "the scene has no tiles";
    if (n_slabs > ((int64_t)1 << 31) / ((int64_t)H * W)) return "a grid of more than 2^31 floats";
    return nullptr;
}

// The flat offset of a hit of tile (l, m, n) at (x, y) in a grid [nl, ny, nx, H, W] over the range r = (xmin, xmax,
// ymin, ymax), or -1 for one outside the buffer: eyebox_offset with (kEbNy, kEbNx) -> (H, W).
WGRT_HD int64_t hits_offset(const double *r, int nl, int nx, int ny, int l, int m, int n, int32_t H, int32_t W, double x,
                            double y) {
    const double xmin = r[0], xmax = r[1], ymin = r[2], ymax = r[3];
    const double dx = (xmax - xmin) / W, dy = (ymax - ymin) / H;
    int64_t ix = (int64_t)floor((x - xmin) / dx);
    int64_t iy = (int64_t)floor((y - ymin) / dy);
    if (ix < 0) ix += W;
    if (iy < 0) iy += H;
    const int64_t off = ((((int64_t)l * ny + n) * nx + m) * H + iy) * W + ix;
    const int64_t total = (int64_t)nl * ny * nx * H * W;
    return (off >= 0 && off < total) ? off : -1;
}

// Record h into the grid: its offset, or -1 when it does not count.  scene_range(tile, m, n): the scene's range of
// the hit's FoV (eff_reg_FOV_range[m, n]; the device reads it from the packed tile, the twin from the host array);
// caller_r: the caller's range array [nx, ny, 4], or NULL.
template <class RangeF>
WGRT_HD int64_t hits_record_offset(const wgrt_hit &h, int nl, int nx, int ny, RangeF scene_range, const double *caller_r,
                                   int32_t H, int32_t W) {
    const uint32_t g = h.tile;
    if ((uint64_t)g >= (uint64_t)nl * (uint64_t)nx * (uint64_t)ny) return -1;
    const int n = (int)(g % (uint32_t)ny), m = (int)(g / (uint32_t)ny % (uint32_t)nx);
    const int l = (int)(g / ((uint32_t)ny * (uint32_t)nx));
    const double *r;
    if (caller_r) {
        r = caller_r + ((int64_t)m * ny + n) * 4;
        if (!(r[0] <= h.x && h.x <= r[1] && r[2] <= h.y && h.y <= r[3])) return -1;
    } else {
        if (!(h.flags & kHitInside)) return -1;
        r = scene_range(g, m, n);
    }
    return hits_offset(r, nl, nx, ny, l, m, n, H, W, h.x, h.y);
}

}  // namespace wgrt
