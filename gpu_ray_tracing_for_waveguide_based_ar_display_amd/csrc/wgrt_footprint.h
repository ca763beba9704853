// wgrt_footprint.h -- where on the plate: the binning rule of the interaction / out-coupling footprint maps
// (wgrt_trace_footprint), stated once for both lanes of the state machine, the host twin wgrt_footprint_bin_host and
// (through it) the Python layer.
//
// A map is int64 [num_lmd, kFootprintChannels, ny_cells, nx_cells] over the plan's rectangle of the plate.  A point
// (x, y) of wavelength l and channel c counts into
//     ix = (int64_t)floor((x - x0) / cell_x),   iy = (int64_t)floor((y - y0) / cell_y),
//     offset = ((l * 9 + c) * ny_cells + iy) * nx_cells + ix,
// and is dropped when ix lies outside [0, nx_cells), iy outside [0, ny_cells), or a coordinate is not finite.  The
// rule is a subtraction, an IEEE division and a floor: nothing a compiler could contract, so the device, the host
// twin, numpy and the test-side C checker give the same integer for the same doubles.
//
// Channels.  The position is the ray's at the draw, before the taken branch moves it:
//     0..5  every Monte-Carlo draw of the bounce loop in state R0..R5 (4 after the R3 -> R4 switch, as in the fate
//           code): the draws wgrt_trace_stats.interactions counts; the in-coupling event is not among them;
//     6     the draws that took no branch (fate reason 2): where light is lost;
//     7     the draws that out-coupled the ray inside its FoV's eyebox rectangle (reason 3; the rectangle test, not the
//           aliased store, as the fate);
//     8     the draws that out-coupled it outside the rectangle (reason 4).
// Channels 6..8 are subsets of 0..5 at the same cell.  The counts are integers, so a map does not depend on the order
// of the adds, is the same bits on every run and for every work split, and the maps of shards add up exactly.
#pragma once

#include <cmath>
#include <cstdint>

#include "../../include/wgrt.h"
#include "wgrt_common.h"
#include "wgrt_fate.h"

namespace wgrt {

constexpr int kFootprintChannels = WGRT_FOOTPRINT_CHANNELS;
constexpr int kFootprintLost = 6, kFootprintEyebox = 7, kFootprintBeside = 8;
constexpr int kFootprintMaxCells = 4096;   // per axis

// NULL, or why the plan is refused (wgrt_footprint_plan_validate, wgrt_trace_footprint).
inline const char *footprint_plan_error(const wgrt_footprint_plan *fp) {
    if (!fp) return "NULL footprint plan";
    if (!(fp->x0 - fp->x0 == 0.0) || !(fp->y0 - fp->y0 == 0.0)) return "the footprint plan's origin must be finite";
    if (!(fp->cell_x > 0.0) || !(fp->cell_y > 0.0) || !(fp->cell_x - fp->cell_x == 0.0) ||
        !(fp->cell_y - fp->cell_y == 0.0))
        return "the footprint plan's cell sizes must be > 0 and finite";
    if (fp->nx_cells < 1 || fp->nx_cells > kFootprintMaxCells || fp->ny_cells < 1 || fp->ny_cells > kFootprintMaxCells)
        return "the footprint plan's nx_cells / ny_cells must be 1 .. 4096";
    return nullptr;
}

// The cell of (x, y) within one [ny_cells, nx_cells] slab: iy * nx_cells + ix, or -1 for a point that is dropped.
// (A NaN or infinite quotient fails both range tests below: the comparisons are made on the double.)
WGRT_HD int32_t footprint_cell(const wgrt_footprint_plan &fp, double x, double y) {
    const double fx = floor((x - fp.x0) / fp.cell_x), fy = floor((y - fp.y0) / fp.cell_y);
    if (!(fx >= 0.0 && fx < (double)fp.nx_cells && fy >= 0.0 && fy < (double)fp.ny_cells)) return -1;
    return (int32_t)((int64_t)fy * fp.nx_cells + (int64_t)fx);
}

// The flat offset of (wavelength l, channel c, cell) in the map.
WGRT_HD int64_t footprint_offset(const wgrt_footprint_plan &fp, int l, int c, int32_t cell) {
    return ((int64_t)l * kFootprintChannels + c) * ((int64_t)fp.ny_cells * fp.nx_cells) + cell;
}

// The second channel of a draw that ended its ray's trace with fate reason `reason` (wgrt_fate.h): -1 for none.
WGRT_HD int footprint_end_channel(int reason) {
    return reason == kFateLost ? kFootprintLost : reason == kFateEyebox ? kFootprintEyebox
           : reason == kFateBeside ? kFootprintBeside : -1;
}

inline const char *footprint_channel_name(int c) {
    static const char *const names[kFootprintChannels] = {"R0", "R1", "R2", "R3", "R4", "R5", "lost", "eyebox",
                                                          "beside_eyebox"};
    return c >= 0 && c < kFootprintChannels ? names[c] : nullptr;
}

}  // namespace wgrt
