// wgrt_paths.h -- ray paths: the record a paths launch (wgrt_trace_paths) appends for every draw of a selected ray, the
// rule that says which records a trace leaves, and the reduction of a path list into a footprint map
// (wgrt_paths_footprint), stated once for both lanes of the state machine, the device reduction and its host twin
// wgrt_paths_footprint_host.
//
// A record (wgrt_path_vertex, include/wgrt.h) is the ray's position at the event, its global id, the ordinal `step` of
// the record within the ray's trace, and flags:
//     bits 0..2   the state R0..R5 the ray is in (4 after the R3 -> R4 switch, as the fate code's region);
//     bits 4..7   the kind: 0 a draw after which the trace goes on; 2 a draw that lost the ray (fate reason 2); 3 / 4 a
//                 draw that out-coupled it inside / beside its FoV's eyebox rectangle (reasons 3 / 4); 1 an end record,
//                 the ray left eff_reg1 (reason 1); 5 an end record, the R5 miss (reason 5);
//     bits 8..15  the wavelength index l;
//     bits 16..31 the call's tag.
// Two 16-byte halves, so a lane writes a record with two 16-byte stores.
//
// The rule.  A trace leaves one draw record per Monte-Carlo draw of the bounce loop -- the draws
// wgrt_trace_stats.interactions and footprint channels 0..5 count; the in-coupling event is not one -- at the position
// before the taken branch moves the ray, draw k with step = k (0-based).  A draw at which the in-coupler's second order
// leaves the in-coupler (fate reason 6) is kind 0: it is no Monte-Carlo loss, and the ray's fate tells the rest.  A
// trace that ends by the loop-top eff_reg1 test or by an R5 miss appends one end record at the ray's position there,
// with step = the number of draws the trace made; one that ends at the bounce cap (reason 7) or at the in-coupling
// event appends none.  So (tag, gid, step) is unique, a ray's records sorted by step are its polyline after the start
// point, and the number of its draw records is its interaction count.
//
// The reduction.  A draw record counts into channel `state` of a footprint map through wgrt_footprint.h's own cell
// rule, and one of kind 2 / 3 / 4 also into channel 6 / 7 / 8; end records and records whose l is not below num_lmd
// count nothing.  The list of a launch with every ray selected therefore reduces to wgrt_trace_footprint's map of the
// same launch, bit for bit.
#pragma once

#include <cstdint>

#include "../../include/wgrt.h"
#include "wgrt_common.h"
#include "wgrt_fate.h"
#include "wgrt_footprint.h"

namespace wgrt {

static_assert(sizeof(wgrt_path_vertex) == 32 && alignof(wgrt_path_vertex) == 16, "a record is two 16-byte halves");

constexpr uint32_t kPathStateMask = 7u;   // flags bits 0..2
constexpr int kPathKindShift = 4;         // flags bits 4..7
constexpr int kPathLmdShift = 8;          // flags bits 8..15
constexpr int kPathTagShift = 16;         // flags bits 16..31
constexpr uint32_t kPathMaxTag = 65535u;
constexpr int kPathMaxLmd = 256;          // wavelengths a record can name
constexpr int kPathDraw = 0;              // the kind of a draw after which the trace goes on

WGRT_HD uint32_t path_flags(int state, int kind, int l, uint32_t tag) {
    return (uint32_t)state | (uint32_t)kind << kPathKindShift | (uint32_t)l << kPathLmdShift | tag << kPathTagShift;
}
WGRT_HD int path_state(uint32_t flags) { return (int)(flags & kPathStateMask); }
WGRT_HD int path_kind(uint32_t flags) { return (int)(flags >> kPathKindShift & 15u); }
WGRT_HD int path_lmd(uint32_t flags) { return (int)(flags >> kPathLmdShift & 255u); }

// The kind of a draw from the fate reason of the trace it ended (0: the trace goes on).
WGRT_HD int path_draw_kind(int reason) {
    return reason == kFateLost || reason == kFateEyebox || reason == kFateBeside ? reason : kPathDraw;
}
// Whether a trace that ended with this fate reason outside a draw leaves an end record (whose kind is the reason).
WGRT_HD bool path_end_reason(int reason) { return reason == kFateLeftEff1 || reason == kFateOcMiss; }
WGRT_HD bool path_is_end(int kind) { return kind == kFateLeftEff1 || kind == kFateOcMiss; }

// What a record adds to a footprint map [num_lmd, 9, ny_cells, nx_cells]: the flat offset of its state channel in *a
// and of its lost / eyebox / beside channel in *b, each -1 for none.
WGRT_HD void path_footprint_offsets(const wgrt_footprint_plan &fp, int32_t num_lmd, double x, double y, uint32_t flags,
                                    int64_t *a, int64_t *b) {
    *a = -1;
    *b = -1;
    const int kind = path_kind(flags), l = path_lmd(flags), state = path_state(flags);
    if (path_is_end(kind) || l >= num_lmd || state > 5) return;
    const int32_t cell = footprint_cell(fp, x, y);
    if (cell < 0) return;
    *a = footprint_offset(fp, l, state, cell);
    const int c2 = footprint_end_channel(kind);
    if (c2 >= 0) *b = footprint_offset(fp, l, c2, cell);
}

}  // namespace wgrt
