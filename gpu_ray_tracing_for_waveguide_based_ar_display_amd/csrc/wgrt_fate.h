// wgrt_fate.h -- where a ray ends, stated once: the per-ray fate code both lanes of the state machine store
// (wgrt_trace_fate), the reasons' names, which codes exist, and the census table's column of a code
// (wgrt_fate_census, its host twin, the C header's WGRT_FATE_COLS and -- through wgrt_fate_col /
// wgrt_fate_reason_name -- the Python layer).  The code is the CPU oracle's (oracle/wgrt_oracle.c trace_one):
//     code = 10 * region + reason,
// region the state R0..R5 the ray is in when its trace ends (4 after the R3 -> R4
// switch), 9 for the in-coupling event (GRTF:860-904), and
//     1  left eff_reg1 (GRTF:906)                       5  missed every out-coupler slice in R5 (GRTF:1244-1246)
//     2  Monte-Carlo loss: the draw took no branch      6  the in-coupler's second order left the in-coupler
//     3  out-coupled inside the FoV's eyebox rectangle  7  range(100000) exhausted (GRTF:905)
//     4  out-coupled outside it
// Code 0 is "no trace": a ray skipped for an m / n / lmd_num outside the scene.  An out-coupling whose aliased
// grid offset falls outside the buffer (GRTF:164) is still reason 3: the reason follows the rectangle test, not
// the store.
#pragma once

#include <cstdint>

#include "wgrt_common.h"

namespace wgrt {

enum FateReason : int {
    kFateNone = 0, kFateLeftEff1 = 1, kFateLost = 2, kFateEyebox = 3, kFateBeside = 4, kFateOcMiss = 5,
    kFateLeftIc = 6, kFateBounceCap = 7
};
constexpr int kFateEntry = 9;   // the "region" of the in-coupling event
constexpr int kFateCols = 56;   // columns of a census row: 8 per region 0..5, the entry's as region 6; column 0 unused

WGRT_HD uint8_t fate_code(int region, int reason) { return (uint8_t)(10 * region + reason); }

// The codes a trace can end with -- the termination sites of the state machine, nothing else:
//   reason 1, 7  any loop iteration: regions 0-5;          reason 2  any interaction: regions 0-5 and the entry;
//   reason 6     the in-coupler states: the entry, 0, 1;   reasons 3, 4  the three-branch states: regions 4, 5;
//   reason 5     region 5.
WGRT_HD bool fate_valid(int code) {
    if (code <= 0 || code >= 100) return false;
    const int region = code / 10, reason = code % 10;
    if (region == kFateEntry) return reason == kFateLost || reason == kFateLeftIc;
    if (region > 5) return false;
    switch (reason) {
    case kFateLeftEff1:
    case kFateLost:
    case kFateBounceCap: return true;
    case kFateLeftIc: return region <= 1;
    case kFateEyebox:
    case kFateBeside: return region >= 4;
    case kFateOcMiss: return region == 5;
    default: return false;
    }
}

// Column of a code in a census row (include/wgrt.h WGRT_FATE_COLS): 8 * min(region, 6) + reason.  Injective
// on the valid codes (regions 0-5 and the entry's 6 are distinct, reasons are 1-7 < 8), never 0, below kFateCols.
WGRT_HD int fate_col(int code) {
    const int region = code / 10;
    return 8 * (region < 6 ? region : 6) + code % 10;
}

inline const char *fate_reason_name(int reason) {
    switch (reason) {
    case kFateLeftEff1: return "left_plate";
    case kFateLost: return "lost";
    case kFateEyebox: return "eyebox";
    case kFateBeside: return "beside_eyebox";
    case kFateOcMiss: return "oc_miss";
    case kFateLeftIc: return "left_in_coupler";
    case kFateBounceCap: return "bounce_cap";
    default: return nullptr;
    }
}

// Slab of a ray's tile in a census table, matrix_EB's slab order (l * ny + n) * nx + m; -1 for an index outside
// the scene (such a ray is counted nowhere).  The columns hold the indices as floats (wgrt_rays).
WGRT_HD int64_t fate_slab(float fm, float fn, float fl, bool has_l, int nx, int ny, int nl) {
    const int m = (int)fm, n = (int)fn, l = has_l ? (int)fl : 0;
    if (!(m >= 0 && m < nx && n >= 0 && n < ny && l >= 0 && l < nl)) return -1;
    return ((int64_t)l * ny + n) * nx + m;
}

// The argument check wgrt_fate_census and its host twin share: NULL, or why the call is refused.
inline const char *fate_census_args_error(const uint8_t *fate, const float *m, const float *n, int64_t n_rays, int nx,
                                          int ny, int nl, const int64_t *table) {
    if (n_rays < 0) return "negative n_rays";
    if (nx < 1 || ny < 1 || nl < 1) return "need nx, ny, num_lmd >= 1";
    if ((int64_t)nx * ny * nl > 0x7fffffff) return "nx * ny * num_lmd must fit 31 bits";
    if (n_rays > 0 && (!fate || !m || !n || !table)) return "NULL fate / m / n / table";
    return nullptr;
}

}  // namespace wgrt
