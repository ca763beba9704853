// wgrt_sources.h -- source what-ifs: the rule by which a hit list (wgrt_hit records, wgrt_hits.h) is re-weighted for K
// projector pupils (wgrt_hits_reweight_sources) and counted per entry class (wgrt_hits_source_counts), stated once for
// the device kernels and their host twins.
//
// A ray's entry point and input polarisation are a pure function of its global id.  With R rays per FoV x wavelength
// block, ray gid has the block index r = gid mod R; it starts at points[r mod (R / 2)] and is TE for r < R / 2, TM
// otherwise (rays_init_kernel, wgrt_rays.hip).  Rays are independent, so a source that emits class r with relative
// radiance w[r] delivers exactly the table in which every out-coupling deposits w[gid mod R] instead of 1.
//
//   block index   source_index(gid, R) = gid mod R for gid >= 0; a record with gid < 0 is dropped.
//   what counts   a record whose flag bit 0 (kHitInside) is set and whose tile is below num_lmd * nx * ny.
//   binning       hits_record_offset(..., caller_r = NULL, 80, 120): the trace's own eyebox_offset, aliasing and the
//                 [0, total) guard included; the deposits go through window_visit, so the slab comes from the offset.
//   the deposit   q = expected_quantize(w) = rint(w * 2^32) * 2^-32 (wgrt_expected.h): sums are exact and order-free
//                 while an entry stays below 2^21; a weight of 1 deposits exactly 1.0, so a row of ones gives the
//                 launches' window table bit for bit.  q == 0 deposits nothing and adds nothing to the sums.
//   weights       finite, 0 <= w <= kSourceMaxWeight; the device entry points validate nothing (the host wrapper and
//                 the Python layer do): a weight outside gives a table that means nothing, never a write out of bounds.
//   weight sums   as wgrt_visits_reweight_many keeps them (wgrt_visits.h): int64 [K, 2, num_lmd] in quanta of 2^-32, a
//                 depositing record adds visit_quanta(q * 2^32) and visit_quanta(q * q * 2^32) at l = tile / (nx * ny).
//                 With w <= 1024 the first is below 2^43 and the second below 2^53: both exact.
//   class counts  counts[l][0][r] += 1 for a record inside its FoV's eyebox rectangle (flag bit 0 set), counts[l][1][r]
//                 for one beside it: the flag decides, not whether the aliased offset was stored.  A record with
//                 gid < 0 or a tile beyond the scene is dropped.
#pragma once

#include <cstdint>

#include "../../include/wgrt.h"
#include "wgrt_common.h"
#include "wgrt_expected.h"
#include "wgrt_hits.h"
#include "wgrt_visits.h"
#include "wgrt_window.h"

namespace wgrt {

constexpr double kSourceMaxWeight = 1024.0;

// gid >= 0, R >= 1
WGRT_HD int64_t source_index(int64_t gid, int64_t R) { return gid % R; }

// The flat eyebox-grid offset of a record that deposits, or -1 (gid < 0, not flagged inside, a tile index outside the
// scene, a bin outside the buffer).  scene_range(tile, m, n): the FoV's eff_reg_FOV_range.
template <class RangeF>
WGRT_HD int64_t source_record_offset(const wgrt_hit &h, int nl, int nx, int ny, RangeF scene_range) {
    if (h.gid < 0) return -1;
    return hits_record_offset(h, nl, nx, ny, scene_range, (const double *)nullptr, kEbNy, kEbNx);
}

// The entry of counts [nl, 2, R] a record adds 1 to, or -1 for a record that is dropped.
WGRT_HD int64_t source_count_entry(const wgrt_hit &h, int nl, int nx, int ny, int64_t R) {
    if (h.gid < 0) return -1;
    if ((uint64_t)h.tile >= (uint64_t)nl * (uint64_t)nx * (uint64_t)ny) return -1;
    const int64_t l = h.tile / ((uint32_t)nx * (uint32_t)ny);
    return (l * 2 + ((h.flags & kHitInside) ? 0 : 1)) * R + source_index(h.gid, R);
}

// NULL, or why the arguments of wgrt_hits_source_counts are refused.
inline const char *source_counts_error(const void *hits, int64_t n, int64_t R, const void *counts) {
    if (n < 0) return "need n >= 0";
    if (R < 1) return "need R >= 1 rays per block";
    if (n > 0 && (!hits || !counts)) return "NULL hits / counts";
    if (((uintptr_t)hits & 15) || ((uintptr_t)counts & 7)) return "the hit list must be 16-B aligned (counts 8-B)";
    return nullptr;
}

// NULL, or why the arguments of wgrt_hits_reweight_sources are refused.
inline const char *source_reweight_error(const void *plan, const void *hits, int64_t n, const void *weights, int64_t R,
                                         int64_t K, const void *out, const void *wsums) {
    if (!plan) return "NULL plan";
    if (n < 0) return "need n >= 0";
    if (R < 1) return "need R >= 1 rays per block";
    if (K < 1) return "need K >= 1 sources";
    if (!weights || ((uintptr_t)weights & 7)) return "NULL or misaligned weights";
    if (n > 0 && (!hits || !out)) return "NULL hits / table";
    if (((uintptr_t)hits & 15) || ((uintptr_t)out & 7)) return "the hit list must be 16-B aligned (the table 8-B)";
    if ((uintptr_t)wsums & 7) return "wsums must be 8-B aligned";
    return nullptr;
}

}  // namespace wgrt
