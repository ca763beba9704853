// wgrt_visits.h -- branch visit counts: the channel table of a visits launch (wgrt_trace_visits), the end record a
// counted ray leaves when it out-couples, and the rule by which the two reductions (wgrt_visits_sensitivity,
// wgrt_visits_reweight) turn a table of counted rays into window tables -- stated once for both lanes of the state
// machine, the device reductions and their host twins.
//
// A channel is (state, coupler slice, branch): one quadruple of Jones coefficients of one LUT.  With nfc fold-coupler
// and noc out-coupler slices there are C = 6 + 4 nfc + 6 noc of them, B = 6 + 4 nfc:
//     0, 1                  ic.b1, ic.b2           the in-coupling event (GRTF:860-904)
//     2, 3                  r0.b1, r0.b2           R0
//     4, 5                  r1.b1, r1.b2           R1
//     6 + 4 i + {0, 1}      r2[i].b1, .b2          R2 in fold-coupler slice i
//     6 + 4 i + {2, 3}      r3[i].b1, .b2          R3 in fold-coupler slice i
//     B + 6 i + {0, 1, 2}   r4[i].b1, .b2, .b3     R4 in out-coupler slice i (b3: the out-coupling)
//     B + 6 i + {3, 4, 5}   r5[i].b1, .b2, .b3     R5 in out-coupler slice i
// The interaction blocks of a tile are in the same order (wgrt_common.h: 0 the event, 1 R0, 2 R1, 3 + i R2, 3 + nfc + i
// R3, 3 + 2 nfc + i R4, 3 + 2 nfc + noc + i R5), so a channel is a block and a branch.
//
// The rule.  Every Monte-Carlo draw that takes a branch -- the in-coupling event's too -- adds 1 to its channel in the
// ray's row; a draw that loses the ray counts nothing; a draw whose second in-coupler branch carries the ray out of
// the in-coupler (fate reason 6) still counts its b2.  A ray reaches the eyebox with probability prod e_taken, and
// scaling one channel's four coefficients by sqrt(s) multiplies that branch's efficiency by s and nothing else, so
// for a delivered ray d log p / d log s_c = N_c, its count in channel c: summed over the delivered rays the counts are
// the sensitivity of the window table, and re-weighted by prod_c s_c^{N_c} the same rays give the table of the scaled
// design (DESIGN.md §4.10 has the identity's limits).
//
// The end record (wgrt_visit_end, include/wgrt.h) is written when a counted ray's last draw out-couples: the position
// before the move (wgrt_hit's), the global id, the tile index and flags -- bit 1 out-coupled, bit 0 inside the FoV's
// eyebox rectangle.  Two 16-byte halves.  A row is DELIVERED when bit 0 is set; its eyebox bin is eyebox_offset's
// (hits_offset at 80 x 120 over the scene's own range, wgrt_hits.h), and what it is deposited into is the window
// sink's own membership (window_visit, wgrt_window.h: the aliased offset gives the slab, an offset outside the buffer
// is dropped).
#pragma once

#include <cstdint>

#include "../../include/wgrt.h"
#include "wgrt_common.h"
#include "wgrt_expected.h"
#include "wgrt_hits.h"
#include "wgrt_window.h"

namespace wgrt {

static_assert(sizeof(wgrt_visit_end) == 32 && alignof(wgrt_visit_end) == 16, "an end record is two 16-byte halves");

constexpr uint32_t kVisitInside = 1u;   // flags bit 0
constexpr uint32_t kVisitOut = 2u;      // flags bit 1
constexpr int kVisitEntryState = 9;     // the in-coupling event, as the fate code's region

WGRT_HD int visit_channel_count(int nfc, int noc) { return 6 + 4 * nfc + 6 * noc; }

// The channel of branch b (0-based) taken in `state` (9: the in-coupling event; 0..5: R0..R5) in slice `slice` of that
// state's coupler, or -1 for a triple that names none.
WGRT_HD int visit_channel_of(int state, int slice, int b, int nfc, int noc) {
    if (b < 0) return -1;
    if (state == kVisitEntryState) return b < 2 ? b : -1;
    if (state == 0 || state == 1) return b < 2 ? 2 + 2 * state + b : -1;
    if (state == 2 || state == 3) return (b < 2 && slice >= 0 && slice < nfc) ? 6 + 4 * slice + 2 * (state - 2) + b : -1;
    if (state == 4 || state == 5)
        return (b < 3 && slice >= 0 && slice < noc) ? 6 + 4 * nfc + 6 * slice + 3 * (state - 4) + b : -1;
    return -1;
}

// The same from the interaction block both lanes index a tile with (blk in [0, 3 + 2 nfc + 2 noc), b a branch the
// block has).
WGRT_HD int visit_channel(int blk, int b, int nfc, int noc) {
    if (blk < 3) return 2 * blk + b;
    int j = blk - 3;
    if (j < 2 * nfc) {
        const int r3 = j >= nfc ? 1 : 0;
        return 6 + 4 * (j - r3 * nfc) + 2 * r3 + b;
    }
    j -= 2 * nfc;
    const int r5 = j >= noc ? 1 : 0;
    return 6 + 4 * nfc + 6 * (j - r5 * noc) + 3 * r5 + b;
}

// The branch a draw took, from its outcome: kind 0 the in-coupler states (event, R0, R1), 1 R2, 2 R3, 3 R4, 4 R5, as
// both lanes' interact(); next the region the draw led to (< 0: the trace ended there); left_ic: it ended because the
// second in-coupler branch left the in-coupler; out: it ended by out-coupling.  -1: no branch (the ray was lost).
WGRT_HD int visit_branch(int kind, int next, bool left_ic, bool out) {
    if (out) return 2;
    if (left_ic) return 1;
    if (next < 0) return -1;
    return kind == 0 ? (next == 1 ? 1 : 0) : kind <= 2 ? (next == 3 ? 1 : 0) : (next == 5 ? 1 : 0);
}

// The flat eyebox-grid offset of a delivered row, or -1 for a row that deposits nothing (not delivered, a tile index
// outside the scene, a bin outside the buffer).  scene_range(tile, m, n): the FoV's eff_reg_FOV_range.
template <class RangeF>
WGRT_HD int64_t visit_end_offset(const wgrt_visit_end &e, int nl, int nx, int ny, RangeF scene_range) {
    if (!(e.flags & kVisitInside)) return -1;
    const uint32_t g = e.tile;
    if ((uint64_t)g >= (uint64_t)nl * (uint64_t)nx * (uint64_t)ny) return -1;
    const int n = (int)(g % (uint32_t)ny), m = (int)(g / (uint32_t)ny % (uint32_t)nx);
    const int l = (int)(g / ((uint32_t)ny * (uint32_t)nx));
    return hits_offset(scene_range(g, m, n), nl, nx, ny, l, m, n, kEbNy, kEbNx, e.x, e.y);
}

// A row's log-weight under the channel scales: sum_c counts[c] * lnscale[c] in ascending c, one fma each -- the order
// the device thread and the host twin both take.
WGRT_HD double visit_log_weight(const uint32_t *counts, const double *lnscale, int C) {
    double a = 0.0;
    for (int c = 0; c < C; ++c) a = fma((double)counts[c], lnscale[c], a);
    return a;
}

// Design ensembles (wgrt_visits_reweight_many): K designs from one pass over the rows.  Design k has the log-scales
// lnscale[k * C + c]; a row deposits for it exactly what wgrt_visits_reweight deposits with lnscale + k * C,
//     q = expected_quantize(exp(visit_log_weight(counts_row, lnscale + k * C, C))),
// through window_visit at visit_end_offset's offset into out + k * n_slabs * W, and a row whose offset is negative
// deposits nothing for any design.  Table k is therefore the single call's table bit for bit on the same device: the
// same fma chain in ascending c, the same exp, and sums on the 2^-32 grid, which do not depend on their order.
//
// Skipping zero counts.  A kernel may walk only a row's non-zero counts, in ascending c, and get visit_log_weight's
// bits.  A step with a zero count is a = fma(0.0, x, a): for finite x the product is +0 or -0 exactly, and a + (+-0)
// is a for every a but -0.0, which a never is: it starts at +0.0, and a sum that is exactly zero rounds to +0.0 (to
// nearest) unless both terms are -0.0, which would need a to have been -0.0 before.  So the zero steps change nothing,
// and leaving them out leaves the chain of the non-zero steps, each still one fma, in the same order.  (A non-finite
// lnscale breaks the argument -- 0 * inf is NaN -- and is outside the contract; the Python layer refuses it.)
//
// Weight sums.  Every row that deposits also adds, with l = tile / (nx * ny), visit_quanta(q * 2^32) to
// wsums[k][0][l] and visit_quanta(q * q * 2^32) to wsums[k][1][l] (int64 [K, 2, num_lmd], quanta of 2^-32).  Integer
// adds: exact, order-free and additive over shards at any job size, where a float64 sum on the grid stops being exact
// at 2^21.  The effective sample size is s1^2 / s2 of these sums.
constexpr double kVisitQuantaLimit = 0x1p62;

// v as int64 quanta: rint(v), and 2^62 for a v that is not below 2^62 (an overflowed exp, a NaN): such a design has no
// meaningful effective sample size, and the guard keeps the conversion defined.
WGRT_HD int64_t visit_quanta(double v) { return v < kVisitQuantaLimit ? (int64_t)rint(v) : (int64_t)1 << 62; }

// visit_log_weight over the non-zero counts only (the argument above): the host twin's form of what the kernel does
// with a ballot.
WGRT_HD double visit_log_weight_sparse(const uint32_t *counts, const double *lnscale, int C) {
    double a = 0.0;
    for (int c = 0; c < C; ++c)
        if (counts[c]) a = fma((double)counts[c], lnscale[c], a);
    return a;
}

// NULL, or why the ensemble's own arguments are refused (after visits_reduce_error).
inline const char *visits_many_error(const void *lnscale, int64_t K, const void *wsums) {
    if (K < 1) return "need K >= 1 designs";
    if (!lnscale || ((uintptr_t)lnscale & 7)) return "NULL or misaligned lnscale";
    if ((uintptr_t)wsums & 7) return "wsums must be 8-B aligned";
    return nullptr;
}

// NULL, or why the arguments of a reduction are refused.
inline const char *visits_reduce_error(const void *plan, const void *counts, const void *ends, int64_t n_rows,
                                       const void *out) {
    if (!plan) return "NULL plan";
    if (n_rows < 0) return "need n_rows >= 0";
    if (n_rows > 0 && (!counts || !ends || !out)) return "NULL counts / ends / table";
    if (((uintptr_t)ends & 15) || ((uintptr_t)counts & 3) || ((uintptr_t)out & 7))
        return "ends must be 16-B aligned (counts 4-B, the table 8-B)";
    return nullptr;
}

}  // namespace wgrt
