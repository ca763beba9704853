// wgrt_expected.h -- the expected-value (collision) estimator's weight, stated once for both lanes of the state
// machine, the host twin wgrt_expected_weight_host and (through it) the Python layer (wgrt_trace_expected).
//
// An out-coupler interaction (R4 / R5, GRTF:1110-1246) draws u in [0, 1] and takes, in this order,
//     branch 1 if u <= e1           and en1 > t,
//     branch 2 if u <= e1 + e2      and en2 > t,
//     out      if u <= e1 + e2 + e3 and en3 > t          (en_k = ener * e_k; t = 0 full colour, 1e-15 one wavelength)
// and loses the ray otherwise.  The analog estimator adds 1 to the bin under the ray when the draw out-couples it;
// the expected-value estimator adds, at EVERY such interaction inside the FoV's eyebox rectangle, the probability
// that the draw does: the length of the set of u in [0, 1] that reaches the third line,
//     w  = 0                                        if !(en3 > t)
//     lo = (en2 > t) ? e1 + e2 : (en1 > t) ? e1 : 0       (a branch whose guard is off passes its draws on)
//     w  = max(0, min(e1 + e2 + e3, 1) - min(lo, 1)),
// e3 in the ordinary regime.  The walk is untouched -- the same draws, branches, RNG states, counters -- and
// the expectation of every table entry is the analog estimator's.
//
// The deposit is fixed point: q = rint(w * 2^32) * 2^-32 (ties to even; w == 1 gives exactly 1.0, q == 0 deposits
// nothing).  The draw itself is one of 2^32 values, so treating it as continuous is the rounding q already makes.
// Sums of multiples of 2^-32 are exact in float64 while an entry stays below 2^21 (53 - 32 bits of integer part):
// below that limit the table does not depend on the order of the atomic adds, is the same bits on every run, and
// the tables of shards and replicas add up exactly, as the count table's do.  2^21 expected out-couplings in one
// table entry is what a caller must stay below between two reads of the table.
#pragma once

#include <cmath>

#include "wgrt_common.h"

namespace wgrt {

constexpr double kExpectedQuantum = 0x1p-32;
constexpr double kExpectedEntryLimit = 0x1p21;   // exact sums below this

// w of the rule above (a NaN e3 fails the guard: nothing is deposited).
WGRT_HD double expected_weight(double e1, double e2, double e3, double en1, double en2, double en3, double t) {
    if (!(en3 > t)) return 0.0;
    const double lo = (en2 > t) ? e1 + e2 : (en1 > t) ? e1 : 0.0;
    const double hi = e1 + e2 + e3;
    const double w = (hi < 1.0 ? hi : 1.0) - (lo < 1.0 ? lo : 1.0);
    return w > 0.0 ? w : 0.0;
}

// q: the weight on the 2^-32 grid (rint: round to nearest, ties to even, the default rounding mode).
WGRT_HD double expected_quantize(double w) { return rint(w * 0x1p32) * kExpectedQuantum; }

WGRT_HD double expected_deposit(double e1, double e2, double e3, double en1, double en2, double en3, double t) {
    return expected_quantize(expected_weight(e1, e2, e3, en1, en2, en3, t));
}

}  // namespace wgrt
