// wgrt_stokes.h -- the polarisation of an out-coupled ray as fixed-point normalised Stokes parameters, stated once for
// both lanes of the state machine and the host twin wgrt_stokes_quanta_host (wgrt_trace_stokes).
//
// The draw that out-couples a ray towards the eye (the third branch of an R4 / R5 interaction, GRTF:1162-1171,
// 1231-1240) has computed the out-coupled order's field E3 = M3 E (E_field_cal, GRTF:132-152) to get its
// efficiency.  With a = E3's complex TE amplitude and b = its complex TM amplitude,
//     S0 = |a|^2 + |b|^2
//     s1 = (|a|^2 - |b|^2) / S0          +1: all TE, -1: all TM
//     s2 = 2 Re(a conj b) / S0           +1: linear at +45 degrees from the TE axis
//     s3 = 2 Im(conj a b) / S0           for a = Ete, b = Etm e^{i delta}: 2 Ete Etm sin(delta) / S0
// Every one is invariant under a global phase of (a, b): the exact lane's (|Ete|, |Etm|, delta) and the Jones-vector
// lane's complex pair describe the same state and give the same parameters.
//
// Basis.  (a, b) are the TE / TM components of THAT FoV's out-coupled order, exactly as the reference's LUTs define
// them (the rows of the out-coupling matrix: channels 13 / 18 / 33 / 38 of lut_oc1 in R4, 15 / 20 / 35 / 40 of lut_oc2
// in R5).  The basis turns with the order's azimuth from FoV to FoV; nothing here rotates it into a common frame.
//
// A deposit is three int32 quanta q_k = rint(s_k * 2^30) (ties to even), |q_k| <= 2^30; (0, 0, 0) when S0 is not a
// positive finite number.  They are summed into int64 tables beside the window table (wgrt_window.h's membership), so
// the sums are order-independent and exact while an entry has fewer than 2^33 deposits.
//
// Every product that feeds a sum is an explicit fma, the rest are single IEEE operations (+ - / rint): no compiler
// can contract the device code, the host twin or a C restatement differently, whatever its -ffp-contract.
#pragma once

#include <cmath>

#include "wgrt_common.h"

namespace wgrt {

constexpr double kStokesScale = 0x1p30;   // quanta per unit of a normalised Stokes parameter

// q[0..2] of the field a = (ar, ai), b = (br, bi).
WGRT_HD void stokes_quanta(double ar, double ai, double br, double bi, int32_t q[3]) {
    const double aa = fma(ar, ar, ai * ai), bb = fma(br, br, bi * bi);
    const double s0 = aa + bb;
    q[0] = q[1] = q[2] = 0;
    if (!(s0 > 0.0 && s0 < INFINITY)) return;
    const double re = fma(ar, br, ai * bi);      // Re(a conj b)
    const double im = fma(ar, bi, -(ai * br));   // Im(conj a b)
    q[0] = (int32_t)rint((aa - bb) / s0 * kStokesScale);
    q[1] = (int32_t)rint((re + re) / s0 * kStokesScale);
    q[2] = (int32_t)rint((im + im) / s0 * kStokesScale);
}

}  // namespace wgrt
