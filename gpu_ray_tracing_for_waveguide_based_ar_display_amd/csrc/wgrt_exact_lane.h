// wgrt_exact_lane.h -- the exact lane of the reference's per-ray state machine
// (GPU_ray_tracing_functions.py = GRTF:833-1246): the reference's float64
// arithmetic in its expression order, stated once.  Who runs what:
//   trace_one     variant 1 (trace_grid_kernel) and every replay (replay_tail, epilogue_kernel; wgrt_trace.hip):
//                 lane_load, then interact / advance in turn, lane_retire;
//   lane_load, take_branch, advance, lane_retire
//                 the certification shadow too (wgrt_shadow.hip), around its own literal all-branches decision:
//                 what it certifies the product lane against is this file's arithmetic, not a copy of it;
//   eyebox_add    the Jones kernels' out-coupling queue (bin_entry, wgrt_trace.hip); interact's out-coupling runs
//                 its two halves, eyebox_inside (the rectangle test: also the fate's reason 3 / 4, and what the
//                 Jones lane's FATE instantiations call) and eyebox_bin.
// FATE (a template parameter of interact, advance, lane_retire and trace_one; off by default): every place a trace
// ends sets the lane's fate code (wgrt_fate.h) and lane_retire stores it beside per_ray.  Without it the lane is
// the code it was before fates existed -- the replays inlined into the Jones kernels keep their registers.
// EV (a template parameter of interact and trace_one; off by default): the expected-value estimator of
// wgrt_trace_expected (wgrt_expected.h).  Every R4 / R5 interaction inside the FoV's eyebox rectangle evaluates
// the reference's exact efficiencies and deposits the fixed-point weight q through eyebox_deposit; the analog +1 of
// the out-coupling itself is not added (Lane::hit still says whether it would have been).  *ev_skip, when not
// zero, is the number of such visits whose deposit has already been made (a replay of a ray the Jones lane
// abandoned after scoring them): they are passed over.  The walk -- draws, branches, counters -- is EV = false's.
// FP (a template parameter of trace_one; off by default): the footprint maps of wgrt_trace_footprint
// (wgrt_footprint.h).  trace_one counts every draw of the bounce loop where the ray stood before interact() moved
// it, and reads the draw's second channel (lost / out-coupled inside / beside the eyebox) from the fate code that
// interact<FATE> leaves in the lane -- so interact itself has no FP of its own.  Its `skip` draws are passed over
// (counted by the Jones lane before it abandoned the ray).  The walk is FP = false's.
// HITS (a template parameter of interact and trace_one; off by default): the hit list of wgrt_trace_hits
// (wgrt_hits.h).  interact's out-coupling appends one record for both outcomes of the rectangle test (hit_store).  A
// template parameter and not a test of TraceArgs::hits, so that every other kernel is the code it was.
// STOKES (a template parameter of interact and trace_one; off by default): the Stokes window tables of
// wgrt_trace_stokes (wgrt_stokes.h).  interact's out-coupling, inside the FoV's eyebox rectangle, evaluates the
// out-coupled order's field E3 (the third E_field_cal of the interaction, as the reference computes it) and adds its
// three quanta to the entries the window table counts the out-coupling into (eyebox_bin_stokes).  A template parameter
// for the same reason.
#pragma once

#include "wgrt_args.h"
#include "wgrt_expected.h"
#include "wgrt_fate.h"
#include "wgrt_footprint.h"
#include "wgrt_hits.h"
#include "wgrt_locator.h"
#include "wgrt_paths.h"
#include "wgrt_stokes.h"
#include "wgrt_visits.h"
#include "wgrt_window.h"

namespace wgrt {

// E_field_cal (GRTF:132-152).  rec = (p, q, r, s) complex in the reference call's argument
// order: Ete' = p*te_in + r*tm_in, Etm' = q*te_in + s*tm_in.  The multiplications by 0.0 are
// Python's real->complex promotions; they are kept so signed zeros propagate exactly.
struct Field {
    double te_re, te_im, tm_re, tm_im;
};

__device__ __forceinline__ Field efield(double Ete, double Etm, double cd, double sd, const double *rec) {
    const double pr = rec[0], pi = rec[1], qr = rec[2], qi = rec[3];
    const double rr = rec[4], ri = rec[5], sr = rec[6], si = rec[7];
    const double ti_re = cd * Etm - sd * 0.0, ti_im = cd * 0.0 + sd * Etm;
    const double a_re = pr * Ete - pi * 0.0, a_im = pr * 0.0 + pi * Ete;
    const double b_re = rr * ti_re - ri * ti_im, b_im = rr * ti_im + ri * ti_re;
    const double c_re = qr * Ete - qi * 0.0, c_im = qr * 0.0 + qi * Ete;
    const double d_re = sr * ti_re - si * ti_im, d_im = sr * ti_im + si * ti_re;
    return Field{a_re + b_re, a_im + b_im, c_re + d_re, c_im + d_im};
}

// |Ete'|^2 + |Etm'|^2 of efield() without the "* 0.0" promotion terms: for finite inputs
// (LUTs are checked at scene creation, ray state stays finite) those terms only change the
// sign of zero components, so every component has the same magnitude as efield()'s and the
// sum of squares is identical.  Used for the branch estimates only.
__device__ __forceinline__ double efield_sq(double Ete, double Etm, double cd, double sd, const double *rec) {
    const double pr = rec[0], pi = rec[1], qr = rec[2], qi = rec[3];
    const double rr = rec[4], ri = rec[5], sr = rec[6], si = rec[7];
    const double ti_re = cd * Etm, ti_im = sd * Etm;
    const double a_re = pr * Ete + (rr * ti_re - ri * ti_im), a_im = pi * Ete + (rr * ti_im + ri * ti_re);
    const double c_re = qr * Ete + (sr * ti_re - si * ti_im), c_im = qi * Ete + (sr * ti_im + si * ti_re);
    return (a_re * a_re + a_im * a_im) + (c_re * c_re + c_im * c_im);
}

// The exact lane carries the ray's delta_phase as the reference does (GRTF:857): a taken branch
// sets it to E_field_cal's wrapped phase difference plus lut_TIR (GRTF:145-150, 877, 926, ...), a
// miss hop adds 2 lut_TIR without a wrap (GRTF:1052, 1108, 1178), and every E_field_cal takes
// cos / sin of the accumulated, unwrapped value (GRTF:135).  The rounding of that accumulation is
// part of the reference's result: with lut_TIR near +-pi and runs of hundreds of hops the phase
// reaches thousands of radians, and a rotation carried as a product of hop phasors instead (round
// 4's lane) drifted from it far enough to change decisions (the adversarial_lossless LUTs of
// tests/test_gpu_certification.py: 33 of 96,768 rays).  This lane differs from the reference only by
// the device's cos / sin / atan2 against glibc's (ulps of the result).
struct Ray {
    double x, y, te, tm, cos_t, ener;
    double dph;   // delta_phase (GRTF:857), unwrapped as the reference carries it
    uint32_t s;
    int region;
};

// One ray in flight on a lane.
struct Lane {
    Ray r;
    const double *T;   // this ray's (lambda, m, n) tile
    int64_t i;         // local ray index
    int l, m, n;
    uint32_t bounces;  // 1 in-coupling event + loop iterations (GRTF:905)
    bool hit;          // accumulated into matrix_EB
    bool libm;         // a guard product ener * e_k fell below 2^-1000 (wgrt_trace_stats.libm_rays)
    uint8_t why;       // fate code (wgrt_fate.h), set where the trace ends
};

// Load ray i (GRTF:846-859).  Returns false (and leaves the lane empty) for a ray whose
// FoV / wavelength indices fall outside the scene.
__device__ __forceinline__ bool lane_load(const TraceArgs &A, int64_t i, Lane &L) {
    const int m = (int)A.m[i], n = (int)A.n[i], l = A.l ? (int)A.l[i] : 0;
    if (!(m >= 0 && m < A.nx && n >= 0 && n < A.ny && l >= 0 && l < A.nl)) return false;
    L.i = i;
    L.l = l;
    L.m = m;
    L.n = n;
    L.T = A.tiles + (int64_t)((l * A.nx + m) * A.ny + n) * A.tile_d;
    L.r.x = (double)A.x[i];
    L.r.y = (double)A.y[i];
    L.r.te = (double)A.te[i];
    L.r.tm = (double)A.tm[i];
    L.r.dph = (double)A.dph[i];
    L.r.cos_t = 1.0;
    L.r.ener = 1.0;
    L.r.s = A.rng[i];
    L.r.region = 0;
    L.bounces = 1;
    L.hit = false;
    L.libm = false;
    L.why = 0;
    return true;
}

// Eyebox accumulation of an out-coupling (GRTF:1162-1171, 1231-1240) of a ray of tile T = (l, m, n) at (x, y):
// the per-FoV eyebox rectangle test (eyebox_inside: the one statement of it), then the bin and the atomic
// (eyebox_bin) -- into the grid, into the pupil-window table of wgrt_trace_windows, or both (wave-uniform: they
// are launch arguments).  eyebox_bin / eyebox_add return whether the bin was added to.
__device__ __forceinline__ bool eyebox_inside(const double *T, double x, double y) {
    return inside_or_on_edge(x, y, T + kTileEbRect, 4);
}

// rep() gives the ray's replica (wgrt_trace_replicas): called only where a launch with replica tables bins into
// them, so a launch without pays one wave-uniform test inside the table branch.
// The flat grid offset of the bin under (x, y), or -1 for one outside the buffer.
__device__ __forceinline__ int64_t eyebox_offset(const TraceArgs &A, const double *T, int l, int m, int n, double x,
                                                 double y) {
    const double xmin = T[kTileEbRange], xmax = T[kTileEbRange + 1];
    const double ymin = T[kTileEbRange + 2], ymax = T[kTileEbRange + 3];
    const double dx = (xmax - xmin) / kEbNx, dy = (ymax - ymin) / kEbNy;
    int64_t ix = (int64_t)floor((x - xmin) / dx);
    int64_t iy = (int64_t)floor((y - ymin) / dy);
    // compiled-numba addressing (GRTF:164): a negative index wraps once, an index
    // equal to the axis length aliases into the next row; guarded to the buffer
    if (ix < 0) ix += kEbNx;
    if (iy < 0) iy += kEbNy;
    const int64_t off = ((((int64_t)l * A.ny + n) * A.nx + m) * kEbNy + iy) * kEbNx + ix;
    const int64_t total = (int64_t)A.nl * A.ny * A.nx * kEbNy * kEbNx;
    return (off >= 0 && off < total) ? off : -1;
}

template <class RepF>
__device__ __forceinline__ bool eyebox_bin(const TraceArgs &A, const double *T, int l, int m, int n, double x,
                                           double y, RepF rep) {
    const int64_t off = eyebox_offset(A, T, l, m, n, x, y);
    if (off >= 0) {
        if (A.eb) unsafeAtomicAdd(A.eb + off, 1.0f);
        if (A.win_table) {
            double *table = A.win_table;
            if (A.win_reps) table += (int64_t)rep() * A.win_rep_stride;
            window_visit(*A.win, off, [table](int64_t k) { unsafeAtomicAdd(table + k, 1.0); });
        }
        return true;
    }
    return false;
}

// An out-coupling of a Stokes launch (wgrt_trace_stokes; wgrt_stokes.h) that has passed eyebox_inside: eyebox_bin's
// adds (no replicas: such a launch has none), and the quanta q[k] added to table k of A.stokes at every entry the
// window table counts it into -- unsigned 64-bit adds of the sign-extended quanta whose result is not used, so the
// tables do not depend on the order.  Both lanes deposit through it.
__device__ __forceinline__ bool eyebox_bin_stokes(const TraceArgs &A, const double *T, int l, int m, int n, double x,
                                                  double y, int32_t q0, int32_t q1, int32_t q2) {
    const int64_t off = eyebox_offset(A, T, l, m, n, x, y);
    if (off < 0) return false;
    if (A.eb) unsafeAtomicAdd(A.eb + off, 1.0f);
    double *const table = A.win_table;
    unsigned long long *const st = (unsigned long long *)A.stokes;
    const int64_t stride = A.stokes_stride;
    window_visit(*A.win, off, [=](int64_t k) {
        unsafeAtomicAdd(table + k, 1.0);
        if (q0) atomicAdd(st + k, (unsigned long long)(int64_t)q0);
        if (q1) atomicAdd(st + stride + k, (unsigned long long)(int64_t)q1);
        if (q2) atomicAdd(st + 2 * stride + k, (unsigned long long)(int64_t)q2);
    });
    return true;
}

// The expected-value estimator's deposit (wgrt_expected.h) of a visit at (x, y) that has passed eyebox_inside: q
// (a multiple of 2^-32; 0: nothing) added to the window table's entries under the bin, by the same membership
// rule.  Returns whether the bin lies in the buffer -- whether an out-coupling here is an analog hit.
template <class RepF>
__device__ __forceinline__ bool eyebox_deposit(const TraceArgs &A, const double *T, int l, int m, int n, double x,
                                               double y, double q, RepF rep) {
    const int64_t off = eyebox_offset(A, T, l, m, n, x, y);
    if (off < 0) return false;
    if (q > 0.0) {
        double *table = A.win_table;
        if (A.win_reps) table += (int64_t)rep() * A.win_rep_stride;
        window_visit(*A.win, off, [table, q](int64_t k) { unsafeAtomicAdd(table + k, q); });
    }
    return true;
}

template <class RepF>
__device__ __forceinline__ bool eyebox_add(const TraceArgs &A, const double *T, int l, int m, int n, double x,
                                           double y, RepF rep) {
    return eyebox_inside(T, x, y) && eyebox_bin(A, T, l, m, n, x, y, rep);
}

// One record of the hit list (wgrt_trace_hits; wgrt_hits.h) at its reserved index: stored iff the index is below
// the capacity, as two 16-byte stores (position; global id, tile index, flags), so nothing at or beyond hits + cap is
// written.  Both lanes append through it.
__device__ __forceinline__ void hit_store(wgrt_hit *hits, int64_t cap, unsigned long long idx, double x, double y,
                                          int64_t gid, uint32_t tile, uint32_t flags) {
    static_assert(offsetof(wgrt_hit, gid) == 16 && offsetof(wgrt_hit, tile) == 24 && offsetof(wgrt_hit, flags) == 28,
                  "the second half: gid, then tile below flags in one 64-bit word");
    if (idx < (unsigned long long)cap) {
        double2 *const p = (double2 *)(hits + idx);
        p[0] = double2{x, y};
        ((ulonglong2 *)p)[1] = ulonglong2{(unsigned long long)gid, (unsigned long long)tile | (unsigned long long)flags << 32};
    }
}

// One record of the path list (wgrt_trace_paths; wgrt_paths.h) at its reserved index, by hit_store's pattern: stored
// iff the index is below the capacity, as two 16-byte stores (position; global id, step below flags).
__device__ __forceinline__ void path_store(wgrt_path_vertex *paths, int64_t cap, unsigned long long idx, double x,
                                           double y, int64_t gid, uint32_t step, uint32_t flags) {
    static_assert(offsetof(wgrt_path_vertex, gid) == 16 && offsetof(wgrt_path_vertex, step) == 24 &&
                      offsetof(wgrt_path_vertex, flags) == 28,
                  "the second half: gid, then step below flags in one 64-bit word");
    if (idx < (unsigned long long)cap) {
        double2 *const p = (double2 *)(paths + idx);
        p[0] = double2{x, y};
        ((ulonglong2 *)p)[1] = ulonglong2{(unsigned long long)gid, (unsigned long long)step | (unsigned long long)flags << 32};
    }
}

// One certified draw of a counted ray (wgrt_trace_visits; wgrt_visits.h), by both lanes: the taken branch's channel c
// (< 0: the draw took none) adds 1 to the ray's row -- an unsigned add whose result is not used -- and a draw that
// out-couples writes the row's end record as two 16-byte stores (position; global id, tile index below flags).  gid():
// the ray's global id, looked up only there.
template <class GidFn>
__device__ __forceinline__ void visit_count(uint32_t *counts, wgrt_visit_end *ends, int C, int64_t row, int c, bool out,
                                            bool inside, double x, double y, uint32_t tile, GidFn gid) {
    static_assert(offsetof(wgrt_visit_end, gid) == 16 && offsetof(wgrt_visit_end, tile) == 24 &&
                      offsetof(wgrt_visit_end, flags) == 28,
                  "the second half: gid, then tile below flags in one 64-bit word");
    if (c >= 0) atomicAdd(counts + row * C + c, 1u);
    if (out) {
        const uint32_t flags = kVisitOut | (inside ? kVisitInside : 0u);
        double2 *const p = (double2 *)(ends + row);
        p[0] = double2{x, y};
        ((ulonglong2 *)p)[1] = ulonglong2{(unsigned long long)gid(), (unsigned long long)tile | (unsigned long long)flags << 32};
    }
}

// Take branch b (0 or 1) of block B in state `kind` (GRTF:872-882 and every branch body after it): cte / ctm are
// the branch's exact magnitudes (correctly rounded hypot of E_field_cal's components), dphi its wrapped phase
// difference (GRTF:145-150) and e its exact efficiency.  Returns the next region, or kDie for a ray that the
// in-coupler's second branch carries out of the in-coupler.
template <class Loc>
__device__ __forceinline__ int take_branch(const Loc &loc, Lane &L, const double *B, int b, int kind, double cte,
                                           double ctm, double dphi, double e) {
    Ray &r = L.r;
    const double *T = L.T;
    const double norm = sqrt(cte * cte + ctm * ctm);
    int tir, gap;
    if (kind == 0) { tir = b == 0 ? 0 : 2; gap = b == 0 ? 0 : 4; }
    else if (kind <= 2) { tir = b == 0 ? 0 : 1; gap = b == 0 ? 0 : 2; }
    else { tir = b == 0 ? 1 : 3; gap = b == 0 ? 2 : 6; }
    r.cos_t = B[b];
    r.te = cte / norm;
    r.tm = ctm / norm;
    r.dph = dphi + T[kTileTir + tir];   // delta_phase = delta_phase_b + lut_TIR[...] (GRTF:877, ...)
    r.x += T[kTileGap + gap];
    r.y += T[kTileGap + gap + 1];
    r.ener = r.ener * e;
    if (kind == 0) {
        const bool in_ic = in_poly(loc, locate(loc, r.x, r.y), kPolyIC, r.x, r.y);
        if (b == 0) return in_ic ? 0 : 2;
        return in_ic ? 1 : kDie;   // (interact sets the fate: reason 6)
    }
    if (kind <= 2) return b == 0 ? 2 : 3;
    return b == 0 ? 4 : 5;
}

// A coupler interaction: `blk` of the lane's tile, `kind` 0 in-coupler states (entry event,
// R0, R1), 1 R2, 2 R3, 3 R4, 4 R5.  Evaluates every branch's efficiency (GRTF:860-869,
// 909-918, ..., 1186-1200), draws, and applies the chosen branch.  Returns the next region
// or kDie (FATE: with the lane's fate set; its region is the state the ray is in, 9 at the entry).
// Only the chosen branch's phase (two atan2) is evaluated; its field is recomputed
// by the same operations rather than kept in registers for every branch.
template <bool FATE = false, bool EV = false, bool HITS = false, bool STOKES = false, class Loc>
__device__ __forceinline__ int interact(const TraceArgs &A, const Loc &loc, Lane &L, int blk, int kind,
                                        bool entry, uint32_t *ev_skip = nullptr) {
    Ray &r = L.r;
    const double *T = L.T;
    const double *B = T + kTileHeader + kBlock * blk;
    // phase = complex(math.cos(delta), math.sin(delta)) (GRTF:135), once for every E_field_cal call of
    // this interaction (they all take the same delta)
    const double cd = cos(r.dph), sd = sin(r.dph);
    const bool three = kind >= 3;
    const bool thr = kind >= 1;  // the ener > threshold guard exists only in R2..R5
    const double denom = entry ? T[kTileCosIc1] : r.cos_t;
    const double u = rng_draw_lazy(r.s, [&]() { return ray_gid(A, L.i); });
    const int freg = entry ? kFateEntry : r.region;   // (FATE only)
    // EV: a scored visit.  Its weight is made of the reference's own e_k, so the decision is taken on the exact
    // path below too (either path gives the reference's decision)
    const bool ev_here = EV && three && eyebox_inside(T, r.x, r.y);

    // Decide the branch.  The reference compares u with cumulative branch efficiencies
    // e_k = (hypot(Ete')^2 + hypot(Etm')^2) * cosA_k / cos(theta) [* or / n_g].  Here the
    // comparisons are first made with cheap estimates (squared moduli instead of the
    // correctly rounded hypot, one reciprocal instead of three divisions), whose relative
    // error is below 1e-14; a decision is accepted only when every threshold it depends on
    // is farther than 1e-12 (relative) from u and no product can underflow, which makes it
    // provably the reference's decision.  Otherwise -- about once in 1e12 draws -- the lane
    // recomputes every e_k exactly as the reference does.  The chosen branch's magnitudes
    // and efficiency are always computed exactly.
    // one branch at a time (a rolled loop keeps the register peak down)
    double q[3] = {0.0, 0.0, 0.0};
    const int nbr = three ? 3 : 2;
#pragma unroll 1
    for (int k = 0; k < nbr; ++k) {
        const double v = efield_sq(r.te, r.tm, cd, sd, B + kBlockRec + 8 * k);
        q[0] = k == 0 ? v : q[0];
        q[1] = k == 1 ? v : q[1];
        q[2] = k == 2 ? v : q[2];
    }
    // 1 / denom to ~1e-16 relative (estimates only): hardware reciprocal + two Newton steps
    double inv = __builtin_amdgcn_rcp(denom);
    inv = fma(inv, fma(-denom, inv, 1.0), inv);
    inv = fma(inv, fma(-denom, inv, 1.0), inv);
    double a0 = q[0] * B[0] * inv, a1 = q[1] * B[1] * inv;
    if (entry) {
        a0 *= A.n_g;
        a1 *= A.n_g;
    }
    const double a2 = three ? q[2] * B[2] * inv * A.inv_n_g : 0.0;
    const double c0 = a0, c1 = a0 + a1, c2 = c1 + a2;
    const double scale = fabs(a0) + fabs(a1) + fabs(a2);   // bounds every partial sum
    const double tol = 1e-12 * scale;
    const bool tiny = thr && !(r.ener > 1e-200 && (a0 == 0.0 || a0 > 1e-100) && (a1 == 0.0 || a1 > 1e-100) &&
                               (!three || a2 == 0.0 || a2 > 1e-100));
    // ener * e_k > threshold (GRTF:606 single-lambda: 1e-15; GRTF:1020 full colour: 0).  With
    // threshold 0 and no underflow it is e_k > 0, i.e. a_k > 0; otherwise the estimate
    // ener * a_k must clear the threshold by a relative margin far above its error.
    const double t = A.threshold;
    const double p0 = r.ener * a0, p1 = r.ener * a1, p2 = r.ener * a2;
    const double tmar = 1e-12 * t;
    const bool tsure = !thr || t == 0.0 ||
                       (fabs(p0 - t) > tmar && fabs(p1 - t) > tmar && (!three || fabs(p2 - t) > tmar));
    const bool pass0 = !thr || (t == 0.0 ? a0 > 0.0 : p0 > t);
    const bool pass1 = !thr || (t == 0.0 ? a1 > 0.0 : p1 > t);
    const bool pass2 = t == 0.0 ? a2 > 0.0 : p2 > t;
    const bool sure = scale > 1e-290 && !tiny && tsure && fabs(u - c0) > tol && fabs(u - c1) > tol &&
                      (!three || fabs(u - c2) > tol);
    int b;
    if (sure && !ev_here) {
        if (u <= c0 && pass0) b = 0;
        else if (u <= c1 && pass1) b = 1;
        else if (three && u <= c2 && pass2) b = 2;
        else {
            if (FATE) L.why = fate_code(freg, kFateLost);
            return kDie;
        }
    } else {
        double te[3], tm[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            te[k] = tm[k] = 0.0;
            if (k < 2 || three) {
                const Field f = efield(r.te, r.tm, cd, sd, B + kBlockRec + 8 * k);
                te[k] = hypot_cr(f.te_re, f.te_im);
                tm[k] = hypot_cr(f.tm_re, f.tm_im);
            }
        }
        double e0 = (te[0] * te[0] + tm[0] * tm[0]) * B[0] / denom;
        double e1 = (te[1] * te[1] + tm[1] * tm[1]) * B[1] / denom;
        if (entry) {
            e0 = e0 * A.n_g;
            e1 = e1 * A.n_g;
        }
        double e2 = 0.0;
        if (three) e2 = (te[2] * te[2] + tm[2] * tm[2]) * B[2] / denom / A.n_g;
        // the ener-underflow regime: a guard product ener * e_k (GRTF:1020, 1073, 1136,
        // ...) of a nonzero efficiency below 2^-1000, next to the subnormal range, where whether it rounds
        // to zero -- and so the decision -- hangs on the last bits of the libm's cos / sin / atan2.  The
        // certain path above never gets here with such a product (it needs ener > 1e-200 and every
        // nonzero a_k > 1e-100), so checking this path sees every one.
        if (thr)
            L.libm |= ((e0 > 0.0) & (r.ener * e0 < 0x1p-1000)) | ((e1 > 0.0) & (r.ener * e1 < 0x1p-1000)) |
                      (three & (e2 > 0.0) & (r.ener * e2 < 0x1p-1000));
        if (EV && ev_here) {
            if (*ev_skip) {
                --*ev_skip;   // scored by the lane that abandoned the ray
            } else {
                const double q = expected_deposit(e0, e1, e2, r.ener * e0, r.ener * e1, r.ener * e2, t);
                eyebox_deposit(A, T, L.l, L.m, L.n, r.x, r.y, q,
                               [&]() { return replica_of(ray_gid(A, L.i), (uint32_t)A.win_reps); });
            }
        }
        if (u <= e0 && (!thr || r.ener * e0 > t)) b = 0;
        else if (u <= e0 + e1 && (!thr || r.ener * e1 > t)) b = 1;
        else if (three && u <= e0 + e1 + e2 && r.ener * e2 > t) b = 2;
        else {
            if (FATE) L.why = fate_code(freg, kFateLost);
            return kDie;
        }
    }

    if (EV && b == 2) {   // the out-coupling scores nothing more than its visit has; hit: the analog estimator's
        if (ev_here && eyebox_offset(A, T, L.l, L.m, L.n, r.x, r.y) >= 0) L.hit = true;
        return kDie;
    }
    if (b == 2) {  // out-coupling (GRTF:1162-1171, 1231-1240)
        // (the replica is the global id's, as the RNG fix-up's id above)
        const auto rep = [&]() { return replica_of(ray_gid(A, L.i), (uint32_t)A.win_reps); };
        if (STOKES) {
            // a Stokes launch (wgrt_trace_stokes; the STOKES instantiations only, as HITS below): the out-coupled
            // order's field E3, the reference's own third E_field_cal of this interaction, for an out-coupling inside
            // the rectangle -- beside it nothing is deposited
            if (eyebox_inside(T, r.x, r.y)) {
                const Field f3 = efield(r.te, r.tm, cd, sd, B + kBlockRec + 16);
                int32_t q[3];
                stokes_quanta(f3.te_re, f3.te_im, f3.tm_re, f3.tm_im, q);
                if (eyebox_bin_stokes(A, T, L.l, L.m, L.n, r.x, r.y, q[0], q[1], q[2])) L.hit = true;
            }
        } else if (HITS) {
            // a hits launch (wgrt_trace_hits; the HITS instantiations only, so that every other kernel is the code it
            // was): the record for both outcomes of the rectangle test, its index reserved by this thread's own
            // returning add (the path is rare)
            const bool in = eyebox_inside(T, r.x, r.y);
            hit_store(A.hits, A.hits_cap, atomicAdd(A.hits_count, 1ull), r.x, r.y, ray_gid(A, L.i),
                      (uint32_t)((L.l * A.nx + L.m) * A.ny + L.n), hit_flags(in, A.hits_tag));
            if (in && eyebox_bin(A, T, L.l, L.m, L.n, r.x, r.y, rep)) L.hit = true;
            if (FATE) L.why = fate_code(freg, in ? kFateEyebox : kFateBeside);
        } else if (FATE) {
            const bool in = eyebox_inside(T, r.x, r.y);
            if (in && eyebox_bin(A, T, L.l, L.m, L.n, r.x, r.y, rep)) L.hit = true;
            L.why = fate_code(freg, in ? kFateEyebox : kFateBeside);
        } else if (eyebox_add(A, T, L.l, L.m, L.n, r.x, r.y, rep)) {
            L.hit = true;
        }
        return kDie;
    }
    const Field f = efield(r.te, r.tm, cd, sd, B + kBlockRec + 8 * b);
    const double cte = hypot_cr(f.te_re, f.te_im);
    const double ctm = hypot_cr(f.tm_re, f.tm_im);
    double e = (cte * cte + ctm * ctm) * B[b] / denom;   // exact e_b (GRTF:868-869, 917-918, ...)
    if (entry) e = e * A.n_g;
    // E_field_cal's output phase (GRTF:145-150): 0 for a component below 1e-20, wrapped difference
    const double pte = cte >= 1e-20 ? atan2(f.te_im, f.te_re) : 0.0;
    const double ptm = ctm >= 1e-20 ? atan2(f.tm_im, f.tm_re) : 0.0;
    const int next = take_branch(loc, L, B, b, kind, cte, ctm, wrap_pi(ptm - pte), e);
    if (FATE && next == kDie) L.why = fate_code(freg, kFateLeftIc);
    return next;
}

// Run a ray through the loop iterations that need no Monte-Carlo interaction -- hops that
// miss every coupler slice (GRTF:1049-1052, 1102-1108, 1175-1178) and the R3 -> R4 switch
// -- until the next interaction is due.  Returns that interaction's block index, or kDie
// when the ray terminated (left eff_reg1 at GRTF:906, R5 miss at GRTF:1244-1246, or
// range(1e5) exhausted; FATE: the lane's fate is set, reason 1, 5 or 7 in the region the ray is in).
// Each iteration counts one bounce.  With `hops`, the miss hops made are added to it
// (the certification shadow turns its Jones state by as many hop phasors; everything is inlined, so the
// other callers pay nothing for it).
template <bool FATE = false, class Loc>
__device__ __forceinline__ int advance(const TraceArgs &A, const Loc &loc, Lane &L, int &kind,
                                       uint32_t *hops = nullptr) {
    Ray &r = L.r;
    const double *T = L.T;
    // A miss hop's step is fixed by the region: R2 moves by gap[0:2] and adds 2*TIR[0],
    // R3 and R4 move by gap[2:4] and add 2*TIR[1] (R5 misses die).  Fetch it once.
    const int g = (r.region == 2) ? 0 : 2;
    const double gx = T[kTileGap + g], gy = T[kTileGap + g + 1];
    const double tir2 = 2 * T[kTileTir + g / 2];   // 2*lut_TIR[...] (exact doubling)
    for (;;) {
        if (L.bounces > (uint32_t)kMaxLoop) {
            if (FATE) L.why = fate_code(r.region, kFateBounceCap);
            return kDie;
        }
        ++L.bounces;
        const Cell c = locate(loc, r.x, r.y);
        if (!in_poly(loc, c, kPolyEff1, r.x, r.y)) {
            if (FATE) L.why = fate_code(r.region, kFateLeftEff1);
            return kDie;
        }
        const int region = r.region;
        if (region <= 1) {
            kind = 0;
            return 1 + region;
        }
        int s;
        if (region <= 3) {
            s = first_slice(loc, c, kPolyFC0, A.nfc, r.x, r.y);
            if (s >= 0) {
                kind = region - 1;
                return 3 + (region - 2) * A.nfc + s;
            }
            if (region == 3 && !in_poly(loc, c, kPolyEff2, r.x, r.y)) {
                r.region = 4;   // GRTF:1103-1104: switch to the out-coupler state without moving
                continue;
            }
        } else {
            s = first_slice(loc, c, kPolyFC0 + A.nfc, A.noc, r.x, r.y);
            if (s >= 0) {
                kind = region - 1;
                return 3 + 2 * A.nfc + (region - 4) * A.noc + s;
            }
            if (region == 5) {
                if (FATE) L.why = fate_code(5, kFateOcMiss);
                return kDie;
            }
        }
        r.x += gx;
        r.y += gy;
        r.dph += tir2;   // delta_phase += 2*lut_TIR[...] (GRTF:1052, 1108, 1178)
        if (hops) ++*hops;
    }
}

template <bool FATE = false, class LaneT>
__device__ __forceinline__ void lane_retire(const TraceArgs &A, const LaneT &L) {
    A.rng[L.i] = L.r.s;
    if (A.per_ray) A.per_ray[L.i] = L.bounces;
    if (FATE) A.fate[L.i] = L.why;   // (a FATE kernel is launched with the buffer)
}

// Per-wave reduction of the ray counters, then one 64-bit atomic per non-zero counter per wave.
__device__ __forceinline__ void add_stats(wgrt_trace_stats *stats, Counters c) {
    c.wave_reduce();
    if ((threadIdx.x & 63) == 0 && stats) c.add_to(stats);
}

// The footprint sink (wgrt_trace_footprint): one count into the int64 map at flat offset off (< 0: none), called by
// every lane that is active at the call site, whatever the exec mask.  Unsigned 64-bit atomics whose result is not
// used (global_atomic_add_x2, no compare-and-swap loop): integer adds commute, so the map does not depend on their
// order.  aggregate: the lanes of the wave that hit the same entry are summed on chip -- the first pending lane's
// offset is broadcast, the lanes that share it are counted with a ballot, and the first of them adds the count; at
// most kFootprintRounds distinct offsets are served that way, and whoever is left adds its own 1.  Every ray starts
// in the in-coupler, whose few cells would otherwise take a wave's 64 adds on one address at a time.
constexpr int kFootprintRounds = 8;
__device__ __forceinline__ void footprint_add(int64_t *map, int64_t off, bool aggregate) {
    unsigned long long *const m = (unsigned long long *)map;
    bool todo = off >= 0;
    if (aggregate) {
#pragma unroll 1
        for (int round = 0; round < kFootprintRounds && __ballot(todo) != 0ull; ++round) {
            if (todo) {
                const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)(uint64_t)off);
                const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)off >> 32));
                const bool mine = (uint64_t)off == (((uint64_t)hi << 32) | lo);
                const uint64_t same = __ballot(mine);
                if (mine) {
                    const int rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(same >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)same, 0));
                    if (rank == 0) atomicAdd(m + off, (unsigned long long)__popcll(same));
                    todo = false;
                }
            }
        }
    }
    if (todo) atomicAdd(m + off, 1ull);
}

// One counted draw of wavelength l in state `region` at (x, y), its trace ended by it with fate reason `reason` (0: the
// trace goes on): channel `region`, and the reason's channel if it has one (wgrt_footprint.h).
__device__ __forceinline__ void footprint_count(const TraceArgs &A, int l, int region, int reason, double x, double y) {
    const int32_t cell = footprint_cell(A.fp, x, y);
    const bool agg = A.fp_aggregate != 0;
    footprint_add(A.fp_map, cell >= 0 ? footprint_offset(A.fp, l, region, cell) : -1, agg);
    const int c2 = footprint_end_channel(reason);
    if (c2 >= 0) footprint_add(A.fp_map, cell >= 0 ? footprint_offset(A.fp, l, c2, cell) : -1, agg);
}

// Trace ray i to termination with the reference arithmetic (variant 1's lane; replays), counted in c.  With
// s_io, the trace starts from *s_io instead of rng_states[i] and leaves its final state there
// (rng_states untouched).
// EV: with the expected-value deposits (above); skip: the scored visits to pass over.
// FP: with the footprint counts (above); skip: the counted draws to pass over.
// HITS: with the hit list's appends (interact<.., HITS>).
// PATHS: with the path list's appends (wgrt_paths.h), for a ray that A.select names: one record per draw of the bounce
// loop, numbered from 0, and the end record of a trace that advance() ends with reason 1 or 5; skip: the draws to pass
// over, recorded by the Jones lane before it abandoned the ray, which the numbering counts on from.
// STOKES: with the Stokes tables' deposits (interact<.., STOKES>).
// VISITS: with the branch counts of wgrt_trace_visits (wgrt_visits.h), for a ray whose slot is not negative: every draw
// that takes a branch, the in-coupling event's included, counts into its channel -- the branch read from where the draw
// led and the fate code interact<FATE> leaves -- and an out-coupling writes the row's end record; skip: the draws to
// pass over (the event's among them), counted by the Jones lane before it abandoned the ray.
template <bool FATE = false, bool EV = false, bool FP = false, bool HITS = false, bool PATHS = false, bool VISITS = false,
          bool STOKES = false>
__device__ __forceinline__ void trace_one(const TraceArgs &A, int64_t i, Counters &c, uint32_t *s_io = nullptr,
                                          uint32_t skip = 0) {
    static_assert(!(EV && FP) && !(EV && PATHS) && !(FP && PATHS) && !(VISITS && (EV || FP || PATHS)),
                  "a launch scores visits, counts footprints, records paths or counts branches: skip belongs to one of them");
    Lane L;
    if (!lane_load(A, i, L)) {
        ++c.w[kCtrBadRays];
        if (FATE) A.fate[i] = 0;   // no trace (wgrt_fate.h)
        return;
    }
    if (s_io) L.r.s = *s_io;
    int blk = 0, kind = 0;
    bool entry = true;
    // PATHS: whether the ray is recorded, and the ordinal of its next record
    const bool psel = PATHS && (!A.select || A.select[i] != 0);
    const int64_t pgid = psel ? ray_gid(A, L.i) : 0;   // (once per ray, not per record)
    uint32_t pstep = 0;
    // VISITS: the row the ray is counted into (< 0: it is not)
    const int64_t vrow = VISITS ? (A.vis_slot ? (int64_t)A.vis_slot[i] : i) : -1;
    for (;;) {
        // FP, PATHS: where and in which state the ray stands at this draw
        const double fx = L.r.x, fy = L.r.y;
        const int freg = L.r.region;
        const int next = interact<FATE || FP || PATHS || VISITS, EV, HITS, STOKES>(A, A.loc, L, blk, kind, entry, &skip);
        if (VISITS) {   // (blk and kind are still this draw's)
            if (skip) --skip;   // counted by the lane that abandoned the ray
            else if (vrow >= 0) {
                const int why = next < 0 ? L.why % 10 : 0;
                const bool out = why == kFateEyebox || why == kFateBeside;
                const int b = visit_branch(kind, next, why == kFateLeftIc, out);
                visit_count(A.vis_counts, A.vis_ends, A.vis_channels, vrow, b >= 0 ? visit_channel(blk, b, A.nfc, A.noc) : -1,
                            out, why == kFateEyebox, fx, fy, (uint32_t)((L.l * A.nx + L.m) * A.ny + L.n),
                            [&]() { return ray_gid(A, L.i); });
            }
        }
        if (FP && !entry) {
            if (skip) --skip;   // counted by the lane that abandoned the ray
            else footprint_count(A, L.l, freg, next < 0 ? L.why % 10 : 0, fx, fy);
        }
        if (PATHS && !entry) {
            if (skip) --skip;   // recorded by the lane that abandoned the ray
            else if (psel)
                path_store(A.paths, A.paths_cap, atomicAdd(A.paths_count, 1ull), fx, fy, pgid, pstep,
                           path_flags(freg, path_draw_kind(next < 0 ? L.why % 10 : 0), L.l, A.paths_tag));
            ++pstep;
        }
        if (next < 0) break;
        L.r.region = next;
        entry = false;
        blk = advance<FATE || PATHS>(A, A.loc, L, kind);
        if (blk < 0) {
            // PATHS: the trace ended outside a draw, where the ray stands now
            if (PATHS && psel && path_end_reason(L.why % 10))
                path_store(A.paths, A.paths_cap, atomicAdd(A.paths_count, 1ull), L.r.x, L.r.y, pgid, pstep,
                           path_flags(L.why / 10, L.why % 10, L.l, A.paths_tag));
            break;
        }
        ++c.w[kCtrInter];   // the interactions after the in-coupling event
    }
    if (s_io) *s_io = L.r.s;
    else lane_retire<FATE>(A, L);
    c.w[kCtrBounces] += L.bounces;
    c.w[kCtrHits] += L.hit;
    c.w[kCtrLibm] += L.libm ? 1u : 0u;
}

}  // namespace wgrt
