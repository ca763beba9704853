// wgrt_jones_lane.h -- the Jones-vector lane of the per-ray state machine (variants 7 / 9, the product
// path): certified decisions, side-effect-free abandon + replay.
#pragma once

#include "wgrt_args.h"
#include "wgrt_exact_lane.h"   // eyebox_inside: the rectangle test of a scored visit (EV)
#include "wgrt_expected.h"
#include "wgrt_locator.h"
#include "wgrt_seg.h"
#include "wgrt_stokes.h"

namespace wgrt {

// ----------------------------------------------------------------------------
// Jones-vector path (variants 7-9): certified decisions, side-effect-free abandon + replay
// ----------------------------------------------------------------------------
// The reference carries a ray's polarisation as (|Ete|, |Etm|, delta_phase) and re-derives it
// at every taken branch through hypot, atan2 and a wrap (E_field_cal, GRTF:132-152; the
// branch bodies GRTF:872-882, ...).  Up to a global phase that triple is the Jones vector
// E = (|Ete|, |Etm| e^{i delta}): E_field_cal applies a 2x2 complex matrix to it, the branch
// efficiencies are |M E|^2 times a cosine ratio, and taking a branch normalises M E and turns
// its TM component by e^{i lut_TIR} (a miss hop by e^{2 i lut_TIR}).  These variants carry E
// itself -- no hypot, atan2, wrap, sin or cos per interaction, one reciprocal square root for
// the normalisation -- and keep every Monte-Carlo decision the reference's by certifying it:
// a decision is taken only when the draw lies farther from every branch threshold than a bound
// on the difference between this arithmetic and the reference's,
//     tol = D * |1 / cos(theta)| * max(|E|^2, 1) * sum_k W[k]     (W[k]: wgrt_common.h kBlockW),
//     D   = cert_tol * (1 + G (bounces / 100)^2),
// where cert_tol (1e-10) covers the per-step rounding of both evaluations with a wide margin and
// the quadratic term the reference's phase, which grows without a wrap over miss hops (G: the
// tile's max |lut_TIR| / pi).  A ray whose decision cannot be certified (about one in 1e9
// decisions) is abandoned with no side effect -- its RNG state, counters and eyebox cells are
// written only when it terminates -- and re-traced from its launch-start state by the
// reference-arithmetic path (the epilogue kernel).  Positions, hop counts and eyebox indices are the
// reference's exact float64 operations, as in every other variant.
//
// Latency and traffic: a ray's bounces form one dependent chain (cell word -> block -> math ->
// next position).  An interaction loads its block's single-precision part (the TIR step of each
// taken branch is pre-folded into the block's TM rows, wgrt_common.h kJ*), decides, then loads
// the taken branch's double-precision matrix and issues the cell-word load of the new position;
// a miss hop moves the ray, turns Etm by its region's hop phasor (carried in JRay::hr, hi) and
// issues the cell load of its new position.  Either cell word is read in the next pass
// (JLane::pf), so its latency overlaps the rest of the pass and the other waves'.  Out-coupled
// rays are queued (position + ray index) and binned into matrix_EB by the epilogue kernel, so
// the eyebox predicate and its divisions stay out of the wave loop.
struct JRay {
    double x, y;
    double er, ei, mr, mi;   // Jones vector (Ete, Etm), up to a global phase
    double cos_t, ener;
    double eerr;             // relative error bound of ener (threshold > 0 kernels only)
    double gx, gy;           // miss-hop move of the current region
    double hr, hi;           // miss-hop phase step e^{2 i lut_TIR} of the current region, applied at each hop
    float amp;               // bound on the amplification of the lanes' state discrepancy so far (>= 1; §2.4)
    uint32_t s;
    int region;
};

struct JLane {
    JRay r;
    uint32_t tix;            // this ray's (lambda, m, n) tile index (its Jones tile: jtiles + tix * jtile_d)
    uint32_t i;              // local ray index (variants 7 / 9: < 2^32)
    uint32_t bounces;
    uint32_t inter;          // interactions of this trace after the in-coupling event (wgrt_trace_stats.interactions)
    uint32_t k;              // fused launches: the iteration (chained launch) this trace belongs to
    uint32_t s0;             // RNG state at the start of this trace (fused launches: replay point)
    uint64_t pf;             // locator cell word of (x, y), loaded a step ahead
    uint32_t pb;             // byte locator: the cell's palette index instead (pf unused; one register for variant 9 too)
};

// The workgroup's LDS copy of the byte locator's palette (ByteLocatorT): filled once at kernel start
// (fill_palette: 256 threads, one entry each, one barrier), read where a prefetched cell is consumed.
template <class Loc>
__device__ __forceinline__ typename Loc::Word *lds_palette() {
    __shared__ typename Loc::Word pal[kPaletteMax];
    return pal;
}

template <class Loc>
__device__ __forceinline__ void fill_palette(const Loc &loc) {
    if constexpr (Loc::kByte) {
        lds_palette<Loc>()[threadIdx.x & (kPaletteMax - 1)] = loc.palette[threadIdx.x & (kPaletteMax - 1)];
        __syncthreads();
    }
}

// The cell of the lane's (new) position, issued a step ahead of its use: the word, or the byte form's index ...
template <class Loc>
__device__ __forceinline__ void prefetch_cell(const Loc &loc, JLane &L) {
    if constexpr (Loc::kByte) L.pb = locate_c(loc, L.r.x, L.r.y);
    else L.pf = locate_c(loc, L.r.x, L.r.y);
}

// ... and its cell word where it is consumed (byte form: one LDS read after the prefetch has landed).
template <class Loc>
__device__ __forceinline__ typename Loc::Word prefetched_word(const JLane &L) {
    if constexpr (Loc::kByte) return lds_palette<Loc>()[L.pb];
    else return (typename Loc::Word)L.pf;
}

// (kDieIc: what a FATE instantiation's interact returns instead of kDie where the in-coupler's second order leaves
// the in-coupler -- fate reason 6, wgrt_fate.h; every other die of interact is reason 2)
enum : int { kUncertain = -3, kOut = -4, kDieIc = -5 };

// Default bases of the certification bounds (wgrt_debug_opts overrides them per call): the
// double-precision evaluation's, and the single-precision estimate's -- 8e-6 covers the rounding
// of |M E|^2 from float matrices and vector (about 26 ulp(1) of the bound's W scale) five times
// over; wgrt_shadow.hip measures the margin.
constexpr double kCertTol = 1e-10;
constexpr double kCertTol32 = 8e-6;


// The Jones-vector lane combines per-lane predicates with & and | on purpose: no short-circuit,
// so the decision is straight-line code instead of nested divergent branches.
#pragma clang diagnostic ignored "-Wbitwise-instead-of-logical"

// Ray columns staged in LDS a work-queue chunk at a time: the wave that dequeues a chunk of
// at most 64 rays copies their nine columns (wgrt_rays order below; lmd_num 0 when absent)
// into its LDS buffer with one direct-to-LDS load per column (lane j <- ray base + j: no
// VGPR destinations, every lane of the wave busy); once they have landed, lane j turns slot j
// into the ray's start state (prep_staged), and the lanes it refills from that chunk later
// read their ray from there.  A refill then costs LDS reads instead of nine per-lane gathers,
// a memory round trip and the start phase's sincos (a refill runs in almost every bulk pass:
// the sincos on the refilled lanes alone was ~15 % of a pass's instructions; per chunk, all
// 64 lanes compute it once).
constexpr int kStageCols = 9;   // x, y, m, n, lmd_num, te, tm, delta_phase, rng
// ... and the prepared slot: x, y, tile index (kBadTix: FoV / wavelength index out of range),
// Etm's real part (lo, hi), te, Etm's imaginary part (lo, hi), rng
constexpr uint32_t kBadTix = 0xffffffffu;
typedef uint32_t __attribute__((address_space(3))) LdsU32;

__device__ __forceinline__ void glds4(const void *g, LdsU32 *dst) {
    __builtin_amdgcn_global_load_lds(g, (void __attribute__((address_space(3))) *)dst, 4, 0, 0);
}

// Issued by the lanes j < n of a wave (exec-masked): column c of ray base + j -> S[c * 64 + j].
__device__ __forceinline__ void stage_chunk(const KArgs &K, LdsU32 *S, int64_t ray) {
    glds4(KA(x) + ray, S + 0 * 64);
    glds4(KA(y) + ray, S + 1 * 64);
    glds4(KA(m) + ray, S + 2 * 64);
    glds4(KA(n) + ray, S + 3 * 64);
    const float *const cl = KA(l);
    if (cl) glds4(cl + ray, S + 4 * 64);
    glds4(KA(te) + ray, S + 5 * 64);
    glds4(KA(tm) + ray, S + 6 * 64);
    glds4(KA(dph) + ray, S + 7 * 64);
    glds4(KA(rng) + ray, S + 8 * 64);
}

// Slot j of a staged chunk (its loads have landed) -> the ray's start state, in place: lane j
// of the wave that dequeued the chunk, for every ray of it at once.
__device__ __forceinline__ void prep_staged(const TraceArgs &A, const KArgs &K, LdsU32 *S, int j) {
    const int m = (int)__uint_as_float(S[2 * 64 + j]), n = (int)__uint_as_float(S[3 * 64 + j]);
    const int l = KA(l) ? (int)__uint_as_float(S[4 * 64 + j]) : 0;
    const float ftm = __uint_as_float(S[6 * 64 + j]), d = __uint_as_float(S[7 * 64 + j]);
    const bool ok = m >= 0 && m < A.nx && n >= 0 && n < A.ny && l >= 0 && l < A.nl;
    const double tm = (double)ftm;
    double sd = 0.0, cd = 1.0;
    if (d != 0.0f) sincos((double)d, &sd, &cd);   // phase = cos + i sin (GRTF:136), exact at 0
    // te_in = Ete, tm_in = phase * Etm (GRTF:137-138)
    const double mr = cd * tm, mi = sd * tm;
    S[2 * 64 + j] = ok ? (uint32_t)((l * A.nx + m) * A.ny + n) : kBadTix;
    S[3 * 64 + j] = (uint32_t)__double_as_longlong(mr);
    S[4 * 64 + j] = (uint32_t)((uint64_t)__double_as_longlong(mr) >> 32);
    S[6 * 64 + j] = (uint32_t)__double_as_longlong(mi);
    S[7 * 64 + j] = (uint32_t)((uint64_t)__double_as_longlong(mi) >> 32);
}

// A lane's ray from slot j of a prepared chunk.  Fused launches pass the ray's hand-off granule
// address: it is loaded with the slot.  False: a bad ray (not traced).
__device__ __forceinline__ bool lane_load_staged(const LdsU32 *S, int j, int64_t i, JLane &L,
                                                 const uint64_t *granule = nullptr, uint64_t *gword = nullptr) {
    const uint32_t tix = S[2 * 64 + j];
    L.i = (uint32_t)i;
    L.tix = tix == kBadTix ? 0u : tix;
    L.r.x = (double)__uint_as_float(S[0 * 64 + j]);
    L.r.y = (double)__uint_as_float(S[1 * 64 + j]);
    L.r.er = (double)__uint_as_float(S[5 * 64 + j]);
    L.r.ei = 0.0;
    L.r.mr = __longlong_as_double((long long)(((uint64_t)S[4 * 64 + j] << 32) | S[3 * 64 + j]));
    L.r.mi = __longlong_as_double((long long)(((uint64_t)S[7 * 64 + j] << 32) | S[6 * 64 + j]));
    L.r.s = S[8 * 64 + j];
    if (granule) *gword = __hip_atomic_load(granule, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    L.r.cos_t = 1.0;
    L.r.ener = 1.0;
    L.r.eerr = 0.0;
    L.r.amp = 1.0f;
    L.r.gx = L.r.gy = 0.0;
    L.r.hr = 1.0;
    L.r.hi = 0.0;
    L.r.region = 0;
    L.bounces = 1;
    L.inter = 0;
    // L.pf is not set: the first pass runs the in-coupling interaction, which loads it (and a
    // write here would wait for the cell loads other lanes' miss hops have in flight)
    return tix != kBadTix;
}

// Fused launches, whose lanes keep a ray for a run of chained traces (wgrt_items.h): the lane's private copy of
// the prepared slot, word w of it at R[w * 64] (R is the lane's own column of its wave's block: lane-indexed,
// conflict-free).  x, y, te, Etm's real and imaginary parts; the tile index stays in JLane::tix, the RNG state in
// the ray; word kRunS0 is the caller's (the state the run began from).
constexpr int kRunS0 = 7;
constexpr int kRunCols = 8;

// Slot j of a prepared chunk -> the lane's private copy (at the ray's first start of a run).
__device__ __forceinline__ void keep_slot(const LdsU32 *S, int j, LdsU32 *R) {
    R[0 * 64] = S[0 * 64 + j];
    R[1 * 64] = S[1 * 64 + j];
    R[2 * 64] = S[5 * 64 + j];
    R[3 * 64] = S[3 * 64 + j];
    R[4 * 64] = S[4 * 64 + j];
    R[5 * 64] = S[6 * 64 + j];
    R[6 * 64] = S[7 * 64 + j];
}

// The ray's next trace of the run from the private copy: the start state lane_load_staged sets, with the ray
// index, the tile index and the RNG state (where the trace before left it) as they stand.
__device__ __forceinline__ void lane_restart(const LdsU32 *R, JLane &L) {
    L.r.x = (double)__uint_as_float(R[0 * 64]);
    L.r.y = (double)__uint_as_float(R[1 * 64]);
    L.r.er = (double)__uint_as_float(R[2 * 64]);
    L.r.ei = 0.0;
    L.r.mr = __longlong_as_double((long long)(((uint64_t)R[4 * 64] << 32) | R[3 * 64]));
    L.r.mi = __longlong_as_double((long long)(((uint64_t)R[6 * 64] << 32) | R[5 * 64]));
    L.r.cos_t = 1.0;
    L.r.ener = 1.0;
    L.r.eerr = 0.0;
    L.r.amp = 1.0f;
    L.r.gx = L.r.gy = 0.0;
    L.r.hr = 1.0;
    L.r.hi = 0.0;
    L.r.region = 0;
    L.bounces = 1;
    L.inter = 0;
}

struct JField {
    double er, ei, mr, mi;
};

struct Rec {
    double pr, pi, qr, qi, rr, ri, sr, si;
};

__device__ __forceinline__ Rec load_rec(const double *p) {
    const double2 a = *(const double2 *)p, b = *(const double2 *)(p + 2);
    const double2 c = *(const double2 *)(p + 4), d = *(const double2 *)(p + 6);
    return Rec{a.x, a.y, b.x, b.y, c.x, c.y, d.x, d.y};
}

// M E for the coefficients (p, q, r, s) of one E_field_cal call (GRTF:139-144):
// Ete' = p Ete + r Etm, Etm' = q Ete + s Etm.
__device__ __forceinline__ JField jones(const Rec &c, const JRay &r) {
    JField f;
    f.er = fma(c.pr, r.er, fma(-c.pi, r.ei, fma(c.rr, r.mr, -c.ri * r.mi)));
    f.ei = fma(c.pr, r.ei, fma(c.pi, r.er, fma(c.rr, r.mi, c.ri * r.mr)));
    f.mr = fma(c.qr, r.er, fma(-c.qi, r.ei, fma(c.sr, r.mr, -c.si * r.mi)));
    f.mi = fma(c.qr, r.ei, fma(c.qi, r.er, fma(c.sr, r.mi, c.si * r.mr)));
    return f;
}

__device__ __forceinline__ double norm2(const JField &f) {
    return fma(f.er, f.er, fma(f.ei, f.ei, fma(f.mr, f.mr, f.mi * f.mi)));
}

// 1 / d and 1 / sqrt(v) to ~1 ulp: hardware estimate + two Newton steps.
__device__ __forceinline__ double rcp_nr(double d) {
    double y = __builtin_amdgcn_rcp(d);
    y = fma(y, fma(-d, y, 1.0), y);
    return fma(y, fma(-d, y, 1.0), y);
}

__device__ __forceinline__ double rsq_nr(double v) {
    double y = __builtin_amdgcn_rsq(v);
    const double h = 0.5 * v;
    y = y * fma(-h * y, y, 1.5);
    return y * fma(-h * y, y, 1.5);
}

// |M E|^2 in single precision from the block's Hermitian form H = M^H M (the certified estimate
// of a branch efficiency's numerator): h11 |Ete|^2 + h22 |Etm|^2 + 2 Re(h12 conj(Ete) Etm),
// with a = |Ete|^2, b = |Etm|^2, (cr, ci) = conj(Ete) Etm shared by every branch.
__device__ __forceinline__ float herm_form(const float4 &h, float a, float b, float cr, float ci) {
    return fmaf(h.x, a, fmaf(h.y, b, 2.0f * fmaf(h.z, cr, -h.w * ci)));
}

// A Monte-Carlo decision of the Jones-vector lane: the branch efficiencies a_k (estimates of the
// reference's e_k), the draw u, and whether the decision is certified at bound scale `scl`
// (tol = scl * sum_k W[k]; the single-wavelength guard margins use scl * W[k]).
struct JDecision {
    double a0, a1, a2;
    bool ok, s0, s1, s2;
};

__device__ __forceinline__ void jones_decide(JDecision &d, double u, double scl, const double *B, double Wsum,
                                             bool three, bool thr, double t, double ener, double eerr) {
    const double c0 = d.a0, c1 = d.a0 + d.a1, c2 = c1 + d.a2;
    const double tol = scl * Wsum;
    // NaN anywhere fails these comparisons: such a ray is replayed by the reference arithmetic.
    // Non-short-circuit (&, |) throughout: one straight-line evaluation per lane.
    bool ok = (tol > 1e-250) & (fabs(u - c0) > tol) & (fabs(u - c1) > tol) & (!three | (fabs(u - c2) > tol));
    bool p0 = true, p1 = true, p2 = true;
    if (t == 0.0) {   // full colour (uniform branch)
        // a branch the certified draw selects has e_k > tol (it lies between two thresholds more
        // than tol from the draw), so ener * e_k > 0 holds for the reference too unless that
        // product could underflow
        ok = ok & (!thr | (ener * tol > 1e-290));
    } else if (thr) {
        // ener * e_k > threshold (GRTF:606): certified with ener's tracked relative error
        const double g0 = ener * d.a0, g1 = ener * d.a1, g2 = ener * d.a2;
        const double re = eerr + 1e-15;
        const double m0 = re * fabs(g0) + ener * scl * B[kJBlockW] * 1.01;
        const double m1 = re * fabs(g1) + ener * scl * B[kJBlockW + 1] * 1.01;
        const double m2 = re * fabs(g2) + ener * scl * B[kJBlockW + 2] * 1.01;
        p0 = g0 > t;
        p1 = g1 > t;
        p2 = g2 > t;
        ok = ok & ((u > c0) | (fabs(g0 - t) > m0)) & ((u > c1) | (fabs(g1 - t) > m1)) &
             (!three | (u > c2) | (fabs(g2 - t) > m2));
    }
    d.s0 = (u <= c0) & p0;
    d.s1 = !d.s0 & (u <= c1) & p1;
    d.s2 = !d.s0 & !d.s1 & three & (u <= c2) & p2;   // out-coupling (GRTF:1162-1171, 1231-1240)
    d.ok = ok;
}

// A block's {cosA_0, cosA_1, cosA_2, Wsum} for the estimate: cosA_0 and cosA_1 in double (the
// taken branch's efficiency uses them), cosA_2 and Wsum from their floats (the exact cosA_2 is
// read only by the rare double-precision re-evaluation, estimate64).
// The same loads also bring what the tile header would otherwise be loaded for: the phase-growth bound,
// and for block 0 (entry: the in-coupling event) the event's denominator cos(ic1) (kJBlockF32; block 0's
// cosA_2 slot holds the growth bound, and a two-branch block never reads cosA_2).
// Wsum's sign bit flags a block with a branch matrix that is not scaled-unitary (amp_blk: the
// amplification step runs there; wgrt_pack.h).
__device__ __forceinline__ double4 block_cw(const double *B, bool entry, double &growth, double &cos_ic1,
                                            bool &amp_blk) {
    const double2 c01 = *(const double2 *)(B + kJBlockCos);
    const float4 fw = *(const float4 *)(B + kJBlockF32);
    growth = (double)(entry ? fw.y : fw.z);
    cos_ic1 = __hiloint2double(__float_as_int(fw.w), __float_as_int(fw.z));
    amp_blk = __float_as_uint(fw.x) >> 31;
    return double4{c01.x, c01.y, (double)fw.y, (double)fabsf(fw.x)};
}

// The efficiencies from the single-precision Hermitian forms (the estimate every decision starts
// with).  cw = {cosA_0, cosA_1, cosA_2, Wsum}.
__device__ __forceinline__ void estimate32(JDecision &d, const double *B, const JRay &r, bool three, double inv,
                                           double f01, double inv_n_g, const double4 &cw, SegAcc *sg = nullptr) {
    const float4 *H = (const float4 *)(B + kJBlockHerm);
    const float4 h0 = H[0], h1 = H[1];
    SEG_IWAITVM(sg);   // (the third branch's form is loaded after the mark: its wait counts in s[3])
    SEG_IMARK_DEP(sg, 2, h0.x + h1.x);
    const float er = (float)r.er, ei = (float)r.ei, mr = (float)r.mr, mi = (float)r.mi;
    const float a = fmaf(er, er, ei * ei), b = fmaf(mr, mr, mi * mi);
    const float cr = fmaf(er, mr, ei * mi), ci = fmaf(er, mi, -ei * mr);
    const double q0 = (double)herm_form(h0, a, b, cr, ci), q1 = (double)herm_form(h1, a, b, cr, ci);
    double q2 = 0.0;
    if (three) q2 = (double)herm_form(H[2], a, b, cr, ci);
    d.a0 = q0 * cw.x * inv * f01;
    d.a1 = q1 * cw.y * inv * f01;
    d.a2 = three ? q2 * cw.z * inv * inv_n_g : 0.0;
}

// The same in double precision, one matrix at a time (the rare re-evaluation of a decision the
// single-precision estimate could not certify; register-light rather than fast).
__device__ __forceinline__ void estimate64(JDecision &d, const double *B, const JRay &r, bool three, double inv,
                                           double f01, double inv_n_g, const double4 &cw) {
    double q[3] = {0.0, 0.0, 0.0};
#pragma unroll 1
    for (int k = 0; k < (three ? 3 : 2); ++k) {
        const double v = norm2(jones(load_rec(B + kJBlockRec + 8 * k), r));
        q[0] = k == 0 ? v : q[0];
        q[1] = k == 1 ? v : q[1];
        q[2] = k == 2 ? v : q[2];
    }
    d.a0 = q[0] * cw.x * inv * f01;
    d.a1 = q[1] * cw.y * inv * f01;
    d.a2 = three ? q[2] * B[kJBlockCos2] * inv * inv_n_g : 0.0;
}

// Amplification of the lanes' state discrepancy ("The bound, stated").  Both lanes apply
// the same Jones matrix M to states that differ, up to a global phase, by a chordal distance eps; after the
// normalisation the distance is at most a eps / (1 - eps / rho) (first order exact: a = |det M| |E|^2 /
// |M E|^2, the stretch of the direction orthogonal to E over that of E; rho = |M E| / (sigma_max |E|)).
// For a scaled-unitary M, a = 1; a singular one contracts (a = 0); a = kappa at worst, for the least
// transmitted polarisation -- the branch the Monte-Carlo draw takes least often.  The Jones lane carries
// A = prod max(1, a_k) (JRay::amp, times 1.006 per step for the second-order term and this evaluation's
// rounding) and scales its certification bound by it; a branch with rho < 1e3 x the discrepancy bound is
// abandoned (kUncertain).  The step runs only in blocks whose branch matrices are not scaled-unitary to
// within kappa^2 <= 1 + 1e-6 (the sign bit of the block's float Wsum, wgrt_pack.h): a unitary branch has
// a <= kappa <= 1 + 5e-7 for every state, so those blocks' factors multiply to at most exp(5e-7 n), 1.05
// at the 1e5-bounce cap, which the bound's margin covers (§2.4).  It lives in the AMP instantiations of
// the trace kernel, which a launch runs when its scene has such a block (wgrt_scene::nonunitary_blocks):
// on scaled-unitary LUTs the kernel carries none of it (compiled into every launch it cost 2-4 %).
// Without the step the bound is round 5's, proven for scaled-unitary matrices only.

// |det M|^2 = det H, bounded from above from the tile's single-precision H = M^H M: the float products
// are exact in double and the float entries carry 2^-24 relative rounding, so det H lies within
// 7 2^-24 h11 h22 of this evaluation (|h12|^2 <= h11 h22).
__device__ __forceinline__ double det2_ub(const float4 &h) {
    const double hx = h.x, hy = h.y, hz = h.z, hw = h.w;
    const double d = hx * hy - (hz * hz + hw * hw);
    return fmax(d, 0.0) + 0x1p-21 * (hx * hy);
}

// The decision's half of a taken branch's amplification step, from the branch's H (single precision),
// e2 = |E|^2 and q = the discrepancy bound the decision used (cert_tol (1 + G (n / 100)^2) amp):
// pa = |det M|^2 |E|^4 (so a^2 = pa / |M E|^4), and nmin = 1e6 q^2 trace(H) |E|^2, the least |M E|^2 with
// rho >= 1e3 q (sigma_max^2 <= trace H); both rounded up into floats.
__device__ __forceinline__ void amp_prepare(const float4 &hb, double e2, double q, float &pa, float &nmin) {
    pa = (float)(det2_ub(hb) * e2 * e2 * (1.0 + 0x1p-20));
    nmin = (float)(1e6 * q * q * ((double)hb.x + (double)hb.y) * e2 * (1.0 + 0x1p-20));
}

// The take's half: amp times max(1, a) (rn = 1 / |M E| to ~1 ulp), or a negative value when |M E|^2 = n2
// is below nmin (the first-order step is not certain there: the ray is abandoned).
__device__ __forceinline__ float amp_step(float amp, float pa, float nmin, double n2, double rn) {
    const double r2 = rn * rn;
    const double a2 = (double)pa * r2 * r2;
    float out = amp;
    if (__builtin_expect(a2 > 1.0, 0)) out = (float)((double)amp * sqrt(a2) * 1.006);
    return n2 < (double)nmin ? -1.0f : out;
}

// Same contract as interact() (GRTF:860-904 and the branch bodies of GRTF:905-1246), plus
// kUncertain: the decision could not be certified; the lane's ray must be abandoned (nothing
// of it has been written) and replayed.
//
// A decision is first taken from single-precision efficiencies, certified against the bound
// scaled by A.cert_tol32 (which covers single-precision rounding of |M E|^2 with a wide margin,
// wgrt_shadow.hip measures it); the rare decision that bound leaves open is re-evaluated in
// double precision against the A.cert_tol bound, and only if that fails too is the ray
// abandoned.  The taken branch's field is always computed in double precision from its
// double-precision matrix (loaded after the decision), so the carried Jones vector and ener
// are the same values the all-double evaluation gives.
// FATE (the fate-storing instantiations, wgrt_trace_fate): the one die that is not a Monte-Carlo loss returns
// kDieIc, so the caller can tell fate reason 6 from 2; nothing else differs.
// EV (the expected-value instantiations, wgrt_trace_expected; wgrt_expected.h): a certified R4 / R5 interaction
// whose position passes the FoV's eyebox rectangle test is a scored visit: *evq is its fixed-point weight q >= 0,
// made of the lane's double-precision evaluation (estimate64's forms and r.ener) whatever precision the decision
// took, and -1 anywhere else.  The caller deposits it at the position the ray had before this call -- unless
// the call returns kUncertain, which scores nothing: the replay then scores this visit.  About 3 % of bounces
// get here; the common pass pays the kind test alone.
// STOKES (the Stokes instantiations, wgrt_trace_stokes; wgrt_stokes.h): a draw that out-couples the ray (kOut) also
// evaluates the out-coupled order's field M3 E -- block record 2, which wgrt_pack.h leaves unrotated, in double
// precision -- and leaves its three quanta in sq[0..2] for the caller's queue push.  About 2 % of rays get here, once
// each; every other path is the code it was.
template <bool SINGLE, bool AMP, bool FATE, bool EV = false, bool STOKES = false, class Loc>
__device__ __forceinline__ int interact(const TraceArgs &A, const KArgs &K, const Loc &loc, JLane &L, int blk,
                                        int kind, bool entry, SegAcc *sg = nullptr, double *evq = nullptr,
                                        int32_t *sq = nullptr) {
    JRay &r = L.r;
    const double *T = KA(jtiles) + (size_t)L.tix * (size_t)A.jtile_d;
    const double *B = T + kJHeader + kJBlock * blk;
    const bool three = kind >= 3;
    const bool thr = kind >= 1;   // the ener > threshold guard exists only in R2..R5
    const double t = SINGLE ? A.threshold : 0.0;
    // the moves of branch a (index 0) and b (index 1) of this state (GRTF:878, 894, 1027, 1040,
    // 1134, 1147, ...); each is also the miss hop of the region it leads to (R5 never hops)
    const int ga = kind >= 3 ? 2 : 0;
    const int gb = kind == 0 ? 4 : (kind >= 3 ? 6 : 2);
    double growth, cos_ic1;
    bool amp_blk;
    const double4 cw = block_cw(B, entry, growth, cos_ic1, amp_blk);
    // both branches' moves with the estimate's loads: the taken branch's new cell word can then be
    // issued together with its matrix, one memory round trip per interaction less
    const double2 mva = *(const double2 *)(T + kJGap + ga);
    const double2 mvb = *(const double2 *)(T + kJGap + gb);
    const double denom = entry ? cos_ic1 : r.cos_t;
    const double u = rng_draw_lazy(r.s, [&]() { return ray_gid_ka(K, (int64_t)L.i); });
    const double inv = rcp_nr(denom);
    const double f01 = entry ? A.n_g : 1.0;
    const double nb = (double)L.bounces * 0.01;
    const double e2 = fma(r.er, r.er, fma(r.ei, r.ei, fma(r.mr, r.mr, r.mi * r.mi)));
    const double grow = AMP ? fma(nb * nb, growth, 1.0) * (double)r.amp : fma(nb * nb, growth, 1.0);
    const double base = grow * fabs(inv) * fmax(e2, 1.0);
    JDecision d;
    estimate32(d, B, r, three, inv, f01, A.inv_n_g, cw, sg);
    jones_decide(d, u, A.cert_tol32 * base, B, cw.w, three, thr, t, r.ener, SINGLE ? r.eerr : 0.0);
    if (__builtin_expect(!d.ok, 0)) {   // rare: the double-precision evaluation
        estimate64(d, B, r, three, inv, f01, A.inv_n_g, cw);
        jones_decide(d, u, A.cert_tol * base, B, cw.w, three, thr, t, r.ener, SINGLE ? r.eerr : 0.0);
    }
    SEG_IMARK_DEP(sg, 3, d.a0 + d.a1 + d.a2 + (d.ok ? 1.0 : 0.0) + (d.s0 ? 2.0 : 0.0) + (d.s1 ? 4.0 : 0.0));
    // one exit for every outcome but a taken branch; an out-coupling is appended to the
    // out-coupling queue by the caller (at (r.x, r.y))
    const int code = !d.ok ? kUncertain : d.s2 ? kOut : !(d.s0 | d.s1) ? kDie : 0;
    if (EV) {
        *evq = -1.0;
        if (__builtin_expect(three & d.ok, 0) &&
            eyebox_inside(KA(tiles) + (int64_t)L.tix * KA(tile_d), r.x, r.y)) {
            JDecision w;
            estimate64(w, B, r, three, inv, f01, A.inv_n_g, cw);
            *evq = expected_deposit(w.a0, w.a1, w.a2, r.ener * w.a0, r.ener * w.a1, r.ener * w.a2, t);
        }
    }
    if constexpr (STOKES) {
        if (__builtin_expect(code == kOut, 0)) {
            const JField f3 = jones(load_rec(B + kJBlockRec + 16), r);
            stokes_quanta(f3.er, f3.ei, f3.mr, f3.mi, sq);
        }
    }
    if (code != 0) return code;
    const bool ba = d.s0;
    const int b = ba ? 0 : 1;
    // the taken branch's new position and its cell word (read by the next pass's advance(); kind
    // 0: below), issued together with the load of its double-precision matrix.  Only the taken
    // branch's cell word: loading both candidates' before the decision hid no more latency and
    // doubled the cell-word gathers (random 4-B reads of a 71 MB grid): 9-12 % slower on C3
    const double2 mv = ba ? mva : mvb;
    r.x = r.x + mv.x;
    r.y = r.y + mv.y;
    prefetch_cell(loc, L);
    // the phase step of the new region's miss hops (R2: 2 lut_TIR[0]; R3, R4: 2 lut_TIR[1]; the
    // in-coupler states and R5 never hop), loaded with the taken branch's matrix
    const double2 hop = *(const double2 *)(T + kJHop + ((kind == 0 || (kind <= 2 && ba)) ? 0 : 2));
#ifdef WGRT_SEG
    const Rec rec_b = load_rec(B + kJBlockRec + 8 * b);
    SEG_IWAITVM(sg);
    SEG_IMARK_DEP(sg, 4, rec_b.pr + rec_b.si + hop.x);
    const JField f = jones(rec_b, r);
#else
    const JField f = jones(load_rec(B + kJBlockRec + 8 * b), r);
#endif
    // Ete = Ete1 / norm, Etm = Etm1 / norm (GRTF:874-876); the TIR step is in the TM row
    const double n2 = norm2(f);
    if (!(n2 > 1e-300)) return kUncertain;
    const double rn = rsq_nr(n2);
    if (AMP && __builtin_expect(amp_blk, 0)) {
        // a non-unitary branch matrix: the amplification step (its inputs re-read here, off the common path)
        const float4 hb = ((const float4 *)(B + kJBlockHerm))[b];
        const double e2b = fma(r.er, r.er, fma(r.ei, r.ei, fma(r.mr, r.mr, r.mi * r.mi)));
        float pa, nmin;
        amp_prepare(hb, e2b, A.cert_tol * grow, pa, nmin);
        const float a = amp_step(r.amp, pa, nmin, n2, rn);
        if (a < 0.0f) return kUncertain;
        r.amp = a;
    }
    r.er = f.er * rn;
    r.ei = f.ei * rn;
    r.mr = f.mr * rn;
    r.mi = f.mi * rn;
    const double ab = n2 * (ba ? cw.x : cw.y) * inv * f01;   // the taken branch's efficiency, double precision
    // ener accumulates every taken branch's relative error, the in-coupler states' too (no guard there,
    // but their factors are part of ener at every later guard)
    if (SINGLE) r.eerr += A.cert_tol * base * B[kJBlockW + b] * 1.01 * rcp_nr(ab) + 1e-15;
    r.ener = r.ener * ab;
    r.cos_t = ba ? cw.x : cw.y;
    r.gx = mv.x;
    r.gy = mv.y;
    r.hr = hop.x;
    r.hi = hop.y;
    SEG_IMARK_DEP(sg, 5, r.er + r.ei + r.mr + r.mi + r.ener);
    if (kind == 0) {
        const bool in_ic = in_poly_w(loc, prefetched_word<Loc>(L), kPolyIC, r.x, r.y, &K);
        if (ba) return in_ic ? 0 : 2;
        return in_ic ? 1 : (FATE ? kDieIc : kDie);
    }
    if (kind <= 2) return ba ? 2 : 3;
    return ba ? 4 : 5;
}

// The EDGE classes a lane's loop iteration consults -- eff_reg1's, the region's slices' up to the
// first IN one, eff_reg2's in R3 -- replaced by the exact predicate's verdict (IN 1 / OUT 0) through
// the 128-B band records (in_poly_w).  Rare: 0.34 % of C3 lane-passes meet an EDGE cell.
template <class Loc>
__device__ __forceinline__ typename Loc::Word resolve_edges(const KArgs &K, const Loc &loc, typename Loc::Word w,
                                                            int region, int first, int count, double x, double y) {
    using W = typename Loc::Word;
    auto fix = [&](int k) {
        if (((w >> (2 * k)) & 3u) == 2u) {
            const bool in = in_poly_w(loc, w, k, x, y, &K);
            w = (W)((w & ~((W)3 << (2 * k))) | ((W)(in ? 1u : 0u) << (2 * k)));
        }
    };
    fix(kPolyEff1);
    if (region >= 2) {
        for (int sl = 0; sl < count; ++sl) {
            fix(first + sl);
            if (((w >> (2 * (first + sl))) & 3u) == 1u) break;
        }
        if (region == 3) fix(kPolyEff2);
    }
    return w;
}

// lowest set bit of a cell word (undefined for 0: callers guard)
__device__ __forceinline__ int low_bit(uint32_t v) { return __builtin_ctz(v); }
__device__ __forceinline__ int low_bit(uint64_t v) { return __builtin_ctzll(v); }

// Same contract as advance() for the Jones-vector lane: one loop iteration of GRTF:905-1246 that
// needs no Monte-Carlo interaction (a miss hop or the R3 -> R4 switch: kTransit), or the next
// interaction's block index, or kDie.  It tests the cell word loaded a pass earlier (JLane::pf);
// a miss hop issues the load of the next one.  The outcome is computed as selects from the cell
// word's class bits (in the word's own width: 32 bits for variant 7) -- one straight-line
// evaluation per lane -- and only lanes whose outcome hinges on an EDGE class take the (rare)
// exact path first: the earlier nested per-slice tests cost every wave-pass the exec-mask
// bookkeeping of every slice's exact test (SALU per bounce).
// FATE: a trace this iteration ends leaves its fate code in *why (wgrt_fate.h), one more select: the cap before
// eff_reg1 before the R5 miss, the oracle's order (its loop ends before the next eff_reg1 test).
template <bool FATE = false, class Loc>
__device__ __forceinline__ int advance(const TraceArgs &A, const KArgs &K, const Loc &loc, JLane &L, int &kind,
                                       uint32_t *why = nullptr) {
    using W = typename Loc::Word;
    constexpr int kBits = 8 * (int)sizeof(W);
    constexpr W kLow = (W)0x5555555555555555ull;
    constexpr W kTop = (W)1 << (kBits - 1);
    JRay &r = L.r;
    W c = prefetched_word<Loc>(L);
    const int region = r.region;
    const int nfc = A.nfc, noc = A.noc;
    // the coupler slices this region scans (GRTF:1002-1005, 1112-1115) and its blocks
    const bool fc = region <= 3;
    const int first = fc ? kPolyFC0 : kPolyFC0 + nfc, count = fc ? nfc : noc;
    const W gmask = 2 * count < kBits ? ((W)1 << (2 * count)) - (W)1 : (W)~(W)0;
    W f = (c >> (2 * first)) & gmask;
    W in = f & kLow, cand = in | ((f >> 1) & kLow);
    const bool e1edge = ((c >> (2 * kPolyEff1)) & 3u) == 2u;
    const bool sedge = region >= 2 && cand != 0 && !((in >> low_bit((W)(cand | kTop))) & 1u);
    const bool e2edge = region == 3 && cand == 0 && ((c >> (2 * kPolyEff2)) & 3u) == 2u;
    if (__builtin_expect(e1edge | sedge | e2edge, 0)) {
        c = resolve_edges(K, loc, c, region, first, count, r.x, r.y);
        // the band records' loads have all landed (a compiler-visible vmcnt(0), gfx9 encoding): an exit of the
        // exact test that leaves some in flight would otherwise make the wait insertion assume them pending
        // on every path after this rare one, and wait for every load in flight before the interaction's
        // line-0 loads -- the pass's miss-hop gathers among them
        __builtin_amdgcn_s_waitcnt(kWaitVmcnt0);
        f = (c >> (2 * first)) & gmask;
        in = f & kLow;
        cand = in | ((f >> 1) & kLow);
    }
    const bool over = L.bounces > (uint32_t)kMaxLoop;   // range(1e5) exhausted (GRTF:905)
    const bool eff1 = ((c >> (2 * kPolyEff1)) & 3u) == 1u;   // GRTF:906
    const bool eff2 = ((c >> (2 * kPolyEff2)) & 3u) == 1u;
    const bool ic = region <= 1;
    const bool hit = !ic & (cand != 0);
    const int sl = low_bit((W)(cand | kTop)) >> 1;
    const bool die = over | !eff1 | (!ic & !hit & (region == 5));           // GRTF:1244-1246
    const bool sw = !die & !ic & !hit & (region == 3) & !eff2;              // GRTF:1103-1104: R3 -> R4, no move
    const bool hop = !die & !ic & !hit & !sw;                               // miss hop
    // the region's first block: FC regions 2-3 follow the 3 in-coupler states, OC regions 4-5 both FC
    // regions (one multiply of selected operands: no divergent branch)
    const int blkbase = 3 + (fc ? 0 : 2 * nfc) + (region - (fc ? 2 : 4)) * count;
    L.bounces += over ? 0u : 1u;
    kind = ic ? 0 : region - 1;
    r.region = sw ? 4 : region;
    if (hop) {
        // miss hop (GRTF:1049-1052, 1105-1108, 1175-1178)
        r.x = r.x + r.gx;
        r.y = r.y + r.gy;
        // delta_phase += 2 lut_TIR (GRTF:1052, 1108, 1178) as a turn of Etm at the hop itself: a
        // deferred per-interaction loop ran max(hops) iterations over a wave's lanes (+3 % single
        // launch, +5 % fused on C3, +10 % on C5's short hops)
        const double mr = r.mr;
        r.mr = fma(mr, r.hr, -r.mi * r.hi);
        r.mi = fma(mr, r.hi, r.mi * r.hr);
        prefetch_cell(loc, L);   // read by the next pass
    }
    const int step = hit ? blkbase + sl : kTransit;
    const int next = ic ? 1 + region : step;
    if (FATE) *why = die ? (uint32_t)(10 * region + (over ? 7 : !eff1 ? 1 : 5)) : *why;
    return die ? kDie : next;
}

}  // namespace wgrt
