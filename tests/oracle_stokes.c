/*
 * oracle_stokes.c -- TEST INFRASTRUCTURE ONLY: the checker of the Stokes window tables (wgrt_trace_stokes).  The CPU
 * oracle (oracle/wgrt_oracle.c, untouched) with its hooks defined: every Monte-Carlo draw of an out-coupler state
 * (ORACLE_EV(0, 4 | 5, x, y)) remembers the oracle's own st.x, st.y and its own out-coupled field E3 -- the local of
 * trace_one that the third efield_amp of the interaction has just filled -- in thread-locals; when the ray's trace has
 * ended (ORACLE_RAY_END), its fate code -- the oracle's fate_out[i], in scope there -- says whether that last draw
 * out-coupled the ray inside its eyebox rectangle (reason 3), and the trace then adds the draw's three quanta to three
 * int64 grids of matrix_EB's shape, and 1 to a fourth, at eb_add's offset and under its guard.  The Stokes rule is
 * restated here on its own (this file does not include the product's csrc/wgrt_stokes.h).  The walk is the oracle's:
 * rng, bounces and the analog grid come out as ever.  tests/_stokes.py builds this file with the oracle Makefile's
 * flags and loads it.
 */
#include <math.h>
#include <stdint.h>

#include "../oracle/wgrt_oracle.h"

static void stokes_draw(double x, double y, double ar, double ai, double br, double bi);
static void stokes_begin(void);
static void stokes_end(const wgrt_oracle_scene *sc, int code, int l, int m, int n);

/* (E3: trace_one's local, in scope at every hook site; read only where the oracle has just computed it) */
#define ORACLE_EV(ev, region, x, y, gx, gy)                                            \
    do {                                                                               \
        if ((ev) == 0 && ((region) == 4 || (region) == 5))                             \
            stokes_draw((x), (y), E3.te_re, E3.te_im, E3.tm_re, E3.tm_im);             \
    } while (0)
#define ORACLE_RAY_BEGIN(i) stokes_begin()
/* (sc, rays, fate_out: wgrt_oracle_trace's, in scope at the hook site) */
#define ORACLE_RAY_END(i)                                                                                  \
    stokes_end(sc, fate_out ? fate_out[i] : 0, rays->lmd ? (int)rays->lmd[i] : 0, (int)rays->m[i], (int)rays->n[i])

#include "../oracle/wgrt_oracle.c"

/* where the deposits go: set before a trace, read after it (one trace at a time) */
static int64_t *g_stokes;   /* [3, L, NY, NX, 80, 120] int64: the sum of q_k per bin */
static int64_t *g_count;    /* [L, NY, NX, 80, 120] int64: the deposits per bin */

static _Thread_local double t_x, t_y, t_ar, t_ai, t_br, t_bi;
static _Thread_local int t_draws;

void wgrt_oracle_stokes_set(int64_t *stokes, int64_t *count) {
    g_stokes = stokes;
    g_count = count;
}

/* The rule, restated: a = (ar, ai) the complex TE amplitude, b = (br, bi) the complex TM amplitude;
 * q_k = rint(s_k * 2^30) with s1 = (|a|^2 - |b|^2) / S0, s2 = 2 Re(a conj b) / S0, s3 = 2 Im(conj a b) / S0,
 * S0 = |a|^2 + |b|^2; zeros unless S0 is positive and finite.  Every product that feeds a sum is an explicit fma. */
void wgrt_oracle_stokes_q(double ar, double ai, double br, double bi, int32_t *q) {
    const double aa = fma(ar, ar, ai * ai), bb = fma(br, br, bi * bi);
    const double s0 = aa + bb;
    q[0] = q[1] = q[2] = 0;
    if (!(s0 > 0.0) || isinf(s0)) return;
    const double re = fma(ar, br, ai * bi);
    const double im = fma(ar, bi, -(ai * br));
    q[0] = (int32_t)nearbyint((aa - bb) / s0 * 1073741824.0);   /* ties to even in the default rounding mode */
    q[1] = (int32_t)nearbyint((re + re) / s0 * 1073741824.0);
    q[2] = (int32_t)nearbyint((im + im) / s0 * 1073741824.0);
}

static void stokes_begin(void) { t_draws = 0; }

static void stokes_draw(double x, double y, double ar, double ai, double br, double bi) {
    t_x = x, t_y = y;
    t_ar = ar, t_ai = ai, t_br = br, t_bi = bi;
    ++t_draws;
}

static void stokes_end(const wgrt_oracle_scene *sc, int code, int l, int m, int n) {
    if (!(t_draws > 0 && (code / 10 == 4 || code / 10 == 5) && code % 10 == 3)) return;
    int32_t q[3];
    wgrt_oracle_stokes_q(t_ar, t_ai, t_br, t_bi, q);
    /* eb_add's offset (GRTF:164) and its guard */
    const double *rg = sc->eff_reg_fov_range + 4 * ((int64_t)m * sc->ny + n);
    double dx = (rg[1] - rg[0]) / EB_NX;
    double dy = (rg[3] - rg[2]) / EB_NY;
    int64_t ix = (int64_t)floor((t_x - rg[0]) / dx);
    int64_t iy = (int64_t)floor((t_y - rg[2]) / dy);
    if (ix < 0) ix += EB_NX;
    if (iy < 0) iy += EB_NY;
    int64_t off = ((((int64_t)l * sc->ny + n) * sc->nx + m) * EB_NY + iy) * EB_NX + ix;
    int64_t total = (int64_t)sc->num_lmd * sc->ny * sc->nx * EB_NY * EB_NX;
    if (off >= 0 && off < total && g_stokes) {
        for (int k = 0; k < 3; ++k) {
#pragma omp atomic
            g_stokes[k * total + off] += q[k];
        }
#pragma omp atomic
        g_count[off] += 1;
    }
}
