/*
 * oracle_expected.c -- TEST INFRASTRUCTURE ONLY: the checker of the expected-value eyebox estimator
 * (wgrt_trace_expected).  The CPU oracle (oracle/wgrt_oracle.c, untouched) with its event hook ORACLE_EV defined:
 * every Monte-Carlo draw of an out-coupler state (regions 4 and 5) hands the reference's own efficiencies e1, e2,
 * e3 and guard products en1, en2, en3 -- locals of the oracle at that site -- to ev_deposit below, which restates
 * the weight rule on its own (it does not include the product's csrc/wgrt_expected.h), applies the FoV's eyebox
 * rectangle test and eb_add's offset rule, and adds q to a float64 grid of matrix_EB's shape and 1 to an int64
 * grid of deposit counts.  The walk is the oracle's: rng, bounces and the analog grid come out as ever.
 *
 * The hook sites outside regions 4 / 5 do not declare all of those locals: the file-scope stand-ins below are
 * what the macro names there (never used: the region test is false); the oracle's locals shadow them where they
 * exist.  tests/_expected.py builds this file with the oracle Makefile's flags and loads it.
 */
#include <math.h>
#include <stdint.h>

#include "../oracle/wgrt_oracle.h"

static const double e1 = 0, e2 = 0, e3 = 0, en1 = 1, en2 = 1, en3 = 1;

static void ev_deposit(const wgrt_oracle_scene *sc, int l, int m, int n, int64_t i, uint32_t bounce, double x, double y,
                       double a1, double a2, double a3, double g1, double g2, double g3);

/* (sc, l, m, n, i, bounces: trace_one's parameters and locals, in scope at every hook site) */
#define ORACLE_EV(ev, region, x, y, gx, gy)                                                                   \
    do {                                                                                                      \
        if ((ev) == 0 && ((region) == 4 || (region) == 5))                                                    \
            ev_deposit(sc, l, m, n, i, bounces, (x), (y), e1, e2, e3, en1, en2, en3);                         \
    } while (0)

#include "../oracle/wgrt_oracle.c"

/* where the deposits go: set before a trace, read after it (one trace at a time) */
static double *g_weight;    /* [L, NY, NX, 80, 120] float64: the sum of q per bin */
static int64_t *g_count;    /* the same shape: deposits (q > 0) per bin */
static uint32_t *g_first;   /* per ray: the bounce number of its first deposit (0: none); may be NULL */

void wgrt_oracle_expected_set(double *weight, int64_t *count, uint32_t *first) {
    g_weight = weight;
    g_count = count;
    g_first = first;
}

/* q of one interaction, for the weight rule's own unit test */
double wgrt_oracle_expected_q(double a1, double a2, double a3, double g1, double g2, double g3, double t) {
    double w = 0.0;
    if (g3 > t) {
        double lo = 0.0;
        if (g2 > t) lo = a1 + a2;
        else if (g1 > t) lo = a1;
        double hi = a1 + a2 + a3;
        if (hi > 1.0) hi = 1.0;
        if (lo > 1.0) lo = 1.0;
        w = hi - lo;
        if (w < 0.0) w = 0.0;
    }
    return nearbyint(w * 4294967296.0) / 4294967296.0;   /* ties to even in the default rounding mode */
}

static void ev_deposit(const wgrt_oracle_scene *sc, int l, int m, int n, int64_t i, uint32_t bounce, double x, double y,
                       double a1, double a2, double a3, double g1, double g2, double g3) {
    const double *rect = sc->eff_reg_fov + 8 * ((int64_t)m * sc->ny + n);
    if (!inside_or_on_edge(x, y, rect, 4)) return;
    const double q = wgrt_oracle_expected_q(a1, a2, a3, g1, g2, g3, sc->threshold);
    if (!(q > 0.0)) return;
    if (g_first && g_first[i] == 0u) g_first[i] = bounce;   /* (ray i is traced by one thread) */
    /* eb_add's offset (GRTF:164) */
    const double *rg = sc->eff_reg_fov_range + 4 * ((int64_t)m * sc->ny + n);
    double dx = (rg[1] - rg[0]) / EB_NX;
    double dy = (rg[3] - rg[2]) / EB_NY;
    int64_t ix = (int64_t)floor((x - rg[0]) / dx);
    int64_t iy = (int64_t)floor((y - rg[2]) / dy);
    if (ix < 0) ix += EB_NX;
    if (iy < 0) iy += EB_NY;
    int64_t off = ((((int64_t)l * sc->ny + n) * sc->nx + m) * EB_NY + iy) * EB_NX + ix;
    int64_t total = (int64_t)sc->num_lmd * sc->ny * sc->nx * EB_NY * EB_NX;
    if (off >= 0 && off < total) {
#pragma omp atomic
        g_weight[off] += q;
#pragma omp atomic
        g_count[off] += 1;
    }
}
