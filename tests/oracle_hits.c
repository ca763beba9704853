/*
 * oracle_hits.c -- TEST INFRASTRUCTURE ONLY: the checker of the hit list (wgrt_trace_hits).  The CPU oracle
 * (oracle/wgrt_oracle.c, untouched) with its hooks defined: every Monte-Carlo draw of the bounce loop
 * (ORACLE_EV(0, region != 9, x, y)) remembers the oracle's own st.x, st.y in a thread-local; when the ray's trace has
 * ended (ORACLE_RAY_END), its fate code -- the oracle's fate_out[i], in scope there -- says whether that last draw
 * out-coupled the ray inside / outside its eyebox rectangle (reasons 3 / 4), and the trace then records
 * (x, y, gid_offset + i, tile, reason == 3).  The walk is the oracle's: rng, bounces and the grid come out as ever.
 * tests/_hits.py builds this file with the oracle Makefile's flags and loads it.
 */
#include <math.h>
#include <stdint.h>

#include "../oracle/wgrt_oracle.h"

static void hit_draw(double x, double y);
static void hit_begin(void);
static void hit_end(int code, int64_t gid, int64_t tile);

#define ORACLE_EV(ev, region, x, y, gx, gy)                 \
    do {                                                    \
        if ((ev) == 0 && (region) != 9) hit_draw((x), (y)); \
    } while (0)
#define ORACLE_RAY_BEGIN(i) hit_begin()
/* (sc, rays, gid_offset, fate_out: wgrt_oracle_trace's, in scope at the hook site) */
#define ORACLE_RAY_END(i)                                                                                          \
    hit_end(fate_out ? fate_out[i] : 0, gid_offset + (i),                                                          \
            (((int64_t)(rays->lmd ? (int)rays->lmd[i] : 0) * sc->nx + (int)rays->m[i]) * sc->ny + (int)rays->n[i]))

#include "../oracle/wgrt_oracle.c"

/* where the records go: set before a trace, read after it (one trace at a time) */
static double *g_xy;        /* (x, y) pairs ... */
static int64_t *g_gt;       /* ... and (gid, tile, inside) triples, g_cap entries each */
static int64_t g_cap, g_n;

static _Thread_local double t_x, t_y;
static _Thread_local int t_draws;

void wgrt_oracle_hits_set(double *xy, int64_t *gt, int64_t cap) {
    g_xy = xy, g_gt = gt, g_cap = cap, g_n = 0;
}

/* the out-couplings since _set (whether or not the arrays had room for them) */
int64_t wgrt_oracle_hits_recorded(void) { return g_n; }

static void hit_begin(void) { t_draws = 0; }

static void hit_draw(double x, double y) {
    t_x = x, t_y = y;
    ++t_draws;
}

static void hit_end(int code, int64_t gid, int64_t tile) {
    const int reason = code % 10;
    if (!(t_draws > 0 && code / 10 != 9 && (reason == 3 || reason == 4))) return;
    int64_t k;
#pragma omp atomic capture
    k = g_n++;
    if (g_xy && k < g_cap) {
        g_xy[2 * k] = t_x, g_xy[2 * k + 1] = t_y;
        g_gt[3 * k] = gid, g_gt[3 * k + 1] = tile, g_gt[3 * k + 2] = reason == 3;
    }
}
