/*
 * oracle_footprint.c -- TEST INFRASTRUCTURE ONLY: the checker of the footprint maps (wgrt_trace_footprint).  The CPU
 * oracle (oracle/wgrt_oracle.c, untouched) with its hooks defined: every Monte-Carlo draw of the bounce loop
 * (ORACLE_EV(0, region != 9, x, y)) counts into channel `region` of an int64 map at the oracle's own st.x, st.y,
 * by this file's own restatement of the binning rule (it does not include the product's csrc/wgrt_footprint.h), and
 * remembers the position in a thread-local; when the ray's trace has ended (ORACLE_RAY_END), its fate code -- the
 * oracle's fate_out[i], in scope there -- says whether that last draw lost the ray (reason 2: channel 6) or
 * out-coupled it inside / outside its eyebox rectangle (3 / 4: channels 7 / 8).  The walk is the oracle's: rng,
 * bounces and the grid come out as ever.  An optional record takes every count as (x, y, l, channel), for the host
 * twin's test.  tests/_footprint.py builds this file with the oracle Makefile's flags and loads it.
 */
#include <math.h>
#include <stdint.h>

#include "../oracle/wgrt_oracle.h"

#define FP_CHANNELS 9

static void fp_count(int l, int channel, double x, double y);
static void fp_draw(int l, int region, double x, double y);
static void fp_end(int code);

/* (l: trace_one's local, in scope at every hook site) */
#define ORACLE_EV(ev, region, x, y, gx, gy)                          \
    do {                                                             \
        if ((ev) == 0 && (region) != 9) fp_draw(l, (region), (x), (y)); \
    } while (0)
#define ORACLE_RAY_BEGIN(i) fp_begin()
#define ORACLE_RAY_END(i) fp_end(fate_out ? fate_out[i] : 0)

static void fp_begin(void);

#include "../oracle/wgrt_oracle.c"

/* the plan and where the counts go: set before a trace, read after it (one trace at a time) */
static double g_x0, g_y0, g_cx, g_cy;
static int64_t g_nx, g_ny;
static int64_t *g_map;      /* [L, 9, ny, nx] */
static double *g_rec_xy;    /* optional record of every count: (x, y) pairs ... */
static int32_t *g_rec_lc;   /* ... and (l, channel) pairs, g_rec_cap entries each */
static int64_t g_rec_cap, g_rec_n;

static _Thread_local double t_x, t_y;
static _Thread_local int t_l, t_draws;

void wgrt_oracle_footprint_set(double x0, double y0, double cell_x, double cell_y, int64_t nx_cells, int64_t ny_cells,
                               int64_t *map, double *rec_xy, int32_t *rec_lc, int64_t rec_cap) {
    g_x0 = x0, g_y0 = y0, g_cx = cell_x, g_cy = cell_y;
    g_nx = nx_cells, g_ny = ny_cells;
    g_map = map;
    g_rec_xy = rec_xy, g_rec_lc = rec_lc, g_rec_cap = rec_cap, g_rec_n = 0;
}

/* the counts made since _set (whether or not the record had room for them) */
int64_t wgrt_oracle_footprint_recorded(void) { return g_rec_n; }

static void fp_count(int l, int channel, double x, double y) {
    if (g_rec_xy) {
        int64_t k;
#pragma omp atomic capture
        k = g_rec_n++;
        if (k < g_rec_cap) {
            g_rec_xy[2 * k] = x, g_rec_xy[2 * k + 1] = y;
            g_rec_lc[2 * k] = l, g_rec_lc[2 * k + 1] = channel;
        }
    }
    if (!g_map || !isfinite(x) || !isfinite(y)) return;
    const double fx = floor((x - g_x0) / g_cx), fy = floor((y - g_y0) / g_cy);
    if (!(fx >= 0.0 && fx < (double)g_nx && fy >= 0.0 && fy < (double)g_ny)) return;
    const int64_t ix = (int64_t)fx, iy = (int64_t)fy;
    const int64_t off = (((int64_t)l * FP_CHANNELS + channel) * g_ny + iy) * g_nx + ix;
#pragma omp atomic
    g_map[off] += 1;
}

static void fp_begin(void) { t_draws = 0; }

static void fp_draw(int l, int region, double x, double y) {
    t_x = x, t_y = y, t_l = l;
    ++t_draws;
    fp_count(l, region, x, y);
}

static void fp_end(int code) {
    const int reason = code % 10;
    /* reasons 2 / 3 / 4 of a trace that made a draw in the loop end at that draw (a trace lost at the in-coupling
     * event, code 92, made none) */
    if (t_draws > 0 && code / 10 != 9 && reason >= 2 && reason <= 4) fp_count(t_l, 4 + reason, t_x, t_y);
}
