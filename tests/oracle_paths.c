/*
 * oracle_paths.c -- TEST INFRASTRUCTURE ONLY: the checker of the path lists (wgrt_trace_paths).  The CPU oracle
 * (oracle/wgrt_oracle.c, untouched) with its hooks defined: every Monte-Carlo draw of the bounce loop
 * (ORACLE_EV(0, region != 9, x, y)) appends a draw record at the oracle's own st.x, st.y with the ray's thread-local
 * step counter; a termination by the loop-top eff_reg1 test or an R5 miss (ORACLE_EV(3, region, x, y)) appends an end
 * record; and when the ray's trace has ended (ORACLE_RAY_END), its fate code -- the oracle's fate_out[i], in scope
 * there -- gives the last draw its kind (reasons 2 / 3 / 4; never for a code 9x, whose trace made no draw) and the
 * end record its kind (reasons 1 / 5).  The record's packing is restated here (this file does not include the
 * product's csrc/wgrt_paths.h).  An optional select mask names the rays that are recorded; the global id is
 * gid_offset + i.  The walk is the oracle's: rng, bounces, fates and the grid come out as ever.  tests/_paths.py
 * builds this file with the oracle Makefile's flags and loads it.
 */
#include <math.h>
#include <stdint.h>

#include "../oracle/wgrt_oracle.h"

typedef struct {
    double x, y;
    int64_t gid;
    uint32_t step, flags;
} path_rec;   /* 32 bytes: wgrt_path_vertex */

static void pt_begin(int64_t i);
static void pt_event(int l, int region, int end, double x, double y);
static void pt_end(int code);

/* (l: trace_one's local, in scope at every hook site) */
#define ORACLE_EV(ev, region, x, y, gx, gy)                                   \
    do {                                                                      \
        if ((ev) == 0 && (region) != 9) pt_event(l, (region), 0, (x), (y));   \
        else if ((ev) == 3) pt_event(l, (region), 1, (x), (y));               \
    } while (0)
#define ORACLE_RAY_BEGIN(i) pt_begin(i)
#define ORACLE_RAY_END(i) pt_end(fate_out ? fate_out[i] : 0)

#include "../oracle/wgrt_oracle.c"

/* where the records go: set before a trace, read after it (one trace at a time) */
static path_rec *g_rec;
static int64_t g_cap, g_n, g_gid_offset;
static const uint8_t *g_select;
static uint32_t g_tag;

/* per ray: its global id, whether it is recorded, its next step, and where its last draw / its end record went
 * (-1: none, or not stored) */
static _Thread_local int64_t t_gid, t_last_draw, t_end;
static _Thread_local int t_on, t_draws;
static _Thread_local uint32_t t_step;

void wgrt_oracle_paths_set(void *rec, int64_t cap, int64_t gid_offset, const uint8_t *select, uint32_t tag) {
    g_rec = (path_rec *)rec, g_cap = cap, g_n = 0, g_gid_offset = gid_offset, g_select = select, g_tag = tag;
}

/* the records made since _set (whether or not the buffer had room for them) */
int64_t wgrt_oracle_paths_recorded(void) { return g_n; }

static void pt_begin(int64_t i) {
    t_gid = g_gid_offset + i;
    t_on = g_rec && (!g_select || g_select[i] != 0);
    t_step = 0, t_draws = 0, t_last_draw = -1, t_end = -1;
}

static void pt_event(int l, int region, int end, double x, double y) {
    if (!end) ++t_draws;
    if (t_on) {
        int64_t k;
#pragma omp atomic capture
        k = g_n++;
        if (k < g_cap) {
            g_rec[k].x = x, g_rec[k].y = y, g_rec[k].gid = t_gid, g_rec[k].step = t_step;
            /* kind 0 until the fate is known */
            g_rec[k].flags = (uint32_t)region | (uint32_t)l << 8 | g_tag << 16;
            if (end) t_end = k;
            else t_last_draw = k;
        }
    }
    ++t_step;
}

static void pt_end(int code) {
    const int reason = code % 10;
    /* reasons 2 / 3 / 4 of a trace that made a draw in the loop end at that draw (a trace lost at the in-coupling
     * event, code 92, made none); reasons 1 / 5 end at the end record */
    if (t_last_draw >= 0 && t_draws > 0 && code / 10 != 9 && reason >= 2 && reason <= 4)
        g_rec[t_last_draw].flags |= (uint32_t)reason << 4;
    if (t_end >= 0 && (reason == 1 || reason == 5)) g_rec[t_end].flags |= (uint32_t)reason << 4;
}
