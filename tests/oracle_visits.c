/*
 * oracle_visits.c -- TEST INFRASTRUCTURE ONLY: the checker of the branch visit counts (wgrt_trace_visits).  The CPU
 * oracle (oracle/wgrt_oracle.c, untouched) with its hooks defined: at every Monte-Carlo draw
 * (ORACLE_EV(0, region, x, y)) the macro reads the oracle's own locals -- the draw u, the efficiencies e1, e2 and,
 * where they exist, e3 and the guard products en1..en3, and the slice index k -- restates the branch decision on its
 * own, and adds 1 to its own counts[row, c]; when the ray's trace has ended (ORACLE_RAY_END) the fate code -- the
 * oracle's fate_out[i], in scope there -- says whether the last draw out-coupled, and the end record is written from
 * it and that draw's position.  The channel table and the record's packing are restated here (this file does not
 * include the product's csrc/wgrt_visits.h).  An optional slot array names the row of every ray (negative: not
 * counted); the global id is gid_offset + i.  The walk is the oracle's: rng, bounces, fates and the grid come out as
 * ever.  tests/_visits.py builds this file with the oracle Makefile's flags and loads it.
 *
 * The hook sites of regions 0, 1 and 9 declare neither e3, the guard products nor k: the file-scope stand-ins below
 * are what the macro names there (the region says which of them mean anything); the oracle's locals shadow them where
 * they exist.
 */
#include <math.h>
#include <stdint.h>

#include "../oracle/wgrt_oracle.h"

static const double e3 = 0, en1 = 0, en2 = 0, en3 = 0;
static const int64_t k = 0;
/* (the hook sites that are no draw -- hops, the R3 -> R4 switch, the ends -- have no u, e1, e2 either: never used
 * there, the event test is false) */
static const double u = 2, e1 = 0, e2 = 0;

typedef struct {
    double x, y;
    int64_t gid;
    uint32_t tile, flags;
} visit_end;   /* 32 bytes: wgrt_visit_end */

static void vt_begin(int64_t i);
static void vt_draw(const wgrt_oracle_scene *sc, int region, int64_t slice, double u, double a1, double a2, double a3,
                    double g1, double g2, double g3, double x, double y);
static void vt_end(const wgrt_oracle_scene *sc, int code, int l, int m, int n);

/* (sc, u, e1, e2: in scope at every draw's hook site; ORACLE_RAY_END sits in the loop over the rays, where the ray's
 * tile is read from its columns again) */
#define ORACLE_EV(ev, region, x, y, gx, gy)                                                              \
    do {                                                                                                 \
        if ((ev) == 0) vt_draw(sc, (region), (int64_t)k, u, e1, e2, e3, en1, en2, en3, (x), (y));        \
    } while (0)
#define ORACLE_RAY_BEGIN(i) vt_begin(i)
#define ORACLE_RAY_END(i)                                                                                \
    vt_end(sc, fate_out ? fate_out[i] : 0, rays->lmd ? (int)rays->lmd[i] : 0, (int)rays->m[i], (int)rays->n[i])

#include "../oracle/wgrt_oracle.c"

/* where the counts go: set before a trace, read after it (one trace at a time) */
static uint32_t *g_counts;
static visit_end *g_ends;
static const int32_t *g_slot;
static int64_t g_rows, g_gid_offset;
static int g_channels;

/* per ray: its row (-1: not counted), its global id, and where its last draw stood */
static _Thread_local int64_t t_row, t_gid;
static _Thread_local double t_x, t_y;

/* the channel table, restated: C = 6 + 4 nfc + 6 noc */
int32_t wgrt_oracle_visit_channel(int32_t nfc, int32_t noc, int32_t state, int32_t slice, int32_t branch) {
    if (branch < 0) return -1;
    switch (state) {
    case 9: return branch < 2 ? branch : -1;
    case 0: return branch < 2 ? 2 + branch : -1;
    case 1: return branch < 2 ? 4 + branch : -1;
    case 2: return branch < 2 && slice >= 0 && slice < nfc ? 6 + 4 * slice + branch : -1;
    case 3: return branch < 2 && slice >= 0 && slice < nfc ? 6 + 4 * slice + 2 + branch : -1;
    case 4: return branch < 3 && slice >= 0 && slice < noc ? 6 + 4 * nfc + 6 * slice + branch : -1;
    case 5: return branch < 3 && slice >= 0 && slice < noc ? 6 + 4 * nfc + 6 * slice + 3 + branch : -1;
    default: return -1;
    }
}

int32_t wgrt_oracle_visit_channels(int32_t nfc, int32_t noc) { return 6 + 4 * nfc + 6 * noc; }

void wgrt_oracle_visits_set(uint32_t *counts, void *ends, int64_t rows, int32_t channels, const int32_t *slot,
                            int64_t gid_offset) {
    g_counts = counts, g_ends = (visit_end *)ends, g_rows = rows, g_channels = channels, g_slot = slot;
    g_gid_offset = gid_offset;
}

static void vt_begin(int64_t i) {
    t_gid = g_gid_offset + i;
    t_row = g_counts ? (g_slot ? (int64_t)g_slot[i] : i) : -1;
    if (t_row >= g_rows) t_row = -1;   /* (the caller's mistake: nothing is written outside the arrays) */
    t_x = t_y = 0.0;
}

static void vt_draw(const wgrt_oracle_scene *sc, int region, int64_t slice, double u, double a1, double a2, double a3,
                    double g1, double g2, double g3, double x, double y) {
    t_x = x, t_y = y;
    if (t_row < 0) return;
    /* the branch decision, restated: the in-coupler states have no guard (GRTF:860-999), R2 / R3 two guarded
     * branches (GRTF:1000-1108), R4 / R5 three (GRTF:1110-1246) */
    const double t = sc->threshold;
    int b = -1;
    if (region == 9 || region == 0 || region == 1) {
        if (u <= a1) b = 0;
        else if (u <= a1 + a2) b = 1;
    } else if (region == 2 || region == 3) {
        if (u <= a1 && g1 > t) b = 0;
        else if (u <= a1 + a2 && g2 > t) b = 1;
    } else {
        if (u <= a1 && g1 > t) b = 0;
        else if (u <= a1 + a2 && g2 > t) b = 1;
        else if (u <= a1 + a2 + a3 && g3 > t) b = 2;
    }
    const int32_t c = wgrt_oracle_visit_channel((int32_t)sc->n_fc_slices, (int32_t)sc->n_oc_slices, region,
                                                region >= 2 && region <= 5 ? (int32_t)slice : 0, b);
    if (c >= 0) {
#pragma omp atomic
        g_counts[t_row * g_channels + c] += 1u;
    }
}

static void vt_end(const wgrt_oracle_scene *sc, int code, int l, int m, int n) {
    const int reason = code % 10;
    if (t_row < 0 || !g_ends || (reason != 3 && reason != 4)) return;
    visit_end *e = g_ends + t_row;
    e->x = t_x, e->y = t_y, e->gid = t_gid;
    e->tile = (uint32_t)((l * sc->nx + m) * sc->ny + n);
    e->flags = 2u | (reason == 3 ? 1u : 0u);
}
