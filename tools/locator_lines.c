/* locator_lines.c -- analysis tool (not product code): which cells of the locator grid one launch's gathers touch,
 * and how an LRU cache of a given size serves them under different layouts of the grid.
 *
 * It compiles the CPU oracle (oracle/wgrt_oracle.c) into this translation unit with the event hook (ORACLE_EV), as
 * tools/hop_runs.c does, and keeps every position whose cell the Jones-vector lane would gather: the position of
 * every loop iteration (an interaction, a miss hop, a termination) except the one after an R3 -> R4 switch, which
 * does not move the ray (the lane re-reads the cell it holds).  The in-coupling event gathers nothing: the cell of
 * the position its taken branch leads to is the first iteration's.  Cells are indexed as the kernels do
 * (csrc/wgrt_locator.h locate_c: truncation, then a clamp into the grid).
 * Built and driven by tools/locator_lines.py (ctypes).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
    uint8_t ev;
    double x, y;
} ll_event;

#define LL_MAX_EV 200000
static __thread ll_event *ll_buf;
static __thread int ll_n;

#define ORACLE_EV(ev_, region_, x_, y_, gx_, gy_)                                                  \
    do {                                                                                           \
        if ((region_) != 9) { /* (9: the in-coupling event, before the loop) */                   \
            if (ll_n < LL_MAX_EV) {                                                                \
                ll_buf[ll_n].ev = (uint8_t)(ev_);                                                  \
                ll_buf[ll_n].x = (x_);                                                             \
                ll_buf[ll_n].y = (y_);                                                             \
            }                                                                                      \
            ++ll_n;                                                                                \
        }                                                                                          \
    } while (0)

#include "../oracle/wgrt_oracle.c"

/* One launch of rays [0, n_rays): every gathered cell as (ray, bounce index within the ray, ix, iy, flags), flags
 * bit 0 = the position lay outside the grid (clamped).  Returns the number of gathers (the arrays hold `cap`; a
 * larger count means they were too small), -1 on allocation failure.  bounces_out: the launch's bounce total. */
int64_t ll_trace(const wgrt_oracle_scene *sc, const wgrt_oracle_rays *rays, int64_t n_rays, int64_t gid_offset,
                 uint32_t *rng, float *eb, double x0, double y0, double inv_h, int ncx, int ncy, int32_t *o_ray,
                 int32_t *o_k, int16_t *o_ix, int16_t *o_iy, uint8_t *o_flags, int64_t cap, int64_t *bounces_out,
                 int n_threads) {
    int64_t total = 0, bounces = 0;
    int failed = 0;
#ifdef _OPENMP
    if (n_threads > 0) omp_set_num_threads(n_threads);
#endif
#pragma omp parallel reduction(+ : bounces)
    {
        ll_buf = (ll_event *)malloc(LL_MAX_EV * sizeof(ll_event));
        if (!ll_buf) {
#pragma omp atomic write
            failed = 1;
        }
#pragma omp barrier
        if (!failed) {
#pragma omp for schedule(dynamic, 256)
            for (int64_t i = 0; i < n_rays; ++i) {
                ll_n = 0;
                bounces += trace_one(sc, rays, i, gid_offset + i, rng, eb, NULL);
                const int n = ll_n < LL_MAX_EV ? ll_n : LL_MAX_EV;
                int g = 0;
                for (int k = 0; k < n; ++k) g += !(k > 0 && ll_buf[k - 1].ev == 2);
                int64_t at;
#pragma omp atomic capture
                {
                    at = total;
                    total += g;
                }
                for (int k = 0; k < n; ++k) {
                    if (k > 0 && ll_buf[k - 1].ev == 2) continue;
                    if (at < cap) {
                        /* locate_c: (int) of the scaled offset (NaN and out-of-range values convert to the
                         * clamp's ends on the device; here through the double clamp first) */
                        double fx = (ll_buf[k].x - x0) * inv_h, fy = (ll_buf[k].y - y0) * inv_h;
                        const int out = !(fx > -1.0 && fy > -1.0 && fx < (double)ncx && fy < (double)ncy);
                        if (!(fx > -1.0)) fx = 0.0;
                        if (!(fy > -1.0)) fy = 0.0;
                        if (fx > (double)ncx) fx = (double)ncx;
                        if (fy > (double)ncy) fy = (double)ncy;
                        int ix = (int)fx, iy = (int)fy;
                        ix = ix < 0 ? 0 : (ix > ncx - 1 ? ncx - 1 : ix);
                        iy = iy < 0 ? 0 : (iy > ncy - 1 ? ncy - 1 : iy);
                        o_ray[at] = (int32_t)i;
                        o_k[at] = k;
                        o_ix[at] = (int16_t)ix;
                        o_iy[at] = (int16_t)iy;
                        o_flags[at] = (uint8_t)out;
                    }
                    ++at;
                }
            }
        }
        free(ll_buf);
    }
    if (failed) return -1;
    if (bounces_out) *bounces_out = bounces;
    return total;
}

/* Misses of an LRU cache of `capacity` lines over the line ids seq[0 .. n) (each < n_lines): an intrusive list over
 * the line ids.  -1 on allocation failure. */
int64_t ll_lru(const int32_t *seq, int64_t n, int32_t n_lines, int64_t capacity) {
    int32_t *prev = (int32_t *)malloc((size_t)n_lines * sizeof(int32_t));
    int32_t *next = (int32_t *)malloc((size_t)n_lines * sizeof(int32_t));
    uint8_t *in = (uint8_t *)calloc((size_t)n_lines, 1);
    if (!prev || !next || !in) {
        free(prev);
        free(next);
        free(in);
        return -1;
    }
    int32_t head = -1, tail = -1;   /* head: most recent */
    int64_t held = 0, misses = 0;
    for (int64_t j = 0; j < n; ++j) {
        const int32_t l = seq[j];
        if (in[l]) {
            if (l == head) continue;
            /* unlink */
            next[prev[l]] = next[l];
            if (next[l] >= 0) prev[next[l]] = prev[l];
            else tail = prev[l];
        } else {
            ++misses;
            if (held == capacity) {
                const int32_t t = tail;
                tail = prev[t];
                if (tail >= 0) next[tail] = -1;
                else head = -1;
                in[t] = 0;
                --held;
            }
            in[l] = 1;
            ++held;
        }
        prev[l] = -1;
        next[l] = head;
        if (head >= 0) prev[head] = l;
        head = l;
        if (tail < 0) tail = l;
    }
    free(prev);
    free(next);
    free(in);
    return misses;
}
