// wgrt_eyebox_host.cpp -- the eyebox's host-only test hooks (no GPU needed): wgrt_eyebox_evaluate_host and, at the
// end of the file, the window-table sink's (wgrt_window_plan_validate, wgrt_window_table_host).
// wgrt_eyebox_evaluate_host is the host replica of wgrt_eyebox_evaluate.  The pixel function is the one the kernels compile (wgrt_colour.h) and every sum is taken in the
// kernels' order: a position's column over a tile's FoVs in FoV order, the tiles in kEvFoldGroups contiguous
// groups in tile order, the groups in group order, the totals in position order.  What differs from the
// device is the libm behind pow / cbrt / hypot / atan2 / sin / cos / exp, and nothing else.
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/wgrt.h"
#include "wgrt_colour.h"
#include "wgrt_window.h"

namespace wgrt {
wgrt_status fail(wgrt_status s, const std::string &msg);   // wgrt_rays.hip, beside wgrt_last_error
}

using namespace wgrt;

namespace {

void px_at(const double *sums, int64_t n_fov, int64_t n_pos, int64_t f, int64_t p, double divisor, const EvConsts &k,
           double px[3]) {
    const int64_t W = 1 + n_pos, block = n_fov * W, i = f * W + 1 + p;
    ev_px(sums[i], sums[block + i], sums[2 * block + i], divisor, k, px);
}

}  // namespace

extern "C" wgrt_status wgrt_eyebox_evaluate_host(const double *sums, int64_t n_fov, int64_t n_pos, double divisor,
                                                 const double *wl, const double *lab_d65, double *out, float *image,
                                                 int64_t image_pos, void *workspace) {
    if (const char *why = ev_args_error(sums, n_fov, n_pos, divisor, wl, lab_d65, out, image, image_pos, workspace))
        return fail(WGRT_ERR_INVALID_ARGUMENT, why);
    EvConsts k;
    for (int c = 0; c < 3; ++c) k.wl[c] = wl[c], k.lab_d65[c] = lab_d65[c];
    const EvWorkspace ws = ev_workspace(workspace, n_fov, n_pos);
    const int64_t n_tiles = ev_tiles(n_fov);
    // pass 1: one partial record per (tile, position)
    for (int64_t tile = 0; tile < n_tiles; ++tile) {
        const int64_t f0 = tile * kEvTileFov, f1 = f0 + kEvTileFov < n_fov ? f0 + kEvTileFov : n_fov;
        for (int64_t p = 0; p < n_pos; ++p) {
            EvRecord r = ev_record_empty();
            for (int64_t f = f0; f < f1; ++f) {
                double px[3], Y, de;
                float h, s, v;
                px_at(sums, n_fov, n_pos, f, p, divisor, k, px);
                ev_colour(px, k, Y, de);
                ev_hsv(px, h, s, v);
                ev_record_pixel(r, de, Y, v);
            }
            const int64_t at = tile * n_pos + p;
            ws.de_sum[at] = r.de_sum;
            ws.y_min[at] = r.y_min;
            ws.y_max[at] = r.y_max;
            ws.y_sum[at] = r.y_sum;
            ws.dark[at] = r.dark;
            ws.v_max[at] = r.v_max;
        }
    }
    // pass 2: the fold
    const int64_t per = (n_tiles + kEvFoldGroups - 1) / kEvFoldGroups;
    for (int64_t p = 0; p < n_pos; ++p) {
        EvRecord r = ev_record_empty();
        for (int g = 0; g < kEvFoldGroups; ++g) {
            const int64_t lo = g * per, hi = lo + per < n_tiles ? lo + per : n_tiles;
            EvRecord q = ev_record_empty();
            for (int64_t tile = lo; tile < hi; ++tile) {
                const int64_t at = tile * n_pos + p;
                EvRecord o;
                o.de_sum = ws.de_sum[at];
                o.y_min = ws.y_min[at];
                o.y_max = ws.y_max[at];
                o.y_sum = ws.y_sum[at];
                o.dark = ws.dark[at];
                o.v_max = ws.v_max[at];
                ev_record_add(q, o);
            }
            if (g == 0) r = q;
            else ev_record_add(r, q);
        }
        double de_mean, ufov, ueb;
        ev_position(r, n_fov, de_mean, ufov, ueb);
        ws.pos_de[p] = de_mean;
        ws.pos_ufov[p] = ufov;
        ws.max_v[p] = r.v_max;
        out[3 + p] = ueb;
    }
    ev_totals(ws.pos_de, ws.pos_ufov, out + 3, n_pos, out);
    // pass 3: the image
    if (!image) return WGRT_OK;
    for (int64_t f = 0; f < n_fov; ++f)
        for (int64_t p = image_pos < 0 ? 0 : image_pos; p < (image_pos < 0 ? n_pos : image_pos + 1); ++p) {
            double px[3];
            float h, s, v, rgb[3];
            px_at(sums, n_fov, n_pos, f, p, divisor, k, px);
            ev_hsv(px, h, s, v);
            ev_image_rgb(h, s, v, ws.max_v[p], rgb);
            for (int c = 0; c < 3; ++c) {
                if (image_pos < 0) image[(f * 3 + c) * n_pos + p] = rgb[c];
                else image[f * 3 + c] = rgb[c];
            }
        }
    return WGRT_OK;
}

// The window-table sink on the host (test hooks): the plan check of wgrt_window_plan_create, and the table a
// list of hits leaves, through the membership code the trace kernels compile (wgrt_window.h).
extern "C" wgrt_status wgrt_window_plan_validate(const float *mask, int32_t ms, int32_t step_y, int32_t step_x) {
    WindowPlanView v;
    if (const char *why = window_plan_view(mask, ms, step_y, step_x, v)) return fail(WGRT_ERR_INVALID_ARGUMENT, why);
    return WGRT_OK;
}

extern "C" wgrt_status wgrt_window_table_host(const float *mask, int32_t ms, int32_t step_y, int32_t step_x,
                                              const int64_t *offsets, int64_t n, int64_t n_slabs, double *table) {
    WindowPlanView v;
    if (const char *why = window_plan_view(mask, ms, step_y, step_x, v)) return fail(WGRT_ERR_INVALID_ARGUMENT, why);
    if (n < 0 || n_slabs < 0) return fail(WGRT_ERR_INVALID_ARGUMENT, "need n >= 0 and n_slabs >= 0");
    if (n > 0 && (!offsets || (n_slabs > 0 && !table))) return fail(WGRT_ERR_INVALID_ARGUMENT, "NULL argument");
    const int64_t total = n_slabs * kEbSlabCells;
    for (int64_t k = 0; k < n; ++k)
        if (offsets[k] >= 0 && offsets[k] < total) window_visit(v, offsets[k], [table](int64_t e) { table[e] += 1.0; });
    return WGRT_OK;
}

// The fold of the replica window tables over HOST pointers: wgrt_window_replicas_fold's additions in its order.
extern "C" wgrt_status wgrt_window_replicas_fold_host(const double *reps, int32_t B, int64_t n, double *out) {
    if (B < 2 || B > WGRT_MAX_REPLICAS)
        return wgrt::fail(WGRT_ERR_INVALID_ARGUMENT, "need 2 <= B <= " + std::to_string(WGRT_MAX_REPLICAS));
    if (n < 0) return wgrt::fail(WGRT_ERR_INVALID_ARGUMENT, "need n >= 0");
    if (n == 0) return WGRT_OK;
    if (!reps || !out) return wgrt::fail(WGRT_ERR_INVALID_ARGUMENT, "NULL argument");
    for (int64_t k = 0; k < n; ++k) {
        double s = 0.0;
        for (int b = 0; b < B; ++b) s += reps[(int64_t)b * n + k];
        out[k] = s;
        for (int b = 0; b < B; ++b) out[(int64_t)(1 + b) * n + k] = s - reps[(int64_t)b * n + k];
    }
    return WGRT_OK;
}
