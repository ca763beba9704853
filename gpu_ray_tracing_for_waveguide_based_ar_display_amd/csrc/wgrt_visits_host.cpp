// wgrt_visits_host.cpp -- the host twins of wgrt_visits_sensitivity, wgrt_visits_reweight and wgrt_visits_reweight_many
// (no GPU needed), and the
// channel table as a callable: the same rows through the same rule (wgrt_visits.h, and through it wgrt_hits.h's bin and
// wgrt_window.h's membership) over HOST pointers.  The sensitivity's sums are integers, so the twin's table equals the
// device's exactly; the reweighted table's deposits are exp() of the same sums in the same order, and differ from the
// device's by the two libms alone.
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/wgrt.h"
#include "wgrt_visits.h"

namespace wgrt {
wgrt_status fail(wgrt_status s, const std::string &msg);   // wgrt_rays.hip, beside wgrt_last_error
}

using namespace wgrt;

namespace {

const char *host_args_error(int32_t nx, int32_t ny, int32_t num_lmd, int32_t C, const double *scene_ranges,
                            const float *mask, int32_t ms, int32_t step_y, int32_t step_x, WindowPlanView &v) {
    if (nx < 1 || ny < 1 || num_lmd < 1 || C < 1) return "need nx, ny, num_lmd, n_channels >= 1";
    if (!scene_ranges) return "NULL scene_ranges";
    return window_plan_view(mask, ms, step_y, step_x, v);
}

}  // namespace

extern "C" {

wgrt_status wgrt_visits_sensitivity_host(int32_t nx, int32_t ny, int32_t num_lmd, int32_t C, const double *scene_ranges,
                                         const float *mask, int32_t ms, int32_t step_y, int32_t step_x,
                                         const uint32_t *counts, const wgrt_visit_end *ends, int64_t n_rows, double *sens) {
    WindowPlanView v;
    if (const char *why = host_args_error(nx, ny, num_lmd, C, scene_ranges, mask, ms, step_y, step_x, v))
        return fail(WGRT_ERR_INVALID_ARGUMENT, why);
    if (const char *why = visits_reduce_error(&v, counts, ends, n_rows, sens)) return fail(WGRT_ERR_INVALID_ARGUMENT, why);
    const int64_t stride = (int64_t)num_lmd * nx * ny * v.W;
    for (int64_t r = 0; r < n_rows; ++r) {
        const int64_t off = visit_end_offset(
            ends[r], num_lmd, nx, ny, [=](uint32_t, int m, int n) { return scene_ranges + ((int64_t)m * ny + n) * 4; });
        if (off < 0) continue;
        for (int c = 0; c < C; ++c) {
            const uint32_t k = counts[r * C + c];
            if (!k) continue;
            double *const t = sens + c * stride;
            window_visit(v, off, [t, k](int64_t e) { t[e] += (double)k; });
        }
    }
    return WGRT_OK;
}

wgrt_status wgrt_visits_reweight_host(int32_t nx, int32_t ny, int32_t num_lmd, int32_t C, const double *scene_ranges,
                                      const float *mask, int32_t ms, int32_t step_y, int32_t step_x, const uint32_t *counts,
                                      const wgrt_visit_end *ends, int64_t n_rows, const double *lnscale, double *out) {
    WindowPlanView v;
    if (const char *why = host_args_error(nx, ny, num_lmd, C, scene_ranges, mask, ms, step_y, step_x, v))
        return fail(WGRT_ERR_INVALID_ARGUMENT, why);
    if (const char *why = visits_reduce_error(&v, counts, ends, n_rows, out)) return fail(WGRT_ERR_INVALID_ARGUMENT, why);
    if (n_rows > 0 && !lnscale) return fail(WGRT_ERR_INVALID_ARGUMENT, "NULL lnscale");
    for (int64_t r = 0; r < n_rows; ++r) {
        const int64_t off = visit_end_offset(
            ends[r], num_lmd, nx, ny, [=](uint32_t, int m, int n) { return scene_ranges + ((int64_t)m * ny + n) * 4; });
        if (off < 0) continue;
        const double q = expected_quantize(std::exp(visit_log_weight(counts + r * C, lnscale, C)));
        window_visit(v, off, [out, q](int64_t e) { out[e] += q; });
    }
    return WGRT_OK;
}

wgrt_status wgrt_visits_reweight_many_host(int32_t nx, int32_t ny, int32_t num_lmd, int32_t C, const double *scene_ranges,
                                           const float *mask, int32_t ms, int32_t step_y, int32_t step_x,
                                           const uint32_t *counts, const wgrt_visit_end *ends, int64_t n_rows,
                                           const double *lnscale, int32_t K, double *out, int64_t *wsums) {
    WindowPlanView v;
    if (const char *why = host_args_error(nx, ny, num_lmd, C, scene_ranges, mask, ms, step_y, step_x, v))
        return fail(WGRT_ERR_INVALID_ARGUMENT, why);
    if (const char *why = visits_reduce_error(&v, counts, ends, n_rows, out)) return fail(WGRT_ERR_INVALID_ARGUMENT, why);
    if (const char *why = visits_many_error(lnscale, K, wsums)) return fail(WGRT_ERR_INVALID_ARGUMENT, why);
    const int64_t stride = (int64_t)num_lmd * nx * ny * v.W;
    for (int64_t r = 0; r < n_rows; ++r) {
        const int64_t off = visit_end_offset(
            ends[r], num_lmd, nx, ny, [=](uint32_t, int m, int n) { return scene_ranges + ((int64_t)m * ny + n) * 4; });
        if (off < 0) continue;
        const int64_t l = ends[r].tile / ((uint32_t)nx * (uint32_t)ny);
        for (int64_t k = 0; k < K; ++k) {
            // (the non-zero counts only, as the kernel walks them: the same bits, wgrt_visits.h)
            const double q = expected_quantize(std::exp(visit_log_weight_sparse(counts + r * C, lnscale + k * C, C)));
            double *const t = out + k * stride;
            window_visit(v, off, [t, q](int64_t e) { t[e] += q; });
            if (wsums) {
                wsums[(k * 2 + 0) * num_lmd + l] += visit_quanta(q * 0x1p32);
                wsums[(k * 2 + 1) * num_lmd + l] += visit_quanta(q * q * 0x1p32);
            }
        }
    }
    return WGRT_OK;
}

int32_t wgrt_visit_channel_host(int32_t n_fc, int32_t n_oc, int32_t state, int32_t slice, int32_t branch) {
    if (n_fc < 0 || n_oc < 0) return -1;
    return visit_channel_of(state, slice, branch, n_fc, n_oc);
}

int32_t wgrt_visit_channel_count_host(int32_t n_fc, int32_t n_oc) {
    return (n_fc < 0 || n_oc < 0) ? -1 : visit_channel_count(n_fc, n_oc);
}

}  // extern "C"
