// wgrt_sources_host.cpp -- the host twins of wgrt_hits_source_counts and wgrt_hits_reweight_sources (no GPU needed): the
// same records through the same rule (wgrt_sources.h, and through it wgrt_hits.h's bin and wgrt_window.h's membership)
// over HOST pointers.  The deposits are on the 2^-32 grid and the sums integers, so the twins' tables, sums and counts
// equal the device's exactly, in any order of the records.  The twins also check what the device entry points leave to
// the caller: every weight finite and in [0, 1024].
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/wgrt.h"
#include "wgrt_sources.h"

namespace wgrt {
wgrt_status fail(wgrt_status s, const std::string &msg);   // wgrt_rays.hip, beside wgrt_last_error
}

using namespace wgrt;

extern "C" {

wgrt_status wgrt_hits_source_counts_host(int32_t nx, int32_t ny, int32_t num_lmd, const wgrt_hit *hits, int64_t n, int64_t R,
                                         int64_t *counts) {
    if (nx < 1 || ny < 1 || num_lmd < 1) return fail(WGRT_ERR_INVALID_ARGUMENT, "need nx, ny, num_lmd >= 1");
    if (const char *why = source_counts_error(hits, n, R, counts)) return fail(WGRT_ERR_INVALID_ARGUMENT, why);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t e = source_count_entry(hits[i], num_lmd, nx, ny, R);
        if (e >= 0) counts[e] += 1;
    }
    return WGRT_OK;
}

wgrt_status wgrt_hits_reweight_sources_host(int32_t nx, int32_t ny, int32_t num_lmd, const double *scene_ranges,
                                            const float *mask, int32_t ms, int32_t step_y, int32_t step_x,
                                            const wgrt_hit *hits, int64_t n, const double *weights, int64_t R, int32_t K,
                                            double *out, int64_t *wsums) {
    if (nx < 1 || ny < 1 || num_lmd < 1) return fail(WGRT_ERR_INVALID_ARGUMENT, "need nx, ny, num_lmd >= 1");
    if (!scene_ranges) return fail(WGRT_ERR_INVALID_ARGUMENT, "NULL scene_ranges");
    WindowPlanView v;
    if (const char *why = window_plan_view(mask, ms, step_y, step_x, v)) return fail(WGRT_ERR_INVALID_ARGUMENT, why);
    if (const char *why = source_reweight_error(&v, hits, n, weights, R, K, out, wsums))
        return fail(WGRT_ERR_INVALID_ARGUMENT, why);
    for (int64_t i = 0; i < (int64_t)K * R; ++i)
        if (!(weights[i] >= 0.0 && weights[i] <= kSourceMaxWeight))   // (a NaN fails both)
            return fail(WGRT_ERR_INVALID_ARGUMENT, "weights must be finite and in [0, 1024]: weights[" +
                                                       std::to_string(i / R) + "][" + std::to_string(i % R) + "] is not");
    const int64_t stride = (int64_t)num_lmd * nx * ny * v.W;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t off = source_record_offset(
            hits[i], num_lmd, nx, ny, [=](uint32_t, int m, int nn) { return scene_ranges + ((int64_t)m * ny + nn) * 4; });
        if (off < 0) continue;
        const int64_t r = source_index(hits[i].gid, R), l = hits[i].tile / ((uint32_t)nx * (uint32_t)ny);
        for (int64_t k = 0; k < K; ++k) {
            const double q = expected_quantize(weights[k * R + r]);
            if (q == 0.0) continue;
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

}  // extern "C"
