// wgrt_footprint_host.cpp -- the footprint maps' host-only entry points (no GPU needed): the plan check of
// wgrt_trace_footprint alone, and wgrt_footprint_bin_host, the host twin of the kernels' sink through the same
// binning rule (wgrt_footprint.h).  The counts are integers, so the twin's map equals the device's exactly, in any
// order of the points.
#include <cstdint>
#include <string>

#include "../../include/wgrt.h"
#include "wgrt_footprint.h"

namespace wgrt {
wgrt_status fail(wgrt_status s, const std::string &msg);   // wgrt_rays.hip, beside wgrt_last_error
}

using namespace wgrt;

extern "C" {

wgrt_status wgrt_footprint_plan_validate(const wgrt_footprint_plan *fp) {
    if (const char *why = footprint_plan_error(fp)) return fail(WGRT_ERR_INVALID_ARGUMENT, why);
    return WGRT_OK;
}

wgrt_status wgrt_footprint_bin_host(const wgrt_footprint_plan *fp, const double *x, const double *y, const int32_t *l,
                                    const int32_t *channel, int64_t n, int32_t num_lmd, int64_t *map) {
    if (const char *why = footprint_plan_error(fp)) return fail(WGRT_ERR_INVALID_ARGUMENT, why);
    if (n < 0 || num_lmd < 1) return fail(WGRT_ERR_INVALID_ARGUMENT, "need n >= 0 and num_lmd >= 1");
    if (n > 0 && (!x || !y || !l || !channel || !map)) return fail(WGRT_ERR_INVALID_ARGUMENT, "NULL x / y / l / channel / map");
    for (int64_t i = 0; i < n; ++i) {
        if (l[i] < 0 || l[i] >= num_lmd || channel[i] < 0 || channel[i] >= kFootprintChannels) continue;
        const int32_t cell = footprint_cell(*fp, x[i], y[i]);
        if (cell < 0) continue;
        map[footprint_offset(*fp, l[i], channel[i], cell)] += 1;
    }
    return WGRT_OK;
}

const char *wgrt_footprint_channel_name(int c) { return footprint_channel_name(c); }

}  // extern "C"
