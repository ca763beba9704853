// wgrt_hits_host.cpp -- the host twin of wgrt_hits_grid (no GPU needed): the same records through the same rule
// (wgrt_hits.h) over HOST pointers.  The counts are integers, so the twin's grid equals the device's exactly, in any
// order of the records.
#include <cstdint>
#include <string>

#include "../../include/wgrt.h"
#include "wgrt_hits.h"

namespace wgrt {
wgrt_status fail(wgrt_status s, const std::string &msg);   // wgrt_rays.hip, beside wgrt_last_error
}

using namespace wgrt;

extern "C" {

wgrt_status wgrt_hits_grid_host(int32_t nx, int32_t ny, int32_t num_lmd, const double *scene_ranges, const wgrt_hit *hits,
                                int64_t n, const double *ranges, int32_t H, int32_t W, float *grid) {
    if (nx < 1 || ny < 1 || num_lmd < 1) return fail(WGRT_ERR_INVALID_ARGUMENT, "need nx, ny, num_lmd >= 1");
    if (n < 0) return fail(WGRT_ERR_INVALID_ARGUMENT, "negative n");
    if (const char *why = hits_grid_shape_error((int64_t)num_lmd * nx * ny, H, W))
        return fail(WGRT_ERR_INVALID_ARGUMENT, why);
    if (n == 0) return WGRT_OK;
    if (!hits || !grid) return fail(WGRT_ERR_INVALID_ARGUMENT, "NULL hits / grid");
    if (!ranges && !scene_ranges) return fail(WGRT_ERR_INVALID_ARGUMENT, "NULL scene_ranges and ranges");
    for (int64_t k = 0; k < n; ++k) {
        const int64_t off = hits_record_offset(
            hits[k], num_lmd, nx, ny, [=](uint32_t, int m, int nn) { return scene_ranges + ((int64_t)m * ny + nn) * 4; },
            ranges, H, W);
        if (off >= 0) grid[off] += 1.0f;
    }
    return WGRT_OK;
}

}  // extern "C"
