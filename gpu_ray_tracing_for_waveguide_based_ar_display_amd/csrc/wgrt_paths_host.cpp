// wgrt_paths_host.cpp -- the host twin of wgrt_paths_footprint (no GPU needed): the same records through the same rule
// (wgrt_paths.h, and through it wgrt_footprint.h) over HOST pointers.  The counts are integers, so the twin's map equals
// the device's exactly, in any order of the records.
#include <cstdint>
#include <string>

#include "../../include/wgrt.h"
#include "wgrt_paths.h"

namespace wgrt {
wgrt_status fail(wgrt_status s, const std::string &msg);   // wgrt_rays.hip, beside wgrt_last_error
}

using namespace wgrt;

extern "C" {

wgrt_status wgrt_paths_footprint_host(const wgrt_path_vertex *paths, int64_t n, int32_t num_lmd,
                                      const wgrt_footprint_plan *fp, int64_t *map) {
    if (const char *why = footprint_plan_error(fp)) return fail(WGRT_ERR_INVALID_ARGUMENT, why);
    if (n < 0 || num_lmd < 1 || num_lmd > kPathMaxLmd)
        return fail(WGRT_ERR_INVALID_ARGUMENT, "need n >= 0 and 1 <= num_lmd <= 256");
    if (n == 0) return WGRT_OK;
    if (!paths || !map) return fail(WGRT_ERR_INVALID_ARGUMENT, "NULL paths / map");
    for (int64_t k = 0; k < n; ++k) {
        int64_t a, b;
        path_footprint_offsets(*fp, num_lmd, paths[k].x, paths[k].y, paths[k].flags, &a, &b);
        if (a >= 0) map[a] += 1;
        if (b >= 0) map[b] += 1;
    }
    return WGRT_OK;
}

}  // extern "C"
