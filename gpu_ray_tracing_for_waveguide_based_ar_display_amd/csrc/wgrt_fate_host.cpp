// wgrt_fate_host.cpp -- the fate census's host-only entry points (no GPU needed): wgrt_fate_census_host, the host
// twin of wgrt_fate_census through the same validity rule, tile index and column function (wgrt_fate.h), and the
// constants the other layers take from the library (wgrt_fate_col, wgrt_fate_reason_name).  The counts are
// integers, so the twin's table equals the device's exactly, in any ray order.
#include <cstdint>
#include <string>

#include "../../include/wgrt.h"
#include "wgrt_fate.h"

namespace wgrt {
wgrt_status fail(wgrt_status s, const std::string &msg);   // wgrt_rays.hip, beside wgrt_last_error
}

using namespace wgrt;

extern "C" {

wgrt_status wgrt_fate_census_host(const uint8_t *fate, const float *m, const float *n, const float *lmd_num,
                                  int64_t n_rays, int32_t nx, int32_t ny, int32_t num_lmd, int64_t *table) {
    if (const char *why = fate_census_args_error(fate, m, n, n_rays, nx, ny, num_lmd, table))
        return fail(WGRT_ERR_INVALID_ARGUMENT, why);
    for (int64_t i = 0; i < n_rays; ++i) {
        const int code = fate[i];
        if (!fate_valid(code)) continue;
        const int64_t s = fate_slab(m[i], n[i], lmd_num ? lmd_num[i] : 0.0f, lmd_num != nullptr, nx, ny, num_lmd);
        if (s < 0) continue;
        table[s * kFateCols + fate_col(code)] += 1;
    }
    return WGRT_OK;
}

int32_t wgrt_fate_col(int code) { return fate_valid(code) ? fate_col(code) : -1; }

int32_t wgrt_fate_cols(void) { return kFateCols; }

const char *wgrt_fate_reason_name(int reason) { return fate_reason_name(reason); }

}  // extern "C"
