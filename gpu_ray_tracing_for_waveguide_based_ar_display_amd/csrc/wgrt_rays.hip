// wgrt_rays.hip -- the entry points that need no scene: ray setup (wgrt_rays_init), the device math
// self-test, and the library's status / error / version queries (include/wgrt.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/wgrt.h"
#include "wgrt_common.h"
#include "wgrt_host.h"

using namespace wgrt;

namespace wgrt {
thread_local std::string g_last_error;
wgrt_status fail(wgrt_status s, const std::string &msg) {
    g_last_error = msg;
    return s;
}
}  // namespace wgrt

namespace {

// Ray setup of FoV x wavelength blocks [blk_lo, blk_lo + n / R) (reference MAIN:65-115, 158):
// ray i of block b = (ii * ny + jj) * nl + k takes origin point r = i % R (TE half) or
// r - R/2 (TM half); m = ii, n = jj, lmd_num = lambdas[k]; gap / angles / phase 0.  With an
// odd R the reference leaves the last ray of every block all-zero (its two halves cover
// 2 * floor(R / 2) rays), and so does this.
struct RayInitArgs {
    const double *points;   // [R / 2, 2]
    float *col[12];         // wgrt_ray_columns order, NULL = not written
    uint32_t *rng;
    int64_t n, R, blk_lo, gid_offset;
    int ny, nl;
    float lambdas[8];
};

__global__ __launch_bounds__(256) void rays_init_kernel(RayInitArgs A) {
    const int64_t half = A.R / 2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < A.n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t blk = A.blk_lo + i / A.R, r = i % A.R;
        const int k = (int)(blk % A.nl);
        const int64_t fov = blk / A.nl;
        const int jj = (int)(fov % A.ny), ii = (int)(fov / A.ny);
        float v[12] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (r < 2 * half) {
            const int64_t p = r < half ? r : r - half;
            v[0] = (float)A.points[2 * p];       // x    (float64 -> float32, round to nearest)
            v[1] = (float)A.points[2 * p + 1];   // y
            v[6] = (float)ii;                    // m
            v[7] = (float)jj;                    // n
            v[8] = A.lambdas[k];                 // lmd_num
            v[9] = r < half ? 1.f : 0.f;         // te
            v[10] = r < half ? 0.f : 1.f;        // tm
        }
#pragma unroll
        for (int c = 0; c < 12; ++c)
            if (A.col[c]) A.col[c][i] = v[c];
        if (A.rng) A.rng[i] = 0x9E3779B9u * (uint32_t)(A.gid_offset + i + 1);   // MAIN:158, mod 2^32
    }
}

__global__ __launch_bounds__(256) void selftest_math_kernel(const double *a, const double *b, int64_t n,
                                                            double *out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = a[i], y = b[i];
    out[0 * n + i] = sqrt(x);
    out[1 * n + i] = x / y;
    out[2 * n + i] = hypot_cr(x, y);
    out[3 * n + i] = atan2(x, y);
    double s, c;
    sincos(x, &s, &c);
    out[4 * n + i] = s;
    out[5 * n + i] = c;
    out[6 * n + i] = wrap_pi(x);
}

}  // namespace

extern "C" {

wgrt_status wgrt_rays_init(const double *points, int64_t rays_per_fov, int32_t nx, int32_t ny,
                           const int32_t *lambdas, int32_t n_lambdas, int64_t block_lo, int64_t block_hi,
                           const wgrt_ray_columns *out, uint32_t *rng_states, void *stream) {
    if (!out || !lambdas) return fail(WGRT_ERR_INVALID_ARGUMENT, "NULL columns / lambdas");
    if (rays_per_fov < 1 || nx < 1 || ny < 1) return fail(WGRT_ERR_INVALID_ARGUMENT, "sizes must be positive");
    if (n_lambdas < 1 || n_lambdas > 8) return fail(WGRT_ERR_INVALID_ARGUMENT, "1..8 wavelengths");
    const int64_t nblk = (int64_t)nx * ny * n_lambdas;
    if (block_lo < 0 || block_lo > block_hi || block_hi > nblk)
        return fail(WGRT_ERR_INVALID_ARGUMENT, "block range outside [0, nx * ny * n_lambdas]");
    if (rays_per_fov >= 2 && !points) return fail(WGRT_ERR_INVALID_ARGUMENT, "NULL points");
    RayInitArgs A{};
    A.points = points;
    float *const cols[12] = {out->x, out->y, out->gap_x, out->gap_y, out->pol, out->azi, out->m, out->n,
                             out->lmd_num, out->te, out->tm, out->delta_phase};
    for (int c = 0; c < 12; ++c) A.col[c] = cols[c];
    A.rng = rng_states;
    A.n = (block_hi - block_lo) * rays_per_fov;
    A.R = rays_per_fov;
    A.blk_lo = block_lo;
    A.gid_offset = block_lo * rays_per_fov;
    A.ny = ny;
    A.nl = n_lambdas;
    for (int k = 0; k < n_lambdas; ++k) A.lambdas[k] = (float)lambdas[k];
    if (A.n == 0) return WGRT_OK;
    // no scene: the kernel runs on the stream's device
    int sdev = 0;
    HIP_TRY(stream_device(stream, &sdev));
    DEVICE_SCOPE(dev_scope, sdev);
    const int64_t blocks = std::min<int64_t>((A.n + 255) / 256, 65536);
    hipLaunchKernelGGL(rays_init_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, A);
    HIP_TRY(hipGetLastError());
    return WGRT_OK;
}

wgrt_status wgrt_selftest_math(const double *a, const double *b, int64_t n, double *out, void *stream) {
    if (n > 0 && (!a || !b || !out)) return fail(WGRT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n <= 0) return WGRT_OK;
    int sdev = 0;
    HIP_TRY(stream_device(stream, &sdev));
    DEVICE_SCOPE(dev_scope, sdev);
    const int64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(selftest_math_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, b,
                       n, out);
    HIP_TRY(hipGetLastError());
    return WGRT_OK;
}

const char *wgrt_status_string(wgrt_status s) {
    switch (s) {
        case WGRT_OK: return "ok";
        case WGRT_ERR_INVALID_ARGUMENT: return "invalid argument";
        case WGRT_ERR_HIP: return "HIP runtime error";
        case WGRT_ERR_OUT_OF_MEMORY: return "out of device memory";
        case WGRT_ERR_UNSUPPORTED: return "unsupported";
    }
    return "unknown status";
}

const char *wgrt_last_error(void) { return g_last_error.c_str(); }

int wgrt_abi_version(void) { return WGRT_ABI_VERSION; }

}  // extern "C"
