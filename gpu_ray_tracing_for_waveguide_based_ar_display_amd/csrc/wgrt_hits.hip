// wgrt_hits.hip -- a hit list binned into an eyebox grid of any resolution on the device (wgrt_hits_grid,
// include/wgrt.h), through the rule of wgrt_hits.h.
//
// One thread per record, one +1.0f atomic per record that counts: the counts are integers, so the grid does not depend
// on the order of the records while a bin stays below 2^24.  A list is a few per cent of a launch's rays, so the
// kernel is a small fraction of the trace that filled it, and nothing is summed on chip first.  Every read is at a
// record index below n; a record's tile index is checked against the scene before its tile is read; every write is at
// an offset the rule has guarded to [0, num_lmd * ny * nx * H * W).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/wgrt.h"
#include "wgrt_hits.h"
#include "wgrt_scene.h"

using namespace wgrt;

namespace {

constexpr int kHitsThreads = 256;

__global__ __launch_bounds__(kHitsThreads) void hits_grid_kernel(const wgrt_hit *hits, int64_t n, const double *tiles,
                                                                int tile_d, int nl, int nx, int ny, const double *ranges,
                                                                int32_t H, int32_t W, float *grid) {
    const int64_t k = (int64_t)blockIdx.x * kHitsThreads + threadIdx.x;
    if (k >= n) return;
    // the record as its two 16-byte halves
    const double2 p = ((const double2 *)(hits + k))[0];
    const ulonglong2 q = ((const ulonglong2 *)(hits + k))[1];
    wgrt_hit h;
    h.x = p.x;
    h.y = p.y;
    h.gid = (int64_t)q.x;
    h.tile = (uint32_t)q.y;
    h.flags = (uint32_t)(q.y >> 32);
    const int64_t off = hits_record_offset(
        h, nl, nx, ny, [=](uint32_t g, int, int) { return tiles + (int64_t)g * tile_d + kTileEbRange; }, ranges, H, W);
    if (off >= 0) unsafeAtomicAdd(grid + off, 1.0f);
}

}  // namespace

extern "C" {

wgrt_status wgrt_hits_grid(const wgrt_scene *s, const wgrt_hit *hits, int64_t n, const double *ranges, int32_t H,
                           int32_t W, float *grid, void *stream) {
    if (!s) return fail(WGRT_ERR_INVALID_ARGUMENT, "NULL scene");
    if (n < 0) return fail(WGRT_ERR_INVALID_ARGUMENT, "negative n");
    if (const char *why = hits_grid_shape_error((int64_t)s->nl * s->nx * s->ny, H, W))
        return fail(WGRT_ERR_INVALID_ARGUMENT, why);
    if (n == 0) return WGRT_OK;
    if (!hits || !grid) return fail(WGRT_ERR_INVALID_ARGUMENT, "NULL hits / grid");
    if ((uintptr_t)hits & 15) return fail(WGRT_ERR_INVALID_ARGUMENT, "the hit list must be 16-B aligned");
    const int64_t blocks = (n + kHitsThreads - 1) / kHitsThreads;
    if (blocks > 0x7fffffff) return fail(WGRT_ERR_INVALID_ARGUMENT, "too many records for one launch");
    DEVICE_SCOPE(dev_scope, s->device);
    hipLaunchKernelGGL(hits_grid_kernel, dim3((unsigned)blocks), dim3(kHitsThreads), 0, (hipStream_t)stream, hits, n,
                       (const double *)s->d_tiles, s->tile_d, s->nl, s->nx, s->ny, ranges, H, W, grid);
    HIP_TRY(hipGetLastError());
    return WGRT_OK;
}

}  // extern "C"
