// wgrt_visits.hip -- the two reductions of a table of counted rays on the device (wgrt_visits_sensitivity,
// wgrt_visits_reweight, include/wgrt.h) and the scene's channel count, through the rule of wgrt_visits.h.
//
// The table is small -- the driver counts the delivered rays only, a few per cent of a launch -- and each delivered
// row deposits into one slab column and the windows that hold its bin, so neither kernel sums on chip first.
//   sensitivity  one wave per row: every lane reads the row's end record (one 32-byte broadcast), the lanes stride
//                over the row's C counts (a coalesced read), and a lane with a non-zero count deposits it into its
//                channel's table.  The deposits are integers in float64: exact and order-free below 2^53.
//   reweight     one thread per row, so that the row's log-weight is summed in ascending channel order with one fma
//                each, the order the host twin takes; the deposit is on the 2^-32 grid (wgrt_expected.h), so the sums
//                are exact and order-free too while an entry stays below 2^21.
// Every read is at a row below n_rows and a channel below C; a row's tile index is checked against the scene before its
// tile is read; every write is at a table entry the window membership derives from an offset guarded to
// [0, n_slabs * 9600), hence below n_slabs * W (times C for the sensitivity).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/wgrt.h"
#include "wgrt_scene.h"
#include "wgrt_visits.h"

using namespace wgrt;

namespace {

constexpr int kVisitsThreads = 256;

__device__ __forceinline__ wgrt_visit_end load_end(const wgrt_visit_end *ends, int64_t r) {
    // the record as its two 16-byte halves
    const double2 p = ((const double2 *)(ends + r))[0];
    const ulonglong2 q = ((const ulonglong2 *)(ends + r))[1];
    wgrt_visit_end e;
    e.x = p.x;
    e.y = p.y;
    e.gid = (int64_t)q.x;
    e.tile = (uint32_t)q.y;
    e.flags = (uint32_t)(q.y >> 32);
    return e;
}

__global__ __launch_bounds__(kVisitsThreads) void visits_sensitivity_kernel(const uint32_t *counts,
                                                                           const wgrt_visit_end *ends, int64_t n_rows,
                                                                           int C, const double *tiles, int tile_d, int nl,
                                                                           int nx, int ny, const WindowPlanView *plan,
                                                                           double *sens) {
    const int64_t r = (int64_t)blockIdx.x * (kVisitsThreads / 64) + (threadIdx.x >> 6);   // (wave-uniform)
    if (r >= n_rows) return;
    const int64_t off = visit_end_offset(load_end(ends, r), nl, nx, ny, [=](uint32_t g, int, int) {
        return tiles + (int64_t)g * tile_d + kTileEbRange;
    });
    if (off < 0) return;
    const int64_t stride = (int64_t)nl * nx * ny * plan->W;
    for (int c = threadIdx.x & 63; c < C; c += 64) {
        const uint32_t k = counts[r * C + c];
        if (!k) continue;
        double *const t = sens + c * stride;
        window_visit(*plan, off, [t, k](int64_t e) { unsafeAtomicAdd(t + e, (double)k); });
    }
}

__global__ __launch_bounds__(kVisitsThreads) void visits_reweight_kernel(const uint32_t *counts, const wgrt_visit_end *ends,
                                                                        int64_t n_rows, int C, const double *tiles,
                                                                        int tile_d, int nl, int nx, int ny,
                                                                        const WindowPlanView *plan, const double *lnscale,
                                                                        double *out) {
    const int64_t r = (int64_t)blockIdx.x * kVisitsThreads + threadIdx.x;
    if (r >= n_rows) return;
    const int64_t off = visit_end_offset(load_end(ends, r), nl, nx, ny, [=](uint32_t g, int, int) {
        return tiles + (int64_t)g * tile_d + kTileEbRange;
    });
    if (off < 0) return;
    const double q = expected_quantize(exp(visit_log_weight(counts + r * C, lnscale, C)));
    window_visit(*plan, off, [out, q](int64_t e) { unsafeAtomicAdd(out + e, q); });
}

wgrt_status reduce_args(const wgrt_scene *s, const wgrt_window_plan *plan, const uint32_t *counts,
                        const wgrt_visit_end *ends, int64_t n_rows, const void *out) {
    if (!s) return fail(WGRT_ERR_INVALID_ARGUMENT, "NULL scene");
    if (const char *why = visits_reduce_error(plan, counts, ends, n_rows, out)) return fail(WGRT_ERR_INVALID_ARGUMENT, why);
    if (plan->device != s->device)
        return fail(WGRT_ERR_INVALID_ARGUMENT, "the window plan lives on device " + std::to_string(plan->device) +
                                                   ", the scene on device " + std::to_string(s->device));
    return WGRT_OK;
}

}  // namespace

extern "C" {

int32_t wgrt_visit_channels(const wgrt_scene *s) { return s ? visit_channel_count(s->nfc, s->noc) : -1; }

wgrt_status wgrt_visits_sensitivity(const wgrt_scene *s, const wgrt_window_plan *plan, const uint32_t *counts,
                                    const wgrt_visit_end *ends, int64_t n_rows, double *sens, void *stream) {
    const wgrt_status e = reduce_args(s, plan, counts, ends, n_rows, sens);
    if (e != WGRT_OK) return e;
    if (n_rows == 0) return WGRT_OK;
    const int64_t blocks = (n_rows + kVisitsThreads / 64 - 1) / (kVisitsThreads / 64);
    if (blocks > 0x7fffffff) return fail(WGRT_ERR_INVALID_ARGUMENT, "too many rows for one launch");
    DEVICE_SCOPE(dev_scope, s->device);
    hipLaunchKernelGGL(visits_sensitivity_kernel, dim3((unsigned)blocks), dim3(kVisitsThreads), 0, (hipStream_t)stream,
                       counts, ends, n_rows, visit_channel_count(s->nfc, s->noc), (const double *)s->d_tiles, s->tile_d,
                       s->nl, s->nx, s->ny, (const WindowPlanView *)plan->d_view, sens);
    HIP_TRY(hipGetLastError());
    return WGRT_OK;
}

wgrt_status wgrt_visits_reweight(const wgrt_scene *s, const wgrt_window_plan *plan, const uint32_t *counts,
                                 const wgrt_visit_end *ends, int64_t n_rows, const double *lnscale, double *out,
                                 void *stream) {
    const wgrt_status e = reduce_args(s, plan, counts, ends, n_rows, out);
    if (e != WGRT_OK) return e;
    if (n_rows == 0) return WGRT_OK;
    if (!lnscale || ((uintptr_t)lnscale & 7)) return fail(WGRT_ERR_INVALID_ARGUMENT, "NULL or misaligned lnscale");
    const int64_t blocks = (n_rows + kVisitsThreads - 1) / kVisitsThreads;
    if (blocks > 0x7fffffff) return fail(WGRT_ERR_INVALID_ARGUMENT, "too many rows for one launch");
    DEVICE_SCOPE(dev_scope, s->device);
    hipLaunchKernelGGL(visits_reweight_kernel, dim3((unsigned)blocks), dim3(kVisitsThreads), 0, (hipStream_t)stream,
                       counts, ends, n_rows, visit_channel_count(s->nfc, s->noc), (const double *)s->d_tiles, s->tile_d,
                       s->nl, s->nx, s->ny, (const WindowPlanView *)plan->d_view, lnscale, out);
    HIP_TRY(hipGetLastError());
    return WGRT_OK;
}

}  // extern "C"
