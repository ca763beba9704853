// wgrt_visits.hip -- the reductions of a table of counted rays on the device (wgrt_visits_sensitivity,
// wgrt_visits_reweight and, for K designs at once, wgrt_visits_reweight_many; include/wgrt.h) and the scene's channel
// count, through the rule of wgrt_visits.h.
//
// The table is small -- the driver counts the delivered rays only, a few per cent of a launch -- and each delivered
// row deposits into one slab column and the windows that hold its bin, so no kernel sums a table on chip first.
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

#include <atomic>
#include <cstdint>
#include <string>

#include "../../include/wgrt.h"
#include "../../include/wgrt_debug.h"
#include "wgrt_many_fold.h"
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

// The ensemble (wgrt_visits_reweight_many; the rule and the zero-skipping argument: wgrt_visits.h).  A workgroup takes
// kManyRows rows and one chunk of kManyDesigns = 64 designs, a lane per design, a wave per row.
//   * The chunk's log-scales sit in LDS channel-major, lns[c * 65 + j]: the 64 lanes of a wave read 64 consecutive
//     doubles (two conflict-free bank rows), and the stride of 65 spreads the fill's writes, which run along c.
//   * A wave reads its row's end record (a broadcast) and its counts (lane c, coalesced) once, for all 64 designs.  The
//     non-zero counts are the set bits of a ballot, walked in ascending c with the count read from its lane into a
//     scalar register: every lane runs the same chain of single fmas on its own design's column.
//   * The deposits.  DIRECT adds into out[k][e]: the wave's 64 adds go to 64 tables, 64 cache lines.  INTERLEAVED
//     adds into a chunk's scratch [n_slabs * W, 64], where they are 512 contiguous bytes, and visits_many_fold_kernel
//     (wgrt_many_fold.h) then adds the scratch into the chunk's tables through an LDS transpose and zeroes it for the
//     next chunk.  Both are sums on the 2^-32 grid, so both give the same bits (wgrt_debug_set_reweight_layout picks;
//     DESIGN.md 4.13 has the timings).
//   * The weight sums stay in registers while a wave's rows share a wavelength (rows are in ray order, so they nearly
//     always do) and go to wsums as plain 64-bit vector atomics when it changes and at the end: a few per workgroup,
//     design and wavelength.
// Reads: rows below n_rows, channels below C, designs below K (a lane beyond K reads zeros and deposits nothing).
// Writes: entries below n_slabs * W (window_visit over a guarded offset) of tables k < K, hence below
// out + K * n_slabs * W; scratch entries below n_slabs * W * 64; wsums[(k * 2 + i) * nl + l] with l < nl because the
// row's tile index was checked against the scene.
// (kManyDesigns, kManyStride, kManyRows and the fold kernel: wgrt_many_fold.h, shared with wgrt_sources.hip)
constexpr size_t kManyLdsLimit = 64 * 1024;

__device__ __forceinline__ void many_flush(int64_t *wsums, int64_t k, int nl, int l, unsigned long long s1,
                                           unsigned long long s2) {
    atomicAdd((unsigned long long *)wsums + (k * 2 + 0) * nl + l, s1);
    atomicAdd((unsigned long long *)wsums + (k * 2 + 1) * nl + l, s2);
}

template <bool INTERLEAVED>
__global__ __launch_bounds__(kVisitsThreads) void visits_reweight_many_kernel(
    const uint32_t *counts, const wgrt_visit_end *ends, int64_t n_rows, int C, const double *tiles, int tile_d, int nl,
    int nx, int ny, const WindowPlanView *plan, const double *lnscale, int K, int k_first, double *dst,
    int64_t table_stride, int64_t *wsums) {
    extern __shared__ double lns[];   // [C][kManyStride]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k0 = k_first + (int)blockIdx.y * kManyDesigns;
    const int nk = K - k0 < kManyDesigns ? K - k0 : kManyDesigns;
    for (int i = threadIdx.x; i < kManyDesigns * C; i += kVisitsThreads) {
        const int j = i / C, c = i - j * C;
        lns[c * kManyStride + j] = j < nk ? lnscale[(int64_t)(k0 + j) * C + c] : 0.0;
    }
    __syncthreads();
    const bool mine = lane < nk;
    const int64_t k = k0 + lane;
    const int64_t r0 = (int64_t)blockIdx.x * kManyRows;
    int cur_l = -1;
    unsigned long long s1 = 0, s2 = 0;
    for (int i = wave; i < kManyRows; i += kVisitsThreads / 64) {
        const int64_t r = r0 + i;   // (wave-uniform)
        if (r >= n_rows) break;
        const wgrt_visit_end e = load_end(ends, r);
        const int64_t off = visit_end_offset(e, nl, nx, ny, [=](uint32_t g, int, int) {
            return tiles + (int64_t)g * tile_d + kTileEbRange;
        });
        if (off < 0) continue;
        double a = 0.0;
        for (int cb = 0; cb < C; cb += 64) {
            const int v = cb + lane < C ? (int)counts[r * C + cb + lane] : 0;
            unsigned long long m = __ballot(v != 0);
            while (m) {   // ascending c; the count from its lane, the same in every lane
                const int b = __builtin_ctzll(m);
                m &= m - 1;
                const uint32_t n = (uint32_t)__builtin_amdgcn_readlane(v, b);
                a = fma((double)n, lns[(cb + b) * kManyStride + lane], a);
            }
        }
        const double q = expected_quantize(exp(a));
        if (mine) {   // (every lane, whatever its design, has served the ballot above as a channel's lane)
            if (INTERLEAVED)
                window_visit(*plan, off, [=](int64_t t) { unsafeAtomicAdd(dst + t * kManyDesigns + lane, q); });
            else
                window_visit(*plan, off, [=](int64_t t) { unsafeAtomicAdd(dst + k * table_stride + t, q); });
        }
        if (wsums && mine) {
            const int l = (int)(e.tile / ((uint32_t)nx * (uint32_t)ny));
            if (l != cur_l) {
                if (cur_l >= 0) many_flush(wsums, k, nl, cur_l, s1, s2);
                cur_l = l;
                s1 = s2 = 0;
            }
            s1 += (unsigned long long)visit_quanta(q * 0x1p32);
            s2 += (unsigned long long)visit_quanta(q * q * 0x1p32);
        }
    }
    if (wsums && mine && cur_l >= 0) many_flush(wsums, k, nl, cur_l, s1, s2);
}

std::atomic<int> g_many_interleaved{1};   // wgrt_debug_set_reweight_layout

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

int32_t wgrt_visit_wavelengths(const wgrt_scene *s) { return s ? s->nl : -1; }

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

wgrt_status wgrt_visits_reweight_many(const wgrt_scene *s, const wgrt_window_plan *plan, const uint32_t *counts,
                                      const wgrt_visit_end *ends, int64_t n_rows, const double *lnscale, int32_t K,
                                      double *out, int64_t *wsums, void *stream) {
    const wgrt_status e = reduce_args(s, plan, counts, ends, n_rows, out);
    if (e != WGRT_OK) return e;
    if (const char *why = visits_many_error(lnscale, K, wsums)) return fail(WGRT_ERR_INVALID_ARGUMENT, why);
    if (n_rows == 0) return WGRT_OK;
    const int C = visit_channel_count(s->nfc, s->noc);
    const size_t lds = (size_t)C * kManyStride * sizeof(double);
    if (lds > kManyLdsLimit)
        return fail(WGRT_ERR_UNSUPPORTED, "a chunk of 64 designs x " + std::to_string(C) + " channels does not fit in LDS");
    const int64_t blocks = (n_rows + kManyRows - 1) / kManyRows, chunks = ((int64_t)K + kManyDesigns - 1) / kManyDesigns;
    if (blocks > 0x7fffffff) return fail(WGRT_ERR_INVALID_ARGUMENT, "too many rows for one launch");
    if (chunks > 65535) return fail(WGRT_ERR_INVALID_ARGUMENT, "too many designs for one launch");
    const int64_t n_entries = (int64_t)s->nl * s->nx * s->ny * plan->host.W;
    const hipStream_t st = (hipStream_t)stream;
    const double *const tiles = (const double *)s->d_tiles;
    const WindowPlanView *const view = (const WindowPlanView *)plan->d_view;
    DEVICE_SCOPE(dev_scope, s->device);
    if (!g_many_interleaved.load(std::memory_order_relaxed)) {
        hipLaunchKernelGGL(visits_reweight_many_kernel<false>, dim3((unsigned)blocks, (unsigned)chunks),
                           dim3(kVisitsThreads), lds, st, counts, ends, n_rows, C, tiles, s->tile_d, s->nl, s->nx, s->ny,
                           view, lnscale, K, 0, out, n_entries, wsums);
        HIP_TRY(hipGetLastError());
        return WGRT_OK;
    }
    // one chunk's scratch, stream-ordered: zeroed once, left zero by every fold
    const int64_t folds = (n_entries + 63) / 64;
    if (folds > 0x7fffffff) return fail(WGRT_ERR_INVALID_ARGUMENT, "too many table entries for one launch");
    double *scratch = nullptr;
    const size_t bytes = (size_t)n_entries * kManyDesigns * sizeof(double);
    const wgrt_status m = malloc_status(hipMallocAsync((void **)&scratch, bytes, st), "hipMallocAsync(design scratch)");
    if (m != WGRT_OK) return m;
    hipError_t h = hipMemsetAsync(scratch, 0, bytes, st);
    for (int64_t c = 0; c < chunks && h == hipSuccess; ++c) {
        const int k0 = (int)(c * kManyDesigns), nk = K - k0 < kManyDesigns ? K - k0 : kManyDesigns;
        hipLaunchKernelGGL(visits_reweight_many_kernel<true>, dim3((unsigned)blocks), dim3(kVisitsThreads), lds, st,
                           counts, ends, n_rows, C, tiles, s->tile_d, s->nl, s->nx, s->ny, view, lnscale, K, k0, scratch,
                           n_entries, wsums);
        hipLaunchKernelGGL(visits_many_fold_kernel, dim3((unsigned)folds), dim3(kManyThreads), 0, st, scratch,
                           n_entries, nk, out + (int64_t)k0 * n_entries, n_entries);
        h = hipGetLastError();
    }
    const hipError_t f = hipFreeAsync(scratch, st);
    HIP_TRY(h);
    HIP_TRY(f);
    return WGRT_OK;
}

wgrt_status wgrt_debug_set_reweight_layout(int interleaved) {
    g_many_interleaved.store(interleaved != 0, std::memory_order_relaxed);
    return WGRT_OK;
}

}  // extern "C"
