// wgrt_sources.hip -- a hit list re-weighted for K projector pupils and counted per entry class on the device
// (wgrt_hits_reweight_sources, wgrt_hits_source_counts; include/wgrt.h), through the rule of wgrt_sources.h.
//
//   counts    one thread per record, one 64-bit integer atomic whose result is not used.
//   prepare   weights [K, R] are quantised once per call (expected_quantize) and transposed through an LDS tile into
//             wq [R, KP], KP = 64 * chunks, the lanes beyond K zero: a wave's 64 weights of one class are then one
//             contiguous 512-byte read.
//   reweight  the shape visits_reweight_many_kernel proved: a workgroup takes kManyRows records and one chunk of 64
//             sources, a lane per source, a wave per record.  The record (a 32-byte broadcast), its range, its offset
//             and the windows that hold its bin are computed once per wave for all 64 sources; the lanes differ in the
//             deposit alone.  The deposits go into the interleaved chunk scratch [n_slabs * W, 64] and
//             visits_many_fold_kernel (wgrt_many_fold.h) adds it into the chunk's tables.  A lane whose deposit is
//             zero -- a class the source does not emit, a lane beyond K -- adds nothing.
// Every read of the list is at a record index below n; a record's tile index is checked against the scene before its
// tile is read; weights are read at k < K and r < R, wq at r < R (gid mod R of a non-negative gid) and a column below
// KP; every table write is at an entry the window membership derives from an offset guarded to [0, n_slabs * 9600),
// hence below n_slabs * W.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/wgrt.h"
#include "wgrt_many_fold.h"
#include "wgrt_scene.h"
#include "wgrt_sources.h"

using namespace wgrt;

namespace {

__device__ __forceinline__ wgrt_hit load_hit(const wgrt_hit *hits, int64_t i) {
    // the record as its two 16-byte halves
    const double2 p = ((const double2 *)(hits + i))[0];
    const ulonglong2 q = ((const ulonglong2 *)(hits + i))[1];
    wgrt_hit h;
    h.x = p.x;
    h.y = p.y;
    h.gid = (int64_t)q.x;
    h.tile = (uint32_t)q.y;
    h.flags = (uint32_t)(q.y >> 32);
    return h;
}

// Writes: counts[(l * 2 + side) * R + r] with l < nl (the tile index was checked), side 0 / 1 and r < R.
__global__ __launch_bounds__(kManyThreads) void hits_source_counts_kernel(const wgrt_hit *hits, int64_t n, int nl, int nx,
                                                                         int ny, int64_t R, int64_t *counts) {
    const int64_t i = (int64_t)blockIdx.x * kManyThreads + threadIdx.x;
    if (i >= n) return;
    const int64_t e = source_count_entry(load_hit(hits, i), nl, nx, ny, R);
    if (e >= 0) atomicAdd((unsigned long long *)counts + e, 1ull);
}

// wq[r][k] = expected_quantize(weights[k][r]) for k < K, 0 for K <= k < KP: a 64 x 64 tile per workgroup (blockIdx.x
// along r, blockIdx.y along k), read along r and written along k, both contiguous.  Reads: k < K and r < R.  Writes:
// r < R and k < KP (KP is a multiple of 64, so a tile's 64 columns are all below it).
__global__ __launch_bounds__(kManyThreads) void sources_prepare_kernel(const double *weights, int64_t R, int K, int64_t KP,
                                                                      double *wq) {
    __shared__ double tile[64][kManyStride];   // [k][r]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * 64, k0 = (int64_t)blockIdx.y * 64;
    for (int j = wave; j < 64; j += kManyThreads / 64) {
        const int64_t k = k0 + j, r = r0 + lane;
        tile[j][lane] = (k < K && r < R) ? expected_quantize(weights[k * R + r]) : 0.0;
    }
    __syncthreads();
    for (int i = wave; i < 64; i += kManyThreads / 64) {
        const int64_t r = r0 + i;
        if (r < R) wq[r * KP + k0 + lane] = tile[lane][i];
    }
}

__device__ __forceinline__ void sources_flush(int64_t *wsums, int64_t k, int nl, int l, unsigned long long s1,
                                              unsigned long long s2) {
    atomicAdd((unsigned long long *)wsums + (k * 2 + 0) * nl + l, s1);
    atomicAdd((unsigned long long *)wsums + (k * 2 + 1) * nl + l, s2);
}

// One chunk: sources k0 .. k0 + 63 (column k0 + lane of wq; the columns beyond K hold zeros).  The weight sums stay in
// registers while a wave's records share a wavelength and go to wsums as plain 64-bit vector atomics when it changes
// and at the end.  Writes: scratch[t * 64 + lane] with t < n_slabs * W; wsums[(k * 2 + i) * nl + l] with k < K (a lane
// beyond K has q == 0 throughout, so its sums stay zero and are never flushed) and l < nl (the tile was checked).
__global__ __launch_bounds__(kManyThreads) void hits_reweight_sources_kernel(const wgrt_hit *hits, int64_t n,
                                                                            const double *tiles, int tile_d, int nl, int nx,
                                                                            int ny, const WindowPlanView *plan,
                                                                            const double *wq, int64_t R, int64_t KP, int k0,
                                                                            double *scratch, int64_t *wsums) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t k = (int64_t)k0 + lane;
    const int64_t i0 = (int64_t)blockIdx.x * kManyRows;
    int cur_l = -1;                                   // (wave-uniform)
    unsigned long long s1 = 0, s2 = 0;
    for (int j = wave; j < kManyRows; j += kManyThreads / 64) {
        const int64_t i = i0 + j;                     // (wave-uniform)
        if (i >= n) break;
        const wgrt_hit h = load_hit(hits, i);
        const int64_t off = source_record_offset(h, nl, nx, ny, [=](uint32_t g, int, int) {
            return tiles + (int64_t)g * tile_d + kTileEbRange;
        });
        if (off < 0) continue;
        const double q = wq[source_index(h.gid, R) * KP + k];
        if (wsums) {
            const int l = (int)(h.tile / ((uint32_t)nx * (uint32_t)ny));
            if (l != cur_l) {
                if (s1 | s2) sources_flush(wsums, k, nl, cur_l, s1, s2);
                cur_l = l;
                s1 = s2 = 0;
            }
        }
        if (q != 0.0) {
            window_visit(*plan, off, [=](int64_t t) { unsafeAtomicAdd(scratch + t * kManyDesigns + lane, q); });
            s1 += (unsigned long long)visit_quanta(q * 0x1p32);
            s2 += (unsigned long long)visit_quanta(q * q * 0x1p32);
        }
    }
    if (wsums && (s1 | s2)) sources_flush(wsums, k, nl, cur_l, s1, s2);
}

}  // namespace

extern "C" {

wgrt_status wgrt_hits_source_counts(const wgrt_scene *s, const wgrt_hit *hits, int64_t n, int64_t R, int64_t *counts,
                                    void *stream) {
    if (!s) return fail(WGRT_ERR_INVALID_ARGUMENT, "NULL scene");
    if (const char *why = source_counts_error(hits, n, R, counts)) return fail(WGRT_ERR_INVALID_ARGUMENT, why);
    if (n == 0) return WGRT_OK;
    const int64_t blocks = (n + kManyThreads - 1) / kManyThreads;
    if (blocks > 0x7fffffff) return fail(WGRT_ERR_INVALID_ARGUMENT, "too many records for one launch");
    DEVICE_SCOPE(dev_scope, s->device);
    hipLaunchKernelGGL(hits_source_counts_kernel, dim3((unsigned)blocks), dim3(kManyThreads), 0, (hipStream_t)stream, hits,
                       n, s->nl, s->nx, s->ny, R, counts);
    HIP_TRY(hipGetLastError());
    return WGRT_OK;
}

wgrt_status wgrt_hits_reweight_sources(const wgrt_scene *s, const wgrt_window_plan *plan, const wgrt_hit *hits, int64_t n,
                                       const double *weights, int64_t R, int32_t K, double *out, int64_t *wsums,
                                       void *stream) {
    if (!s) return fail(WGRT_ERR_INVALID_ARGUMENT, "NULL scene");
    if (const char *why = source_reweight_error(plan, hits, n, weights, R, K, out, wsums))
        return fail(WGRT_ERR_INVALID_ARGUMENT, why);
    if (plan->device != s->device)
        return fail(WGRT_ERR_INVALID_ARGUMENT, "the window plan lives on device " + std::to_string(plan->device) +
                                                   ", the scene on device " + std::to_string(s->device));
    if (n == 0) return WGRT_OK;
    const int64_t blocks = (n + kManyRows - 1) / kManyRows, chunks = ((int64_t)K + kManyDesigns - 1) / kManyDesigns;
    if (blocks > 0x7fffffff) return fail(WGRT_ERR_INVALID_ARGUMENT, "too many records for one launch");
    if (chunks > 65535) return fail(WGRT_ERR_INVALID_ARGUMENT, "too many sources for one launch");
    const int64_t n_entries = (int64_t)s->nl * s->nx * s->ny * plan->host.W;
    const int64_t folds = (n_entries + 63) / 64, r_tiles = (R + 63) / 64;
    if (folds > 0x7fffffff) return fail(WGRT_ERR_INVALID_ARGUMENT, "too many table entries for one launch");
    if (r_tiles > 0x7fffffff) return fail(WGRT_ERR_INVALID_ARGUMENT, "too many rays per block for one launch");
    const int64_t KP = chunks * kManyDesigns;
    const hipStream_t st = (hipStream_t)stream;
    DEVICE_SCOPE(dev_scope, s->device);
    // the call's two scratches, stream-ordered: the quantised weights [R, KP] (every element written by the
    // preparation) and one chunk's deposits [n_entries, 64] (zeroed once, left zero by every fold)
    const size_t wq_bytes = (size_t)R * (size_t)KP * sizeof(double);
    const size_t bytes = (size_t)n_entries * kManyDesigns * sizeof(double);
    double *wq = nullptr, *scratch = nullptr;
    wgrt_status m = malloc_status(hipMallocAsync((void **)&wq, wq_bytes, st), "hipMallocAsync(source weights)");
    if (m != WGRT_OK) return m;
    m = malloc_status(hipMallocAsync((void **)&scratch, bytes, st), "hipMallocAsync(source scratch)");
    if (m != WGRT_OK) {
        (void)hipFreeAsync(wq, st);
        return m;
    }
    hipError_t h = hipMemsetAsync(scratch, 0, bytes, st);
    if (h == hipSuccess) {
        hipLaunchKernelGGL(sources_prepare_kernel, dim3((unsigned)r_tiles, (unsigned)chunks), dim3(kManyThreads), 0, st,
                           weights, R, (int)K, KP, wq);
        h = hipGetLastError();
    }
    for (int64_t c = 0; c < chunks && h == hipSuccess; ++c) {
        const int k0 = (int)(c * kManyDesigns), nk = K - k0 < kManyDesigns ? K - k0 : kManyDesigns;
        hipLaunchKernelGGL(hits_reweight_sources_kernel, dim3((unsigned)blocks), dim3(kManyThreads), 0, st, hits, n,
                           (const double *)s->d_tiles, s->tile_d, s->nl, s->nx, s->ny,
                           (const WindowPlanView *)plan->d_view, (const double *)wq, R, KP, k0, scratch, wsums);
        hipLaunchKernelGGL(visits_many_fold_kernel, dim3((unsigned)folds), dim3(kManyThreads), 0, st, scratch, n_entries,
                           nk, out + (int64_t)k0 * n_entries, n_entries);
        h = hipGetLastError();
    }
    const hipError_t f1 = hipFreeAsync(scratch, st), f2 = hipFreeAsync(wq, st);
    HIP_TRY(h);
    HIP_TRY(f1);
    HIP_TRY(f2);
    return WGRT_OK;
}

}  // extern "C"
