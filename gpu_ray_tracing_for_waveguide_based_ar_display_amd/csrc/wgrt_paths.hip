// wgrt_paths.hip -- a path list added into a footprint map on the device (wgrt_paths_footprint, include/wgrt.h),
// through the rule of wgrt_paths.h.
//
// A list is long (one record per draw of every recorded ray) and most of a ray's first draws fall in the in-coupler's
// few cells, so one global int64 atomic per count would run at the chip's same-address atomic rate.  Each workgroup
// takes a contiguous span of records -- the records of one wave's block, hence of one region of the plate, lie
// together in the list -- and every wave sums its counts in the footprint launch's own counter cache
// (wgrt_footprint_cache.h) before they reach the map: a count whose entry is cached is one LDS add.  With the switch of
// wgrt_debug_set_footprint_aggregate off: one global atomic per count.  Counts are integers, so the map does not
// depend on the order or the form.  Every read is at a record index below n; every write is at an offset the cell
// rule has guarded to the map [num_lmd, 9, ny_cells, nx_cells].
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/wgrt.h"
#include "wgrt_footprint_cache.h"
#include "wgrt_host.h"
#include "wgrt_paths.h"

using namespace wgrt;

namespace wgrt {
int footprint_aggregate_on();   // wgrt_trace.hip: wgrt_debug_set_footprint_aggregate's switch
}

namespace {

constexpr int kPathsThreads = 256;
constexpr int64_t kPathsSpan = 16 * kPathsThreads;   // records per workgroup at least: 16 rounds into each wave's cache
constexpr int64_t kPathsMaxGroups = 4096;

__global__ __launch_bounds__(kPathsThreads) void paths_footprint_kernel(const wgrt_path_vertex *paths, int64_t n,
                                                                       int64_t span, int32_t num_lmd,
                                                                       wgrt_footprint_plan fp, int64_t *map,
                                                                       int aggregate) {
    __shared__ unsigned long long cache_lds[kPathsThreads / 64][kFpSlots];
    LdsU64 *const tab = (LdsU64 *)&cache_lds[threadIdx.x >> 6][0];
    if (aggregate)   // (uniform)
        for (int k = threadIdx.x & 63; k < kFpSlots; k += 64) tab[k] = 0ull;
    const int64_t begin = (int64_t)blockIdx.x * span, end = begin + span < n ? begin + span : n;
    // (the trip count is the workgroup's: every lane of a wave makes every call of the cache)
    for (int64_t base = begin; base < end; base += kPathsThreads) {
        const int64_t k = base + threadIdx.x;
        int64_t a = -1, b = -1;
        if (k < end) {
            // the record as its two 16-byte halves
            const double2 p = ((const double2 *)(paths + k))[0];
            const ulonglong2 q = ((const ulonglong2 *)(paths + k))[1];
            path_footprint_offsets(fp, num_lmd, p.x, p.y, (uint32_t)(q.y >> 32), &a, &b);
        }
        if (aggregate) {
            fp_cached(tab, map, a);
            if (__ballot(b >= 0) != 0ull) fp_cached(tab, map, b);   // (rare: once per ray)
        } else {
            if (a >= 0) atomicAdd((unsigned long long *)map + a, 1ull);
            if (b >= 0) atomicAdd((unsigned long long *)map + b, 1ull);
        }
    }
    if (aggregate) fp_flush(tab, map);
}

}  // namespace

extern "C" {

wgrt_status wgrt_paths_footprint(const wgrt_path_vertex *paths, int64_t n, int32_t num_lmd, const wgrt_footprint_plan *fp,
                                 int64_t *map, void *stream) {
    if (const char *why = footprint_plan_error(fp)) return fail(WGRT_ERR_INVALID_ARGUMENT, why);
    if (n < 0 || num_lmd < 1 || num_lmd > kPathMaxLmd)
        return fail(WGRT_ERR_INVALID_ARGUMENT, "need n >= 0 and 1 <= num_lmd <= 256");
    if (n == 0) return WGRT_OK;
    if (!paths || !map) return fail(WGRT_ERR_INVALID_ARGUMENT, "NULL paths / map");
    if (((uintptr_t)paths & 15) || ((uintptr_t)map & 7))
        return fail(WGRT_ERR_INVALID_ARGUMENT, "the path list must be 16-B aligned (and the map 8-B)");
    const int64_t groups = std::min<int64_t>(kPathsMaxGroups, (n + kPathsSpan - 1) / kPathsSpan);
    // a span is whole rounds of the workgroup, so that spans do not overlap
    const int64_t per = (n + groups - 1) / groups, span = (per + kPathsThreads - 1) / kPathsThreads * kPathsThreads;
    hipLaunchKernelGGL(paths_footprint_kernel, dim3((unsigned)((n + span - 1) / span)), dim3(kPathsThreads), 0,
                       (hipStream_t)stream, paths, n, span, num_lmd, *fp, map, footprint_aggregate_on());
    HIP_TRY(hipGetLastError());
    return WGRT_OK;
}

}  // extern "C"
