// wgrt_fate.hip -- the fate census (wgrt_fate_census, include/wgrt.h): the per-ray fate codes a trace left
// (wgrt_trace_fate; wgrt_fate.h) counted into the per-tile table [n_slabs, WGRT_FATE_COLS].
//
// A batch lies contiguous per tile (wgrt_rays_init), and more than half of all rays share one code (92, the
// in-coupler's first diffraction), so one global atomic per ray would serialise on one address per tile.  A
// workgroup therefore takes a contiguous span of kCensusSpan rays and counts them, 256 consecutive rays at a time,
// in an LDS histogram of one table row: the row of the tile the current 256-ray block starts in, flushed with at
// most kFateCols global atomics when a block starts in another tile and at the end; only rays of a tile other than
// their block's first go to global memory directly.  That is correct for any ray order (the counts are integer
// atomics: the table is the same on every run) and nearly atomic-free for the product's layout at any tile size.
// (With the whole span counted against its first tile alone, C3's 1,024-ray tiles sent three rays in four down the
// global path: 0.089 ms for 1.35 M rays.)
//
// The span's fate bytes are staged in LDS with one 16-B load per lane where the buffer is 16-B aligned (byte loads
// otherwise, and in the batch's last span), then counted ray j of the span by thread j % 256, so the three tile
// index columns are read coalesced.  Every global read is at a ray index below n_rays; every write is to
// table[slab, col] with slab checked against the scene and col < kFateCols for every valid code.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/wgrt.h"
#include "wgrt_fate.h"
#include "wgrt_host.h"

using namespace wgrt;

static_assert(WGRT_FATE_COLS == kFateCols, "include/wgrt.h and wgrt_fate.h state the same row width");

namespace {

constexpr int kCensusThreads = 256;
constexpr int kCensusPerLane = 16;                               // fate bytes per lane: one 16-B load
constexpr int kCensusSpan = kCensusThreads * kCensusPerLane;     // rays per workgroup

__global__ __launch_bounds__(kCensusThreads) void fate_census_kernel(const uint8_t *fate, const float *m, const float *n,
                                                                     const float *l, int64_t n_rays, int nx, int ny,
                                                                     int nl, unsigned long long *table) {
    __shared__ uint32_t hist[kFateCols];
    __shared__ __attribute__((aligned(16))) uint8_t bytes[kCensusSpan];
    const int t = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * kCensusSpan;   // < n_rays: the grid is ceil(n_rays / span)
    const int64_t left = n_rays - base;
    const int cnt = left < kCensusSpan ? (int)left : kCensusSpan;
    if (t < kFateCols) hist[t] = 0u;
    // the tile index columns of this thread's rays, all in flight at once (an index past the span reads the span's
    // first ray and is never used): issued before the bytes are staged, so one memory round trip covers both
    float fm[kCensusPerLane], fn[kCensusPerLane], fl[kCensusPerLane];
#pragma unroll
    for (int k = 0; k < kCensusPerLane; ++k) {
        const int j = k * kCensusThreads + t;
        const int64_t i = base + (j < cnt ? j : 0);
        fm[k] = m[i];
        fn[k] = n[i];
        fl[k] = l ? l[i] : 0.0f;
    }
    const int o = t * kCensusPerLane;
    if (o + kCensusPerLane <= cnt && (((uintptr_t)(fate + base)) & 15u) == 0u) {
        *(uint4 *)(bytes + o) = *(const uint4 *)(fate + base + o);
    } else {
        for (int k = 0; k < kCensusPerLane; ++k)
            if (o + k < cnt) bytes[o + k] = fate[base + o + k];
    }
    // Ray j of the span is counted by thread j % 256, 256 consecutive rays at a time, so the tile index columns are
    // read coalesced.  The histogram holds the counts of ONE tile, that of the current 256-ray block's first ray: when
    // a block starts in another tile, the histogram is flushed (at most 56 atomics) and taken over by the new tile
    // (every branch on cur / first is workgroup-uniform).  A ray of any other tile goes to global memory directly.
    __shared__ long long blk_tile;
    long long cur = -1;   // the histogram's tile (-1: none; then nothing counts in LDS)
#pragma unroll
    for (int k = 0; k < kCensusPerLane; ++k) {
        if (k * kCensusThreads >= cnt) break;
        const int j = k * kCensusThreads + t;
        const long long tile = fate_slab(fm[k], fn[k], fl[k], l != nullptr, nx, ny, nl);
        if (t == 0) blk_tile = tile;   // (thread 0's ray exists: k * 256 < cnt)
        __syncthreads();               // ... and, the first time, the staged bytes and the zeroed histogram
        const long long first = blk_tile;
        if (first != cur) {
            if (t < kFateCols) {
                if (cur >= 0 && hist[t] != 0u) atomicAdd(table + cur * kFateCols + t, (unsigned long long)hist[t]);
                hist[t] = 0u;
            }
            cur = first;
            __syncthreads();
        }
        const int code = j < cnt ? bytes[j] : 0;
        if (fate_valid(code) && tile >= 0) {
            const int col = fate_col(code);
            if (tile == cur) atomicAdd(&hist[col], 1u);
            else atomicAdd(table + tile * kFateCols + col, 1ull);
        }
        __syncthreads();   // this block's counts are in before the next block may flush them
    }
    if (t < kFateCols && cur >= 0 && hist[t] != 0u) atomicAdd(table + cur * kFateCols + t, (unsigned long long)hist[t]);
}

}  // namespace

extern "C" {

wgrt_status wgrt_fate_census(const uint8_t *fate, const float *m, const float *n, const float *lmd_num, int64_t n_rays,
                             int32_t nx, int32_t ny, int32_t num_lmd, int64_t *table, void *stream) {
    if (const char *why = fate_census_args_error(fate, m, n, n_rays, nx, ny, num_lmd, table))
        return fail(WGRT_ERR_INVALID_ARGUMENT, why);
    if (n_rays == 0) return WGRT_OK;
    const int64_t blocks = (n_rays + kCensusSpan - 1) / kCensusSpan;
    if (blocks > 0x7fffffff) return fail(WGRT_ERR_INVALID_ARGUMENT, "too many rays for one census");
    int sdev = 0;
    HIP_TRY(stream_device(stream, &sdev));
    DEVICE_SCOPE(dev_scope, sdev);
    hipLaunchKernelGGL(fate_census_kernel, dim3((unsigned)blocks), dim3(kCensusThreads), 0, (hipStream_t)stream, fate, m, n,
                       lmd_num, n_rays, (int)nx, (int)ny, (int)num_lmd, (unsigned long long *)table);
    HIP_TRY(hipGetLastError());
    return WGRT_OK;
}

}  // extern "C"
