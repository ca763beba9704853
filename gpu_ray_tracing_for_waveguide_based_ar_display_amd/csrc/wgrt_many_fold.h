// wgrt_many_fold.h -- the interleaved chunk scratch of the K-at-once re-weightings and the kernel that folds it into
// the chunk's tables, stated once for wgrt_visits_reweight_many (wgrt_visits.hip) and wgrt_hits_reweight_sources
// (wgrt_sources.hip).  Device code only: each translation unit that includes it gets its own copy of the kernel.
//
// A chunk is kManyDesigns = 64 tables, one per lane.  A wave's 64 deposits for one table entry e go to
// scratch[e * 64 + lane], 512 contiguous bytes, where 64 adds into 64 tables would touch 64 cache lines; the fold then
// adds scratch[e][j] into table j of the chunk and leaves the scratch zero for the next chunk.  The deposits are on the
// 2^-32 grid (wgrt_expected.h), so the detour changes no bit of the tables.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace wgrt {

constexpr int kManyThreads = 256;                // threads of a re-weighting or fold workgroup
constexpr int kManyDesigns = 64;                 // tables per chunk: one per lane
constexpr int kManyStride = kManyDesigns + 1;    // LDS doubles per row of a 64-wide tile
constexpr int kManyRows = 64;                    // rows (records) per workgroup

// out[j][e] += scratch[e][j] for the chunk's nk tables, 64 entries per workgroup through an LDS tile (reads along j,
// writes along e, both contiguous), and scratch is left zero.  Plain adds: a call's kernels are ordered on its stream
// and nothing else writes the tables meanwhile.  Reads and writes of scratch are at entries below n_entries (times 64
// lanes); writes of out at j * table_stride + e with j < nk and e < n_entries.
static __global__ __launch_bounds__(kManyThreads) void visits_many_fold_kernel(double *scratch, int64_t n_entries, int nk,
                                                                              double *out, int64_t table_stride) {
    __shared__ double tile[kManyDesigns][kManyStride];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t e0 = (int64_t)blockIdx.x * 64;
    for (int i = wave; i < 64; i += kManyThreads / 64) {
        double v = 0.0;
        if (e0 + i < n_entries) {
            double *const p = scratch + (e0 + i) * kManyDesigns + lane;
            v = *p;
            if (v != 0.0) *p = 0.0;
        }
        tile[i][lane] = v;
    }
    __syncthreads();
    if (e0 + lane >= n_entries) return;
    for (int j = wave; j < nk; j += kManyThreads / 64) {
        const double v = tile[lane][j];
        if (v != 0.0) out[j * table_stride + e0 + lane] += v;
    }
}

}  // namespace wgrt
