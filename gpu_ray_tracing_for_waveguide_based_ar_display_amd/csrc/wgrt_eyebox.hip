// wgrt_eyebox.hip -- the eyebox grid's own kernels (include/wgrt.h wgrt_eyebox_*): the per-slab
// reduction (wgrt_eyebox_window_sums) and, at the end of the file, the slab collection of the
// strong-scaling gather (wgrt_eyebox_pack / wgrt_eyebox_assemble).
//
// What the driver reads from an 80 x 120 slab of matrix_EB is its total (MAIN:186-192) and the sums
// over a 30-px pupil mask at every 8th / 12th bin (eye_perceive, EVAL:66-109): 1 + 7 x 8 numbers out
// of 9,600.  One 256-thread workgroup per listed slab:
//   1. the slab is read from global memory exactly once, as 16-B loads, into LDS (38.4 KB); the same
//      registers feed the slab total;
//   2. the mask goes to LDS beside it (ms * ms floats) and each mask row is reduced to one run
//      [lo, hi) of taps: the pupil is convex, so the zero taps left and right of a row are skipped (any
//      zero inside a run is multiplied through, so any mask gives the formula's result);
//   3. every window is summed from LDS.  A half-wave (32 lanes) owns a block of 8 neighbouring windows
//      of one window row: lane = (window ix, tap phase q), and a lane adds the taps lo + q, lo + q + 4,
//      ... of every mask row.  With the default step of 12 bins the 32 lanes of a half-wave read
//      32 different banks (12 ix + q mod 32 is a bijection on 8 x 4), the unit of ds_read_b32 conflicts;
//   4. the four phases of a window are added as (q0 + q1) + (q2 + q3) by two lane exchanges.
// Every sum is float64 in an order fixed by the launch shape alone (no atomics): the same input gives
// the same bits on every run, and an integer-valued grid (counts, every partial sum < 2^53) gives the
// exact integers whatever the order.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/wgrt.h"
#include "wgrt_host.h"

using namespace wgrt;

namespace {

constexpr int kEbRows = 80, kEbCols = 120;
constexpr int kSlabF4 = WGRT_EB_SLAB / 4;   // 2400 float4 per slab
constexpr int kThreads = 256;
constexpr int kLoads = (kSlabF4 + kThreads - 1) / kThreads;   // float4 loads per thread (10, the last partial)
constexpr int kPhases = 4;                  // tap phases per window
constexpr int kBlockWin = 32 / kPhases;     // windows per half-wave block
constexpr int kHalfWaves = kThreads / 32;
constexpr int kTaps = 8;                    // LDS reads a lane keeps in flight (one mask row of the default pupil)
constexpr int kLdsPad = kPhases * kTaps;    // floats behind the slab and behind the mask (window_phase_sum)

static_assert(WGRT_EB_SLAB == kEbRows * kEbCols, "slab shape");

// sum over the 64 lanes of a wave, the same tree (and so the same bits) in every lane
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

// One lane's share of a window: taps lo + q, lo + q + kPhases, ... of every mask row, kTaps reads in flight.
// A read past the run's end (at most kPhases * kTaps - 1 floats past it: the kLdsPad floats behind the slab
// and behind the mask keep it inside the allocation) is replaced by 0 before it is used.
template <bool kUnit>
__device__ __forceinline__ double window_phase_sum(const float *win, const float *mask, const int *lo, const int *hi,
                                                   int ms, int q) {
    double a0 = 0.0, a1 = 0.0;
    for (int r = 0; r < ms; ++r) {
        const float *row = win + r * kEbCols + q;
        const float *mrow = mask + r * ms + q;
        const int h = hi[r] - q;
        for (int b = lo[r]; b < h + q; b += kPhases * kTaps) {   // the same trip count in every lane
            float x[kTaps], w[kTaps];
#pragma unroll
            for (int k = 0; k < kTaps; ++k) {
                x[k] = row[b + kPhases * k];
                w[k] = kUnit ? 1.0f : mrow[b + kPhases * k];
            }
#pragma unroll
            for (int k = 0; k < kTaps; ++k) {
                const bool in = b + kPhases * k < h;
                const double xv = (double)(in ? x[k] : 0.0f);
                const double tap = kUnit ? xv : (double)(in ? w[k] : 0.0f) * xv;
                if (k & 1) a1 += tap;
                else a0 += tap;
            }
        }
    }
    return a0 + a1;
}

// dynamic LDS: the slab (9600 floats), kLdsPad floats, the mask (ms * ms floats), kLdsPad floats
__global__ __launch_bounds__(kThreads) void eyebox_window_sums_kernel(const float *eb, int64_t n_slabs,
                                                                      const int64_t *slabs, const float *mask, int ms,
                                                                      int step_y, int step_x, int npy, int npx,
                                                                      double *out) {
    extern __shared__ float4 lds4[];
    __shared__ int s_lo[kEbRows], s_hi[kEbRows];
    __shared__ double s_part[kThreads / 64];
    float *slab = (float *)lds4;
    float *lmask = slab + WGRT_EB_SLAB + kLdsPad;
    const int t = threadIdx.x;
    const int64_t j = blockIdx.x;
    const int W = 1 + npy * npx;
    double *orow = out + j * W;
    const int64_t s = slabs ? slabs[j] : j;
    if (s < 0 || s >= n_slabs) {   // uniform over the workgroup
        for (int k = t; k < W; k += kThreads) orow[k] = 0.0;
        return;
    }
    for (int k = t; k < ms * ms; k += kThreads) lmask[k] = mask[k];
    // 1. the slab: HBM -> registers (all loads in flight) -> LDS, and its total
    const float4 *src = (const float4 *)(eb + s * WGRT_EB_SLAB);
    float4 v[kLoads];
#pragma unroll
    for (int k = 0; k < kLoads; ++k) {
        const int c = t + k * kThreads;
        v[k] = (k < kLoads - 1 || c < kSlabF4) ? src[c] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    double tot = 0.0;
#pragma unroll
    for (int k = 0; k < kLoads; ++k) {
        const int c = t + k * kThreads;
        if (k < kLoads - 1 || c < kSlabF4) lds4[c] = v[k];
        tot += ((double)v[k].x + (double)v[k].y) + ((double)v[k].z + (double)v[k].w);
    }
    tot = wave_sum(tot);
    if ((t & 63) == 0) s_part[t >> 6] = tot;
    __syncthreads();
    // 2. the run of each mask row, and whether every tap inside the runs is 1 (then no multiply)
    int unit_row = 1;
    if (t < ms) {
        int lo = 0, hi = 0, nz = 0, ones = 0;
        for (int c = 0; c < ms; ++c) {
            const float m = lmask[t * ms + c];
            if (m != 0.0f) {
                if (!nz) lo = c;
                hi = c + 1;
                ++nz;
                ones += m == 1.0f;
            }
        }
        s_lo[t] = lo;
        s_hi[t] = hi;
        unit_row = nz == hi - lo && ones == nz;
    }
    const int unit = __syncthreads_and(unit_row);
    if (t == 0) orow[0] = (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
    // 3. the windows, a block of kBlockWin per half-wave
    const int q = t & (kPhases - 1), ixl = (t >> 2) & (kBlockWin - 1), half = t >> 5;
    const int nxb = (npx + kBlockWin - 1) / kBlockWin, nblk = npy * nxb;
    for (int b0 = 0; b0 < nblk; b0 += kHalfWaves) {   // the same trip count in every lane: the exchanges below
        const int blk = b0 + half;                    // are never executed by a part of a wave
        const int bc = blk < nblk ? blk : nblk - 1;
        const int iy = bc / nxb, ix = (bc % nxb) * kBlockWin + ixl;
        const int ixc = ix < npx ? ix : npx - 1;      // lanes past the last window repeat it and write nothing
        const float *win = slab + iy * step_y * kEbCols + ixc * step_x;
        double acc = unit ? window_phase_sum<true>(win, lmask, s_lo, s_hi, ms, q)
                          : window_phase_sum<false>(win, lmask, s_lo, s_hi, ms, q);
        acc += __shfl_xor(acc, 1);
        acc += __shfl_xor(acc, 2);
        if (q == 0 && blk < nblk && ix < npx) orow[1 + iy * npx + ix] = acc;
    }
}

}  // namespace

extern "C" wgrt_status wgrt_eyebox_window_sums(const float *eb, int64_t n_slabs, const int64_t *slabs, int64_t n,
                                               const float *mask, int32_t ms, int32_t step_y, int32_t step_x,
                                               double *out, void *stream) {
    if (n < 0 || n_slabs < 0) return fail(WGRT_ERR_INVALID_ARGUMENT, "need n >= 0 and n_slabs >= 0");
    if (ms < 1 || ms > kEbRows) return fail(WGRT_ERR_INVALID_ARGUMENT, "need 1 <= ms <= 80");
    if (step_y < 1 || step_x < 1) return fail(WGRT_ERR_INVALID_ARGUMENT, "need step_y >= 1 and step_x >= 1");
    if (n == 0) return WGRT_OK;
    if (!mask || !out || (!eb && n_slabs > 0)) return fail(WGRT_ERR_INVALID_ARGUMENT, "NULL argument");
    if ((uintptr_t)eb & 15) return fail(WGRT_ERR_INVALID_ARGUMENT, "eb must be 16-B aligned");
    if ((uintptr_t)out & 7) return fail(WGRT_ERR_INVALID_ARGUMENT, "out must be 8-B aligned");
    if (n > INT32_MAX) return fail(WGRT_ERR_INVALID_ARGUMENT, "at most 2^31 - 1 rows per call");
    const int npy = (kEbRows - ms) / step_y + 1, npx = (kEbCols - ms) / step_x + 1;
    int sdev = 0;
    HIP_TRY(stream_device(stream, &sdev));
    DEVICE_SCOPE(dev_scope, sdev);
    // 38.4 KB + the mask: 42 KB at ms = 30 (three workgroups per CU), 64 KB at ms = 80 (two)
    const size_t lds = (size_t)(WGRT_EB_SLAB + ms * ms + 2 * kLdsPad) * sizeof(float);
    hipLaunchKernelGGL(eyebox_window_sums_kernel, dim3((unsigned)n), dim3(kThreads), lds, (hipStream_t)stream, eb,
                       n_slabs, slabs, mask, (int)ms, (int)step_y, (int)step_x, npy, npx, out);
    HIP_TRY(hipGetLastError());
    return WGRT_OK;
}

// ---------------------------------------------------------------------------------------------
// Eyebox collection of the strong-scaling gather (wgrt_eyebox_pack / wgrt_eyebox_assemble): row copies
// of whole 80 x 120 slabs as 16-B loads / stores, one workgroup per (row, 1/kSlabParts of the slab).
// The spill rows (121 floats) move as dwords.
// ---------------------------------------------------------------------------------------------
namespace {

constexpr int kSlabParts = 3;   // 800 float4 per workgroup: 256 threads x 3-4

inline int64_t eb_spill_floats(int64_t nb) { return (nb * WGRT_EB_SPILL + 3) / 4 * 4; }

__global__ __launch_bounds__(256) void eyebox_pack_kernel(const float *eb, int64_t n_slabs, const int64_t *slabs,
                                                          const int64_t *next, const float *mask, int64_t n, int64_t nb,
                                                          float *payload) {
    const int64_t j = blockIdx.y;
    if (j >= n) return;
    const int64_t s = slabs[j];
    if (s < 0 || s >= n_slabs) return;
    const float4 *src = (const float4 *)(eb + s * WGRT_EB_SLAB);
    float4 *out = (float4 *)(payload + j * WGRT_EB_SLAB);
    const int lo = (int)blockIdx.x * (kSlabF4 / kSlabParts), hi = lo + kSlabF4 / kSlabParts;
    for (int c = lo + threadIdx.x; c < hi; c += blockDim.x) out[c] = src[c];
    if (blockIdx.x == 0 && threadIdx.x < WGRT_EB_SPILL) {
        const int64_t t = next[j];
        const float v = (t >= 0 && t < n_slabs) ? eb[t * WGRT_EB_SLAB + threadIdx.x] * mask[j] : 0.0f;
        payload[nb * WGRT_EB_SLAB + j * WGRT_EB_SPILL + threadIdx.x] = v;
    }
}

__global__ __launch_bounds__(256) void eyebox_copy_kernel(float *eb, int64_t n_slabs, const float *recv, int64_t nb,
                                                          int64_t plen, const int64_t *dst) {
    const int64_t row = blockIdx.y;   // r * nb + j
    const int64_t s = dst[row];
    if (s < 0 || s >= n_slabs) return;
    const int64_t r = row / nb, j = row % nb;
    const float4 *src = (const float4 *)(recv + r * plen + j * WGRT_EB_SLAB);
    float4 *out = (float4 *)(eb + s * WGRT_EB_SLAB);
    const int lo = (int)blockIdx.x * (kSlabF4 / kSlabParts), hi = lo + kSlabF4 / kSlabParts;
    for (int c = lo + threadIdx.x; c < hi; c += blockDim.x) out[c] = src[c];
}

__global__ __launch_bounds__(128) void eyebox_spill_kernel(float *eb, int64_t n_slabs, const float *recv, int64_t nb,
                                                           int64_t plen, const int64_t *spill_dst) {
    const int64_t row = blockIdx.x;
    const int64_t s = spill_dst[row];
    if (s < 0 || s >= n_slabs || threadIdx.x >= WGRT_EB_SPILL) return;
    const int64_t r = row / nb, j = row % nb;
    // one spill row per target slab (slab s's spill comes only from slab s - 1): no atomics needed
    eb[s * WGRT_EB_SLAB + threadIdx.x] += recv[r * plen + nb * WGRT_EB_SLAB + j * WGRT_EB_SPILL + threadIdx.x];
}

}  // namespace

extern "C" {

int64_t wgrt_eyebox_payload_floats(int64_t nb) { return nb < 0 ? -1 : nb * WGRT_EB_SLAB + eb_spill_floats(nb); }

wgrt_status wgrt_eyebox_pack(const float *eb, int64_t n_slabs, const int64_t *slabs, const int64_t *next,
                             const float *spill_mask, int64_t n, int64_t nb, float *payload, void *stream) {
    if (n < 0 || nb < n || n_slabs < 0) return fail(WGRT_ERR_INVALID_ARGUMENT, "need 0 <= n <= nb and n_slabs >= 0");
    if (n == 0) return WGRT_OK;
    if (!eb || !slabs || !next || !spill_mask || !payload) return fail(WGRT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (((uintptr_t)eb | (uintptr_t)payload) & 15) return fail(WGRT_ERR_INVALID_ARGUMENT, "eb / payload must be 16-B aligned");
    if (n > 65535) return fail(WGRT_ERR_INVALID_ARGUMENT, "at most 65535 slabs per rank");
    int sdev = 0;
    HIP_TRY(stream_device(stream, &sdev));
    DEVICE_SCOPE(dev_scope, sdev);
    hipLaunchKernelGGL(eyebox_pack_kernel, dim3(kSlabParts, (unsigned)n), dim3(256), 0, (hipStream_t)stream, eb,
                       n_slabs, slabs, next, spill_mask, n, nb, payload);
    HIP_TRY(hipGetLastError());
    return WGRT_OK;
}

wgrt_status wgrt_eyebox_assemble(float *eb, int64_t n_slabs, const float *recv, int32_t world, int64_t nb,
                                 const int64_t *dst, const int64_t *spill_dst, void *stream) {
    if (world < 0 || nb < 0 || n_slabs < 0) return fail(WGRT_ERR_INVALID_ARGUMENT, "negative world / nb / n_slabs");
    const int64_t rows = (int64_t)world * nb;
    if (rows == 0) return WGRT_OK;
    if (!eb || !recv || !dst || !spill_dst) return fail(WGRT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (((uintptr_t)eb | (uintptr_t)recv) & 15) return fail(WGRT_ERR_INVALID_ARGUMENT, "eb / recv must be 16-B aligned");
    if (rows > 65535) return fail(WGRT_ERR_INVALID_ARGUMENT, "at most 65535 payload rows");
    int sdev = 0;
    HIP_TRY(stream_device(stream, &sdev));
    DEVICE_SCOPE(dev_scope, sdev);
    const int64_t plen = wgrt_eyebox_payload_floats(nb);
    hipLaunchKernelGGL(eyebox_copy_kernel, dim3(kSlabParts, (unsigned)rows), dim3(256), 0, (hipStream_t)stream, eb,
                       n_slabs, recv, nb, plen, dst);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(eyebox_spill_kernel, dim3((unsigned)rows), dim3(128), 0, (hipStream_t)stream, eb, n_slabs, recv,
                       nb, plen, spill_dst);
    HIP_TRY(hipGetLastError());
    return WGRT_OK;
}

}  // extern "C"
