// wgrt_eyebox.hip -- the eyebox grid's own kernels (include/wgrt.h wgrt_eyebox_*): the per-slab
// reduction (wgrt_eyebox_window_sums), the slab collection of the strong-scaling gather
// (wgrt_eyebox_pack / wgrt_eyebox_assemble) and, at the end of the file, the evaluation of the
// reduction's table (wgrt_eyebox_evaluate: colour metrics and images).
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
#include "wgrt_colour.h"
#include "wgrt_host.h"
#include "wgrt_window.h"

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

// The plan of the trace's window-table sink (wgrt_trace_windows; the sink itself is eyebox_add,
// wgrt_exact_lane.h): the mask as one bit per tap and the window grid (wgrt_window.h), copied to the device once.
extern "C" wgrt_status wgrt_window_plan_create(const float *mask, int32_t ms, int32_t step_y, int32_t step_x,
                                               int device, wgrt_window_plan **out) {
    if (!out) return fail(WGRT_ERR_INVALID_ARGUMENT, "NULL out");
    *out = nullptr;
    wgrt_window_plan *p = new wgrt_window_plan;
    if (const char *why = window_plan_view(mask, ms, step_y, step_x, p->host)) {
        delete p;
        return fail(WGRT_ERR_INVALID_ARGUMENT, why);
    }
    p->device = device;
    DeviceScope scope(device);
    hipError_t e = scope.error();
    if (e == hipSuccess) e = hipMalloc((void **)&p->d_view, sizeof(WindowPlanView));
    if (e == hipSuccess) e = hipMemcpy(p->d_view, &p->host, sizeof(WindowPlanView), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(p->d_view);
        delete p;
        return malloc_status(e, "wgrt_window_plan_create");
    }
    *out = p;
    return WGRT_OK;
}

extern "C" wgrt_status wgrt_window_plan_destroy(wgrt_window_plan *plan) {
    if (!plan) return WGRT_OK;
    DEVICE_SCOPE(dev_scope, plan->device);
    (void)hipFree(plan->d_view);
    delete plan;
    return WGRT_OK;
}

extern "C" int64_t wgrt_window_plan_width(const wgrt_window_plan *plan) { return plan ? plan->host.W : -1; }

// The fold of the replica window tables (wgrt_trace_replicas; include/wgrt.h): out[0] = the sum of the B tables
// in ascending b, out[1 + b] = out[0] - reps[b].  A stream of B x n doubles read twice (the second pass out of the
// L2) and (1 + B) x n written: one thread per V entries, V = 2 (16-B accesses) when every row starts 16-B aligned,
// else 1.  No atomics and one order of the additions, the host twin's (wgrt_eyebox_host.cpp).
namespace {

template <int V>
__global__ __launch_bounds__(256) void replicas_fold_kernel(const double *reps, int B, int64_t n, double *out) {
    const int64_t k = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
    if (k >= n) return;   // (V == 2 only with n even: k + 1 < n)
    double s[V];
    for (int v = 0; v < V; ++v) s[v] = 0.0;
    for (int b = 0; b < B; ++b) {
        double r[V];
        if (V == 2) *(double2 *)r = *(const double2 *)(reps + (int64_t)b * n + k);
        else r[0] = reps[(int64_t)b * n + k];
        for (int v = 0; v < V; ++v) s[v] += r[v];
    }
    if (V == 2) *(double2 *)(out + k) = *(const double2 *)s;
    else out[k] = s[0];
    for (int b = 0; b < B; ++b) {
        double r[V];
        if (V == 2) *(double2 *)r = *(const double2 *)(reps + (int64_t)b * n + k);
        else r[0] = reps[(int64_t)b * n + k];
        for (int v = 0; v < V; ++v) r[v] = s[v] - r[v];
        if (V == 2) *(double2 *)(out + (int64_t)(1 + b) * n + k) = *(const double2 *)r;
        else out[(int64_t)(1 + b) * n + k] = r[0];
    }
}

}  // namespace

extern "C" wgrt_status wgrt_window_replicas_fold(const double *reps, int32_t B, int64_t n, double *out, void *stream) {
    if (B < 2 || B > WGRT_MAX_REPLICAS)
        return fail(WGRT_ERR_INVALID_ARGUMENT, "need 2 <= B <= " + std::to_string(WGRT_MAX_REPLICAS));
    if (n < 0) return fail(WGRT_ERR_INVALID_ARGUMENT, "need n >= 0");
    if (n == 0) return WGRT_OK;
    if (!reps || !out) return fail(WGRT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (((uintptr_t)reps | (uintptr_t)out) & 7) return fail(WGRT_ERR_INVALID_ARGUMENT, "reps and out must be 8-B aligned");
    const bool vec = n % 2 == 0 && !(((uintptr_t)reps | (uintptr_t)out) & 15);
    const int64_t threads = vec ? n / 2 : n, blocks = (threads + 255) / 256;
    if (blocks > INT32_MAX) return fail(WGRT_ERR_INVALID_ARGUMENT, "n too large for one launch");
    int sdev = 0;
    HIP_TRY(stream_device(stream, &sdev));
    DEVICE_SCOPE(dev_scope, sdev);
    if (vec) hipLaunchKernelGGL(replicas_fold_kernel<2>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, reps, (int)B, n, out);
    else hipLaunchKernelGGL(replicas_fold_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, reps, (int)B, n, out);
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

// ---------------------------------------------------------------------------------------------
// Evaluation of the window-sum table (wgrt_eyebox_evaluate; EVAL:112-163 on the device).  The pixel math is
// wgrt_colour.h's; here are the three passes around it:
//   1. ev_pixels_kernel: a workgroup owns kEvTileFov FoVs x kEvPosChunk eye positions.  Lane k of the tile
//      takes pixel (k / pw, k % pw), so consecutive lanes read consecutive doubles of a table row (the rows
//      of a tile are contiguous but for column 0) in each of the three wavelength blocks.  The pixel's
//      delta E, Y and float32 V go to LDS, and lane p < pw then adds its position's column over the tile's
//      FoVs in FoV order: one partial record per (tile, position);
//   2. ev_fold_kernel: one workgroup of kEvFoldGroups waves.  Wave g folds its contiguous share of the tiles
//      in tile order, lane = position; wave 0 then folds the groups in group order, applies EVAL:150-163
//      per position, and its lane 0 takes the totals over the positions in position order;
//   3. ev_image_kernel / ev_image_one_kernel: the image side again from the table, normalised by the
//      position's maximum V from pass 2 (recomputing three pow per pixel is cheaper than a 15 MB HSV buffer).
// No atomics, every sum in an order fixed by (n_fov, n_pos): two runs give the same bits.
// ---------------------------------------------------------------------------------------------
namespace {

constexpr int kEvThreads = 256;
constexpr int kEvSlots = kEvTileFov * kEvPosChunk;
static_assert(kEvPosChunk == 64, "a position chunk is one wave of the column pass and of the fold");

struct EvTile {
    int64_t f0;
    int p0, nf, pw;
};

__device__ __forceinline__ EvTile ev_tile(int64_t n_fov, int64_t n_pos) {
    EvTile t;
    t.f0 = (int64_t)blockIdx.x * kEvTileFov;
    t.p0 = (int)blockIdx.y * kEvPosChunk;
    t.nf = (int)(n_fov - t.f0 < kEvTileFov ? n_fov - t.f0 : kEvTileFov);
    t.pw = (int)(n_pos - t.p0 < kEvPosChunk ? n_pos - t.p0 : kEvPosChunk);
    return t;
}

// the pixel (FoV f, position p) of the table: its three window sums -> px
__device__ __forceinline__ void ev_load_px(const double *sums, int64_t n_fov, int64_t n_pos, int64_t f, int64_t p,
                                           double divisor, const EvConsts &k, double px[3]) {
    const int64_t W = 1 + n_pos, block = n_fov * W, i = f * W + 1 + p;
    ev_px(sums[i], sums[block + i], sums[2 * block + i], divisor, k, px);
}

__global__ __launch_bounds__(kEvThreads) void ev_pixels_kernel(const double *sums, int64_t n_fov, int64_t n_pos,
                                                               double divisor, EvConsts k, EvWorkspace ws) {
    __shared__ double s_de[kEvSlots], s_y[kEvSlots];
    __shared__ float s_v[kEvSlots];
    const EvTile t = ev_tile(n_fov, n_pos);
    for (int q = threadIdx.x; q < t.nf * t.pw; q += kEvThreads) {
        const int fl = q / t.pw, pl = q - fl * t.pw;
        double px[3], Y, de;
        float h, s, v;
        ev_load_px(sums, n_fov, n_pos, t.f0 + fl, t.p0 + pl, divisor, k, px);
        ev_colour(px, k, Y, de);
        ev_hsv(px, h, s, v);
        s_de[fl * kEvPosChunk + pl] = de;
        s_y[fl * kEvPosChunk + pl] = Y;
        s_v[fl * kEvPosChunk + pl] = v;
    }
    __syncthreads();
    const int pl = threadIdx.x;
    if (pl < t.pw) {
        EvRecord r = ev_record_empty();
        for (int fl = 0; fl < t.nf; ++fl)
            ev_record_pixel(r, s_de[fl * kEvPosChunk + pl], s_y[fl * kEvPosChunk + pl], s_v[fl * kEvPosChunk + pl]);
        const int64_t at = (int64_t)blockIdx.x * n_pos + t.p0 + pl;
        ws.de_sum[at] = r.de_sum;
        ws.y_min[at] = r.y_min;
        ws.y_max[at] = r.y_max;
        ws.y_sum[at] = r.y_sum;
        ws.dark[at] = r.dark;
        ws.v_max[at] = r.v_max;
    }
}

__global__ __launch_bounds__(kEvFoldGroups * 64) void ev_fold_kernel(int64_t n_fov, int64_t n_pos, EvWorkspace ws,
                                                                     double *out) {
    __shared__ EvRecord s_rec[kEvFoldGroups][64];
    const int g = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t n_tiles = ev_tiles(n_fov);
    const int64_t per = (n_tiles + kEvFoldGroups - 1) / kEvFoldGroups;
    const int64_t lo = g * per, hi = lo + per < n_tiles ? lo + per : n_tiles;
    for (int64_t p0 = 0; p0 < n_pos; p0 += 64) {   // the same trip count in every lane
        const int64_t p = p0 + lane;
        EvRecord r = ev_record_empty();
        if (p < n_pos)
#pragma unroll 4   // 24 loads in flight; a deeper unroll spills at the 128 VGPRs of a 1024-thread workgroup
            for (int64_t tile = lo; tile < hi; ++tile) {
                const int64_t at = tile * n_pos + p;
                EvRecord o;
                o.de_sum = ws.de_sum[at];
                o.y_min = ws.y_min[at];
                o.y_max = ws.y_max[at];
                o.y_sum = ws.y_sum[at];
                o.dark = ws.dark[at];
                o.v_max = ws.v_max[at];
                ev_record_add(r, o);
            }
        s_rec[g][lane] = r;
        __syncthreads();
        if (g == 0 && p < n_pos) {
#pragma unroll 3
            for (int gg = 1; gg < kEvFoldGroups; ++gg) ev_record_add(r, s_rec[gg][lane]);
            double de_mean, ufov, ueb;
            ev_position(r, n_fov, de_mean, ufov, ueb);
            ws.pos_de[p] = de_mean;
            ws.pos_ufov[p] = ufov;
            ws.max_v[p] = r.v_max;
            out[3 + p] = ueb;
        }
        __syncthreads();
    }
    // the per-position values were written by this workgroup's wave 0, before the barrier above
    if (threadIdx.x == 0) {
        double o3[3];
        ev_totals(ws.pos_de, ws.pos_ufov, out + 3, n_pos, o3);
        out[0] = o3[0];
        out[1] = o3[1];
        out[2] = o3[2];
    }
}

// image [n_fov, 3, n_pos]: the same tiling as pass 1, a wave's stores run along the position axis
__global__ __launch_bounds__(kEvThreads) void ev_image_kernel(const double *sums, int64_t n_fov, int64_t n_pos,
                                                              double divisor, EvConsts k, const float *max_v,
                                                              float *image) {
    const EvTile t = ev_tile(n_fov, n_pos);
    for (int q = threadIdx.x; q < t.nf * t.pw; q += kEvThreads) {
        const int fl = q / t.pw, pl = q - fl * t.pw;
        const int64_t f = t.f0 + fl, p = t.p0 + pl;
        double px[3];
        float h, s, v, rgb[3];
        ev_load_px(sums, n_fov, n_pos, f, p, divisor, k, px);
        ev_hsv(px, h, s, v);
        ev_image_rgb(h, s, v, max_v[p], rgb);
        image[(f * 3 + 0) * n_pos + p] = rgb[0];
        image[(f * 3 + 1) * n_pos + p] = rgb[1];
        image[(f * 3 + 2) * n_pos + p] = rgb[2];
    }
}

// image [n_fov, 3] of the one position p: a lane per FoV
__global__ __launch_bounds__(kEvThreads) void ev_image_one_kernel(const double *sums, int64_t n_fov, int64_t n_pos,
                                                                  double divisor, EvConsts k, const float *max_v,
                                                                  int64_t p, float *image) {
    const int64_t f = (int64_t)blockIdx.x * kEvThreads + threadIdx.x;
    if (f >= n_fov) return;
    double px[3];
    float h, s, v, rgb[3];
    ev_load_px(sums, n_fov, n_pos, f, p, divisor, k, px);
    ev_hsv(px, h, s, v);
    ev_image_rgb(h, s, v, max_v[p], rgb);
    image[f * 3 + 0] = rgb[0];
    image[f * 3 + 1] = rgb[1];
    image[f * 3 + 2] = rgb[2];
}

}  // namespace

extern "C" {

int64_t wgrt_eyebox_evaluate_workspace_bytes(int64_t n_fov, int64_t n_pos) {
    return ev_shape_error(n_fov, n_pos) ? -1 : ev_workspace_bytes(n_fov, n_pos);
}

wgrt_status wgrt_eyebox_evaluate(const double *sums, int64_t n_fov, int64_t n_pos, double divisor, const double *wl,
                                 const double *lab_d65, double *out, float *image, int64_t image_pos,
                                 void *workspace, void *stream) {
    if (const char *why = ev_args_error(sums, n_fov, n_pos, divisor, wl, lab_d65, out, image, image_pos, workspace))
        return fail(WGRT_ERR_INVALID_ARGUMENT, why);
    int sdev = 0;
    HIP_TRY(stream_device(stream, &sdev));
    DEVICE_SCOPE(dev_scope, sdev);
    EvConsts k;
    for (int c = 0; c < 3; ++c) k.wl[c] = wl[c], k.lab_d65[c] = lab_d65[c];
    const EvWorkspace ws = ev_workspace(workspace, n_fov, n_pos);
    const dim3 tiles((unsigned)ev_tiles(n_fov), (unsigned)((n_pos + kEvPosChunk - 1) / kEvPosChunk));
    hipLaunchKernelGGL(ev_pixels_kernel, tiles, dim3(kEvThreads), 0, (hipStream_t)stream, sums, n_fov, n_pos, divisor,
                       k, ws);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(ev_fold_kernel, dim3(1), dim3(kEvFoldGroups * 64), 0, (hipStream_t)stream, n_fov, n_pos, ws,
                       out);
    HIP_TRY(hipGetLastError());
    if (image && image_pos < 0)
        hipLaunchKernelGGL(ev_image_kernel, tiles, dim3(kEvThreads), 0, (hipStream_t)stream, sums, n_fov, n_pos,
                           divisor, k, ws.max_v, image);
    else if (image)
        hipLaunchKernelGGL(ev_image_one_kernel, dim3((unsigned)((n_fov + kEvThreads - 1) / kEvThreads)),
                           dim3(kEvThreads), 0, (hipStream_t)stream, sums, n_fov, n_pos, divisor, k, ws.max_v,
                           image_pos, image);
    HIP_TRY(hipGetLastError());
    return WGRT_OK;
}

}  // extern "C"
