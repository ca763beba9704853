// wgrt_args.h -- what every kernel of a launch is handed: the device-side scene view (LocatorT), the
// launch arguments (TraceArgs) and the handle that re-reads them from the kernarg segment (KArgs), the
// codes and the counter record (Counters) shared by both lanes of the per-ray state machine.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/wgrt.h"
#include "wgrt_common.h"
#include "wgrt_scene_build.h"

namespace wgrt {

struct WindowPlanView;   // wgrt_window.h

// s_waitcnt vmcnt(0) with expcnt / lgkmcnt left at their maxima, in the gfx9 simm16 encoding (vmcnt bits
// 3:0 and 15:14, expcnt 6:4 = 7, lgkmcnt 11:8 = 15): through __builtin_amdgcn_s_waitcnt, so the compiler's
// wait insertion knows that every vector-memory access issued before it has completed
constexpr int kWaitVmcnt0 = 0x0F70;

// ----------------------------------------------------------------------------
// device-side scene view
// ----------------------------------------------------------------------------
// The exact polygon locator (wgrt_scene_build.cpp).  CellT = uint64_t cell words (up to 32
// polygons), uint32_t (up to 16 polygons: half the grid's cache footprint).
template <class CellT>
struct LocatorT {
    using Word = CellT;
    using Cell = CellT;   // what the grid holds and a lane prefetches (JLane::pf)
    static constexpr bool kByte = false;
    const CellT *cells;
    const double *verts;
    const int32_t *poly_off;
    const int32_t *row_off;
    const int32_t *row_edges;
    double x0, y0, inv_h;
    int ncx, ncy;
    const double *bands;    // 128-B band records (LocatorHost::bands); NULL: CSR lists only
};
using Locator = LocatorT<uint64_t>;

// The byte form of the locator (the Jones-vector lane only; wgrt_scene_build.h build_palette_host): the grid
// holds each cell's index into the palette of the scene's distinct cell words (88 on the design geometry), a
// quarter of the 32-bit grid's cache footprint at the same cell size and the same index arithmetic.  A lane
// prefetches the byte (JLane::pb) and decodes the word from the workgroup's LDS copy of the palette where it
// is consumed; everything downstream sees the word a LocatorT<CellT> would have loaded.  The fields the exact
// test reads keep LocatorT's names.
template <class CellT>
struct ByteLocatorT {
    using Word = CellT;
    using Cell = uint8_t;
    static constexpr bool kByte = true;
    const uint8_t *cells;
    const double *verts;
    const int32_t *poly_off;
    const int32_t *row_off;
    const int32_t *row_edges;
    double x0, y0, inv_h;
    int ncx, ncy;
    const double *bands;
    const CellT *palette;   // kPaletteMax words, ascending, zero past the scene's count
};

struct TraceArgs {
    const float *x, *y, *m, *n, *l, *te, *tm, *dph;
    uint32_t *rng;
    float *eb;
    wgrt_trace_stats *stats;
    uint32_t *per_ray;
    int64_t n_rays, gid_offset;
    const double *tiles;
    Locator loc;
    int tile_d, nfc, noc, nx, ny, nl;
    double n_g, inv_n_g;
    double threshold;   // ener * efficiency > threshold guard of R2..R5: 0 full colour, 1e-15 single lambda
    const int32_t *order;   // Jones-vector variants: issue order of the 64-ray chunks (NULL: ascending)
    const double *jtiles;   // Jones-vector tiles (wgrt_common.h kJ*)
    int jtile_d;
    // Jones-vector variants: out-couplings appended as (position, tile index) and binned into
    // matrix_EB by the epilogue kernel after the launch
    double2 *q_xy;
    uint32_t *q_i;
    unsigned long long *q_count;
    double cert_tol;   // Jones-vector variants: base of the double-precision certification bound
    double cert_tol32; // ... and of the single-precision estimate's bound
    unsigned long long *replay_count;   // Jones-vector variants: abandoned rays (local indices)
    uint32_t *replay_list;
    // Jones-vector variants: per-workgroup counter partials (a Counters record in a kPartWords slot) of
    // the trace kernel, summed into *stats by the epilogue -- no contended atomics on the stats
    unsigned long long *part;
    int n_trace_waves;                  // partial slots of the trace kernel (one per workgroup)
    unsigned long long *heads0;         // this launch's counter set (kScratchCtr words)
    unsigned long long *other_ctr;      // the next launch's counter set, zeroed by this launch's epilogue
    uint32_t *full_list;                // out-coupling queue blocks the trace waves filled (block numbers); with the
                                        // in-kernel epilogue: per block, the link to the block its wave filled before
    unsigned long long *full_count;
    unsigned long long *epi_acc;        // in-kernel epilogue: the launch's totals (a Counters record) ...
    unsigned long long *epi_done;       // ... and the count of trace workgroups that have added theirs
    unsigned long long *timeline;       // debug: per-wave timeline (wgrt_debug_opts), timeline kernels only
    int64_t timeline_waves;
    // fused launches (variants 7 / 9, n_iter > 1): n_iter chained traces of every ray in one
    // launch; rng64[i] = (state << 32) | iter_tag(iter_epoch, traces completed, broken)
    int n_iter;
    uint64_t *rng64;
    uint32_t iter_epoch;
    unsigned long long handoff_wait_ticks;   // fused: s_memrealtime ticks a lane may wait for a hand-off ...
    uint32_t handoff_min_passes;             // ... once its wave has also run this many passes waiting
    // global ray ids of an interleaved shard (wgrt_launch_opts.gid_blocks): NULL = gid_offset + i
    const int64_t *gid_blocks;
    int64_t gid_block_rays;
    // the window-table sink (wgrt_trace_windows; wgrt_window.h): with win_table, every out-coupling also
    // counts into table [n_slabs, W] under the plan *win; eb may then be NULL.  Last, so that every other
    // field keeps its place in the kernarg segment.
    double *win_table;
    const WindowPlanView *win;
    // per-ray fate codes (wgrt_trace_fate; wgrt_fate.h): with fate, the lane that ends ray i's trace stores its
    // code in fate[i] (0 for a ray that is not traced).  NULL: nothing is stored.  Single launches only; the
    // Jones-vector lane stores it in its FATE instantiations.  Last again, for the same reason.
    uint8_t *fate;
    // replica window tables (wgrt_trace_replicas): with win_reps >= 2, win_table is [win_reps, n_slabs, W] and an
    // out-coupling of the ray with global id g counts into copy g % win_reps, win_rep_stride = n_slabs * W entries
    // apart.  0: one table.  The exact lane reads them where it bins (eyebox_bin); the Jones-vector lane carries
    // the replica in its out-coupling queue entry (the REPS instantiations).  Single launches only.  Last again.
    int64_t win_rep_stride;
    int32_t win_reps;
    // fused launches: the run length, the consecutive traces of a ray one work item covers and one lane keeps the
    // ray for (wgrt_items.h; a power of two, 1: an item per trace), and the first tail length of the launch's taper
    // (a power of two below the run, 0: none) -- together the launch's run partition.  Both in the word that padded
    // the struct, so every other field and the kernel parameters behind it keep their places in the kernarg segment.
    int16_t fused_run;
    int16_t fused_t0;
    // footprint maps (wgrt_trace_footprint; wgrt_footprint.h): with fp_map, every counted draw of the bounce loop adds
    // to the int64 map [nl, 9, fp.ny_cells, fp.nx_cells] under the plan fp (by value).  fp_seen: one word per
    // replay-list entry of the launch scratch, the draws the Jones-vector lane had counted when it abandoned the
    // ray, which the replay passes over.  fp_aggregate: the sink sums a wave's adds to one entry on chip (0: one atomic
    // per lane; wgrt_debug_set_footprint_aggregate).  Single launches only, in the FP instantiations.  Last again.
    int64_t *fp_map;
    uint32_t *fp_seen;
    wgrt_footprint_plan fp;
    int32_t fp_aggregate;
    int32_t fp_pad_;
    // the hit list (wgrt_trace_hits; wgrt_hits.h): with hits, every out-coupling of the launch reserves an index with a
    // returning add on *hits_count and, where the index is below hits_cap, stores its record at hits[index], tagged
    // hits_tag.  Only the HITS instantiations read them: the exact lane appends at interact's out-coupling
    // (trace_grid_hits_kernel, the kHits replay), the Jones-vector lane where it bins its queue, and its push also
    // stores the entry's local ray index in q_ray (beside q_i; allocated by a hits launch's scratch growth only).
    // Single launches only.  Last again.
    wgrt_hit *hits;
    int64_t hits_cap;
    unsigned long long *hits_count;
    uint32_t *q_ray;
    uint32_t hits_tag;
    uint32_t hits_pad_;
    // the path list (wgrt_trace_paths; wgrt_paths.h): with paths, every draw of the bounce loop of a selected ray, and
    // the end of a trace that leaves eff_reg1 or misses in R5, is a record of the list: an index is reserved on
    // *paths_count and, where it is below paths_cap, the record is stored at paths[index], tagged paths_tag.  select:
    // one byte per ray of the batch, nonzero: record the ray (NULL: every ray).  Only the PATHS instantiations read
    // them: the exact lane appends one record at a time (trace_grid_paths_kernel, the kPaths replay), the Jones-vector
    // lane stages a wave's records in LDS and reserves a block's indices at once; the draws it had recorded of a ray it
    // abandons go to the replay in fp_seen's storage.  Single launches only.  Last again.
    wgrt_path_vertex *paths;
    int64_t paths_cap;
    unsigned long long *paths_count;
    const uint8_t *select;
    uint32_t paths_tag;
    uint32_t paths_pad_;
    // branch visit counts (wgrt_trace_visits; wgrt_visits.h): with vis_counts, ray i is counted into row
    // vis_slot ? vis_slot[i] : i (negative: not counted): every draw that takes a branch, the in-coupling event's
    // included, adds 1 to vis_counts[row * vis_channels + channel], and a last draw that out-couples writes
    // vis_ends[row].  Only the VISITS instantiations read them: both lanes add with one unsigned atomic whose result is
    // not used (trace_grid_visits_kernel, the kVisits replay; the Jones-vector lane once the draw is certified); the
    // draws the Jones-vector lane had counted of a ray it abandons go to the replay in fp_seen's storage.  Single
    // launches only.  Last again.
    const int32_t *vis_slot;
    uint32_t *vis_counts;
    wgrt_visit_end *vis_ends;
    int32_t vis_channels;
    int32_t vis_pad_;
    // Stokes window tables (wgrt_trace_stokes; wgrt_stokes.h): with stokes, an out-coupling that the window table counts
    // also adds its three quanta q_k to the same entries of table k of the int64 [3, n_slabs, W] tables, stokes_stride
    // = n_slabs * W entries apart.  Only the STOKES instantiations read them: the exact lane deposits at interact's
    // out-coupling (trace_grid_stokes_kernel, the kStokes replay); the Jones-vector lane computes the quanta where
    // interact returns kOut, pushes them with the queue entry into q_stokes (beside q_i; allocated by a Stokes launch's
    // scratch growth only) and deposits where it bins its queue.  Single launches only.  Last again.
    int64_t *stokes;
    int64_t stokes_stride;
    int4 *q_stokes;
};

// The replica of global ray id g >= 0 among reps (2 .. 64) copies: g % reps from 32-bit remainders (the 64-bit
// one is a long routine; this runs where a ray out-couples).
__device__ __forceinline__ uint32_t replica_of(int64_t g, uint32_t reps) {
    const uint32_t hi = (uint32_t)((uint64_t)g >> 32) % reps, lo = (uint32_t)g % reps;
    const uint32_t two32 = (0xffffffffu % reps + 1u) % reps;   // 2^32 % reps
    return (hi * two32 + lo) % reps;                           // (< 64 * 64 + 64)
}
constexpr int kRepShift = 24;   // a REPS queue entry: tile index | replica << kRepShift (scenes below 2^24 tiles)

// TraceArgs fields re-read from the kernarg segment where they are used (a volatile scalar load,
// a scalar-cache hit) instead of being held in SGPRs for the whole kernel: the Jones loop keeps
// only its per-pass operands in SGPRs; the ray columns and the rare-path pointers (refill,
// retire, replay, out-coupling) are fetched when those run.
//
// KArgs is the handle those reads go through: the base of the kernarg segment as the KERNEL BODY
// saw it.  Only kernel_kargs<Kernel>() makes one, and it refuses to compile unless Kernel's first
// parameter is a TraceArgs (which then lies at offset 0 of the segment).  A function that reads a
// field takes the handle as a parameter, so it reads the right segment whether or not the
// compiler inlines it; __builtin_amdgcn_kernarg_segment_ptr() evaluated inside a called function
// instead reads whatever the caller's registers hold (round 4's out-of-line EDGE build faulted
// with hipErrorIllegalAddress that way).
typedef const char __attribute__((address_space(4))) KSeg;

template <class F>
struct first_param;
template <class A0, class... R>
struct first_param<void(A0, R...)> {
    using type = A0;
};
template <class X, class Y>
struct same_type {
    static constexpr bool value = false;
};
template <class X>
struct same_type<X, X> {
    static constexpr bool value = true;
};

class KArgs {
    KSeg *base_;
    __device__ explicit KArgs(KSeg *b) : base_(b) {}
    template <class Kernel>
    friend __device__ KArgs kernel_kargs();

public:
    template <class T>
    __device__ __forceinline__ T get(size_t off) const {
        return *(volatile const T __attribute__((address_space(4))) *)(base_ + off);
    }
    // the whole TraceArgs, for a rare path that hands it to code written against the struct (the replay)
    __device__ __forceinline__ TraceArgs args() const {
        return *(const TraceArgs *)base_;
    }
};

// Call in the body of the __global__ function Kernel itself: kernel_kargs<decltype(my_kernel<...>)>().
template <class Kernel>
__device__ __forceinline__ KArgs kernel_kargs() {
    static_assert(same_type<typename first_param<Kernel>::type, TraceArgs>::value,
                  "KArgs reads TraceArgs fields at their offsets in the kernarg segment: the kernel's first "
                  "parameter must be the TraceArgs");
    return KArgs((KSeg *)__builtin_amdgcn_kernarg_segment_ptr());
}

// A TraceArgs field through the handle K in scope.
#define KA(f) K.template get<decltype(TraceArgs::f)>(offsetof(TraceArgs, f))
// the same for the locator's exact-test arrays (TraceArgs::loc holds them for every variant)
#define KLOCP(Kp, f) (Kp)->template get<decltype(Locator::f)>(offsetof(TraceArgs, loc) + offsetof(Locator, f))
#define KLOC(f) KLOCP(&K, f)

// Global id of local ray i (wgrt_launch_opts.gid_blocks): only the zero-state RNG fix-up reads it.
__device__ __forceinline__ int64_t ray_gid(const TraceArgs &A, int64_t i) {
    return A.gid_blocks ? A.gid_blocks[i / A.gid_block_rays] + i % A.gid_block_rays : A.gid_offset + i;
}
// The same from the kernarg segment.
__device__ __forceinline__ int64_t ray_gid_ka(const KArgs &K, int64_t i) {
    const int64_t *gb = KA(gid_blocks);
    if (gb) {
        const int64_t r = KA(gid_block_rays);
        return gb[i / r] + i % r;
    }
    return KA(gid_offset) + i;
}

// What a lane's step returns besides a block index / region (the Jones-vector lane adds two, wgrt_jones_lane.h).
enum : int { kDie = -1, kTransit = -2 };
constexpr int kChunk = 64;   // rays per work-queue chunk of the Jones-vector variants (chunk_order unit)

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// The counters a kernel accumulates: one 64-bit word per wgrt_trace_stats field, in the struct's order, so
// word k of a record adds to word k of *stats.  Every site that sums, parks or publishes counters goes
// through this record; a word a kernel never touches stays a compile-time zero and costs nothing up to
// the first trip through memory.
enum Ctr : int { kCtrBounces, kCtrBadRays, kCtrHits, kCtrReplayed, kCtrGiveups, kCtrInter, kCtrLibm, kCtrWords };
static_assert(sizeof(wgrt_trace_stats) == kCtrWords * sizeof(uint64_t) &&
                  offsetof(wgrt_trace_stats, bounces) == 8 * kCtrBounces &&
                  offsetof(wgrt_trace_stats, bad_rays) == 8 * kCtrBadRays &&
                  offsetof(wgrt_trace_stats, eyebox_hits) == 8 * kCtrHits &&
                  offsetof(wgrt_trace_stats, replayed) == 8 * kCtrReplayed &&
                  offsetof(wgrt_trace_stats, handoff_giveups) == 8 * kCtrGiveups &&
                  offsetof(wgrt_trace_stats, interactions) == 8 * kCtrInter &&
                  offsetof(wgrt_trace_stats, libm_rays) == 8 * kCtrLibm,
              "Ctr names the words of wgrt_trace_stats: a new field gets its index here");
constexpr int kPartWords = (kCtrWords + 7) / 8 * 8;   // a trace workgroup's partial slot: whole 64-B lines

struct Counters {
    unsigned long long w[kCtrWords] = {};

    // every lane's record -> its wave's sums (in every lane)
    __device__ __forceinline__ void wave_reduce() {
        for (int k = 0; k < kCtrWords; ++k) w[k] = wave_sum(w[k]);
    }
    // ... -> the 256-thread workgroup's sums through one LDS array: valid in thread 0 only
    __device__ __forceinline__ void block_reduce(unsigned long long (&red)[4][kCtrWords]) {
        wave_reduce();
        if ((threadIdx.x & 63) == 0)
            for (int k = 0; k < kCtrWords; ++k) red[threadIdx.x >> 6][k] = w[k];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int k = 0; k < kCtrWords; ++k) w[k] = red[0][k] + red[1][k] + red[2][k] + red[3][k];
    }
    // the non-zero words added to kCtrWords words of memory, *stats or a launch's totals (the atomics commute)
    __device__ __forceinline__ void add_to(unsigned long long *dst) const {
        for (int k = 0; k < kCtrWords; ++k)
            if (w[k]) atomicAdd(dst + k, w[k]);
    }
    // (st != NULL is the caller's test, made with its own condition: folded in here it cost the single-launch
    // kernels a VGPR across the wave loop, profiles/untangle_kernel_identity.md)
    __device__ __forceinline__ void add_to(wgrt_trace_stats *st) const { add_to((unsigned long long *)st); }
    // parked in / added from a partial slot that only this workgroup writes and a later kernel reads
    __device__ __forceinline__ void store(unsigned long long *slot) const {
        for (int k = 0; k < kCtrWords; ++k) slot[k] = w[k];
    }
    __device__ __forceinline__ void add_from(const unsigned long long *slot) {
        for (int k = 0; k < kCtrWords; ++k) w[k] += slot[k];
    }
    // totals other workgroups of this kernel added with agent-scope atomics
    __device__ __forceinline__ void load_agent(const unsigned long long *acc) {
        for (int k = 0; k < kCtrWords; ++k) w[k] = __hip_atomic_load(acc + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

}  // namespace wgrt
