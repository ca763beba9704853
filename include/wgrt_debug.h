/*
 * wgrt_debug.h -- test and profiling hooks of libwgrt.so (not part of the drop-in boundary).
 *
 * Nothing here is process-wide state: every hook is either a separate entry point or a
 * per-call option block (wgrt_launch_opts.debug), so these hooks are as thread-safe as the
 * calls they ride on.  The production path passes debug = NULL and runs instantiations of the
 * kernels that contain none of this code (the wave timeline is a template parameter of the
 * persistent kernel, off in the product instantiation).
 */
#ifndef WGRT_DEBUG_H
#define WGRT_DEBUG_H

#include "wgrt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per-call overrides of a Jones-vector launch (wgrt_launch_opts.debug). */
struct wgrt_debug_opts {
    /* Base of the double-precision certification bound (0: default 1e-10) and of the
     * single-precision estimate's (0: default 8e-6; the effective value is max(this, cert_tol)).
     * Larger values make more decisions uncertain (more double-precision re-evaluations, more
     * rays through the replay kernel); results unchanged. */
    double cert_tol;
    double cert_tol32;
    /* Rays per work-queue item (0: 64; at most 64: an item is staged one ray per lane).
     * Smaller items make a refill span several items; results unchanged. */
    int chunk_rays;
    /* Wave timeline: when non-NULL, the launch runs the instrumented instantiation and records,
     * per wave w < timeline_waves of its grid, 8 words at timeline[8 w ..]: start,
     * queue-exhausted and end times (s_memrealtime, 100 MHz), passes of the wave loop,
     * lane-passes with a ray in flight, XCD id, and the passes and lane-passes before the
     * queue ran dry (DEVICE buffer). */
    unsigned long long *timeline;
    int64_t timeline_waves;
    /* Fault injection: 1 makes the call return WGRT_ERR_HIP right after the trace kernel is
     * enqueued, before the epilogue kernel (the recovery path of a launch that fails half-way;
     * the next call on the stream must still be exact). */
    int fail_after_trace;
    /* Fused launches: hand-off wait bound in s_memrealtime ticks (100 MHz); 0 = the default
     * derived from num_iter.  A tiny bound makes waiting traces give up
     * (counted in wgrt_trace_stats.handoff_giveups).  Without it, a trace is given up only once the
     * default bound has passed AND the waiting wave has run 4096 passes since the wait began (a wave
     * that was descheduled does not give up a correct hand-off); a given-up ray is marked abandoned,
     * so its later traces in the call skip it instead of waiting again. */
    uint64_t handoff_wait_ticks;
};

/* Certification shadow of the Jones-vector variants (diagnostic; wgrt_shadow.hip).  Traces rays
 * [0, n_rays) with the reference's own arithmetic (unwrapped delta_phase, hypot / atan2 / wrap,
 * GRTF:132-152 and 905-1246) and, at every Monte-Carlo decision, evaluates the Jones-vector lane's
 * thresholds and certification bound tol (default bases) on the same state.  rng_states (DEVICE,
 * in/out) and the optional per_ray_bounces follow the reference's path, so they equal one launch
 * of the exact kernel; matrix_EB is not written.  stats: DEVICE pointer, ADDED to (zero it
 * yourself); max fields are max-combined.  single: the single-wavelength kernel (threshold 1e-15). */
typedef struct {
    uint64_t decisions;          /* Monte-Carlo decisions evaluated                                 */
    uint64_t uncertain;          /* decisions the Jones lane cannot certify (its rays are replayed)   */
    uint64_t silent_flips;       /* certified Jones decisions that differ from the reference's: 0    */
    uint64_t bounces;            /* ray-bounce events traced                                          */
    uint64_t fallbacks;          /* decisions the single-precision estimate leaves to the double one  */
    double max_ratio;            /* max over decisions / thresholds of |c_jones64 - c_ref| / tol64    */
    double max_ratio32;          /* the same for the single-precision estimate against tol32          */
    double max_ratio_by_depth[6];   /* max_ratio32 by bounce depth [1,10) [10,30) [30,100) [100,300)
                                       [300,1000) [1000,inf)                                          */
    uint64_t decisions_by_depth[6];
    uint64_t ratio_hist[20];     /* decisions by log10 of their ratio32: bucket b = [1e(b-18),
                                    1e(b-17)); bucket 0 also holds smaller ratios, 19 larger ones    */
    double max_ener_ratio;       /* single wavelength: max |ener_jones / ener_ref - 1| / tracked bound */
    double max_amp;              /* the largest amplification bound a Jones lane carried (JRay::amp; 1 on
                                    scaled-unitary LUTs) */
} wgrt_shadow_stats;

wgrt_status wgrt_debug_shadow(const wgrt_scene *scene, const wgrt_rays *rays, int64_t n_rays, int64_t gid_offset,
                              int single, uint32_t *rng_states, uint32_t *per_ray_bounces, wgrt_shadow_stats *stats,
                              void *stream);

/* Copies one of a scene's device structures to host memory dst (bytes must equal its size):
 * which = 0 the locator cell words (uint64, ncx * ncy), 1 the exact lane's tiles, 2 the
 * Jones-vector tiles (doubles, tiles * tile / jtile doubles; wgrt_scene_info), 3 the byte locator's
 * byte grid (uint8, ncx * ncy), 4 its palette (uint64, 256); 3 and 4 are WGRT_ERR_UNSUPPORTED for a scene
 * without a byte grid. */
wgrt_status wgrt_debug_scene_copy(const wgrt_scene *scene, int which, void *dst, int64_t bytes);

/* The automatic issue order of single full-colour traces (csrc/wgrt_order.h): a scene counts, per
 * (wavelength, FoV) tile, the traces of its first launches that took more than 24 bounces (until it has
 * seen 1024 rays per tile), and later launches without a chunk_order issue their 64-ray chunks in
 * descending classes of that count.  A scheduling hint: results do not depend on it.  This switch is the
 * one piece of process-wide state here (for A/B timing and tests): 0 turns learning and ordering off, so
 * every launch runs as if the scene had no table; default 1. */
wgrt_status wgrt_debug_set_auto_order(int on);
/* The byte locator of the Jones-vector lane (csrc/wgrt_args.h ByteLocatorT): a scene whose locator grid holds
 * at most 256 distinct cell words also keeps a byte per cell (its index into the palette of those words), and
 * its Jones-vector launches gather that byte instead of the 4- or 8-byte word.  Results do not depend on it.
 * Process-wide, like the switch above, for the same-binary A/B and the tests: 0 makes every launch run the
 * word-form kernels; default 1. */
wgrt_status wgrt_debug_set_byte_locator(int on);
/* The run length of fused launches (num_iter > 1; csrc/wgrt_items.h): a work item covers a run of that many
 * consecutive traces of its chunk's rays, and the lane that takes a ray keeps it for the run -- the RNG state stays in
 * the lane from one trace to the next, and only a run's last trace hands the ray on through memory.  A scheduling
 * detail like the chunk order: results do not depend on it.  Process-wide, for the same-binary A/B and the tests:
 * 0 (the default) lets the library choose from num_iter (at least four runs per launch, runs of at most 16), 1 is
 * one item per trace (a hand-off after every trace), n runs of n; a value that is not a power of two, or above 64,
 * is WGRT_ERR_INVALID_ARGUMENT.  A call whose wgrt_debug_opts.handoff_wait_ticks is not 0 asks for hand-offs and
 * runs with 1 under the automatic choice; an explicit value here wins. */
wgrt_status wgrt_debug_set_fused_run(int run);
/* The run length a fused launch of num_iter traces runs with now (the switch, else the automatic choice;
 * handoff_bound != 0: for a call with a debug hand-off bound). */
wgrt_status wgrt_debug_fused_run(int num_iter, int handoff_bound, int *run);
/* The work items of a fused launch, from the code the kernels compile (csrc/wgrt_items.h; needs no GPU): positions
 * q0 .. q0 + n - 1 of head's (0 .. 7) queue for n_chunks chunks, num_iter traces and runs of `run`.  Item k's chunk,
 * first trace and end trace (exclusive) go to chunk[k], first_trace[k], end_trace[k]; *count is the number of
 * positions before the head's queue ends (<= n). */
wgrt_status wgrt_debug_fused_items_host(int64_t n_chunks, int num_iter, int run, int head, int64_t q0, int64_t n,
                                        int64_t *chunk, int32_t *first_trace, int32_t *end_trace, int64_t *count);
/* The taper of fused launches (csrc/wgrt_items.h): with a first tail length t0 -- a power of two below the run length
 * -- the launch's last 2 t0 - 1 traces are runs of t0, t0 / 2, ..., 2, 1 traces, and the runs before them are aligned
 * from there backwards, so the launch drains like a single trace.  A scheduling detail like the run length: results
 * do not depend on it.  Process-wide, for the same-binary A/B and the tests: -1 (the default) is the library's
 * rule -- a launch whose run length is automatic tapers from half its run where that was measured faster (runs of 8
 * or more, batches of 7,500 to 42,000 64-ray chunks), an explicit run length
 * (wgrt_debug_set_fused_run) means uniform runs; 0 never tapers; a power of two is that t0 for every fused launch,
 * also beside an explicit run length (halved until it is below the launch's run).  Anything else is
 * WGRT_ERR_INVALID_ARGUMENT. */
wgrt_status wgrt_debug_set_fused_taper(int t0);
/* The first tail length a fused launch of num_iter traces of n_rays rays runs with now (0: no taper; handoff_bound
 * as above). */
wgrt_status wgrt_debug_fused_taper(int num_iter, int64_t n_rays, int handoff_bound, int *t0);
/* The run partition of a fused launch and its work items under it, from the code the kernels compile (needs no GPU):
 * num_iter (1 .. 255) traces in runs of `run` with first tail length t0 (0, or a power of two below run).
 * *n_runs is the number of runs and run_first_trace[r] the first trace of run r, filled for r < *n_runs only;
 * trace_first[k] and trace_end[k] (exclusive) are the run that holds trace k, as the dequeue derives it.  The
 * caller gives all three arrays num_iter entries (a launch has at most num_iter runs).  The item arrays are
 * wgrt_debug_fused_items_host's, under this partition. */
wgrt_status wgrt_debug_fused_partition_host(int64_t n_chunks, int num_iter, int run, int t0, int head, int64_t q0,
                                            int64_t n, int32_t *n_runs, int32_t *run_first_trace, int32_t *trace_first,
                                            int32_t *trace_end, int64_t *chunk, int32_t *first_trace,
                                            int32_t *end_trace, int64_t *count);
/* The most distinct cell words a scene created from now on may have and still get a byte grid (0 .. 256,
 * larger values mean 256; default 256): a test forces the word-form fallback with it. */
wgrt_status wgrt_debug_set_palette_cap(int cap);
/* A scene's distinct cell words (saturating at 2048), whether it has a byte grid, and whether its launches
 * run the byte locator now (byte grid and switch).  Each output may be NULL. */
wgrt_status wgrt_debug_scene_palette(const wgrt_scene *scene, int *distinct_words, int *byte_grid, int *active);
/* Copies the order the stream's last automatically ordered launch used to host memory (n must be its
 * ceil(n_rays / 64) chunks); WGRT_ERR_INVALID_ARGUMENT when the stream has built none.  Waits for the stream. */
wgrt_status wgrt_debug_get_auto_order(const wgrt_scene *scene, void *stream, int32_t *out, int64_t n);
/* The replay list of the stream's last expected-value launch (wgrt_trace_expected, variants 7 / 9): the local index
 * of each of its first n abandoned rays and the scored visits its replay passed over (the deposits the Jones-vector
 * lane had made before it abandoned the ray), to host memory; n at most the launch's wgrt_trace_stats.replayed.
 * Valid until the next launch on the stream.  Waits for the stream. */
wgrt_status wgrt_debug_expected_replays(const wgrt_scene *scene, void *stream, uint32_t *rays, uint32_t *skipped, int64_t n);
/* Copies the scene's tile table (uint32 counts, n = num_lmd * nx * ny, index (lambda * nx + m) * ny + n)
 * to host memory.  Waits for the device. */
wgrt_status wgrt_debug_get_tile_tail(const wgrt_scene *scene, uint32_t *out, int64_t n);
/* The order kernel's arithmetic on the host (no device): the issue order of n_chunks chunks, chunk c
 * belonging to tile chunk_tile[c] (out of [0, n_tiles): no tile, the lowest class), from the table
 * tile_tail[n_tiles]. */
wgrt_status wgrt_debug_order_host(const uint32_t *tile_tail, int64_t n_tiles, const int32_t *chunk_tile,
                                  int64_t n_chunks, int32_t *order);

/* The host logic of a chain (wgrt_chain_step; no device): where the next step goes, given what the step is
 * (flags) and where the chain stands (in_segment: chained steps issued since the segment opened, -1 when no
 * segment is open; serial: the last granule tag serial handed out).  Any flag makes the step a plain launch
 * on the caller's stream, behind a join when a segment is open.  A chained step opens a segment when none is
 * open (seed: rng_states -> granules on the caller's stream, the side stream made to wait for it) and closes
 * and reopens it when the tag serial would run out (WGRT_CHAIN_SERIAL_MAX); step k of a segment goes to the
 * caller's stream for even k and to the side stream for odd k, waits for the tag serial - 1 and publishes
 * serial. */
#define WGRT_CHAIN_LEARNS 1u      /* the launch would still learn the scene's tile table */
#define WGRT_CHAIN_VARIANT1 2u    /* variant 1, or auto on more than 2^32 - 1 rays */
#define WGRT_CHAIN_SINGLE 4u      /* the single-wavelength kernel */
#define WGRT_CHAIN_FUSED 8u       /* num_iter > 1 */
#define WGRT_CHAIN_DEBUG 16u      /* chunk_order or a debug timeline */
#define WGRT_CHAIN_CAPTURE 32u    /* the caller's stream is under graph capture */
#define WGRT_CHAIN_FULL 64u       /* the launch's own grid is the kernel's resident grid: it fills the chip alone */
#define WGRT_CHAIN_SERIAL_MAX 0x7ffffffeu
typedef struct {
    int chained;        /* 1: the chained kernel; 0: a plain launch on the caller's stream */
    int side;           /* 0: the caller's stream, 1: the side stream */
    int join;           /* 1: the open segment is closed first (side stream joined, finalize) */
    int seed;           /* 1: a segment is opened first (after the join, if any) */
    int clear;          /* 1: the granules are cleared and the serial restarts before the seed */
    uint32_t wait_serial, publish_serial;   /* chained: the tag it takes states from, the tag it publishes */
    uint32_t serial_after;                  /* the chain's serial after the step */
    int64_t in_segment_after;               /* ... and its in_segment */
} wgrt_chain_plan;
wgrt_status wgrt_debug_chain_plan(int64_t in_segment, uint32_t serial, uint32_t flags, wgrt_chain_plan *out);
/* Sets the tag serial of the stream's granules (clearing them), so that a test reaches WGRT_CHAIN_SERIAL_MAX
 * within a few steps.  No chain may be open on the stream.  Waits for the stream. */
wgrt_status wgrt_debug_chain_set_serial(const wgrt_scene *scene, void *stream, uint32_t serial);
/* What an open chain has done so far (host counters; no device).  A gathering chain (wgrt_chain_gather, wgrt.h)
 * launches a step at once when the stream has finished what the chain issued before, and otherwise counts it;
 * counted steps go out as one fused launch.  steps - plain_steps steps went into launches - plain_steps gathered
 * launches, of which fused_launches carried more than one step, the largest largest_launch; steps not yet launched
 * are pending.  A chain that does not gather reports gathering = 0 and zeros. */
typedef struct {
    int gathering;            /* 1: wgrt_chain_gather took effect; 0: one kernel per step (two queues, or plain)    */
    int cap;                  /* gathering: the most steps one launch takes                                          */
    int64_t steps;            /* gathering: wgrt_chain_step calls so far                                             */
    int64_t launches;         /* ... trace launches made for them                                                    */
    int64_t fused_launches;   /* ... of which carried more than one step                                             */
    int64_t largest_launch;   /* ... the most steps in one launch                                                    */
    int64_t plain_steps;      /* ... steps that ran as plain launches (learning launches, a stream under capture)    */
    int64_t pending;          /* ... steps counted and not yet launched                                              */
} wgrt_chain_report;
wgrt_status wgrt_debug_chain_report(const wgrt_chain *chain, wgrt_chain_report *out);

/* The footprint sink's two forms in one binary (wgrt_trace_footprint; process-wide; the A/B and the tests): 1 (the
 * default) sums the counts that share a map entry on chip before they go to the map -- the Jones-vector lane in a
 * per-wave counter cache in LDS, the exact lane over the lanes of a wave; 0 issues one global atomic per count.  Both
 * give the same map. */
wgrt_status wgrt_debug_set_footprint_aggregate(int on);

/* The two forms of wgrt_visits_reweight_many's deposits in one binary (process-wide; the A/B and the tests): 1 (the
 * default) adds a chunk of 64 designs into a scratch [n_slabs * W, 64], where a wave's 64 adds are contiguous, and
 * folds the scratch into the tables with a second kernel; 0 adds straight into out [K, n_slabs, W], a wave's adds on 64
 * cache lines.  Both give the same tables and weight sums. */
wgrt_status wgrt_debug_set_reweight_layout(int interleaved);

/* The Jones-vector trace kernels the library holds (csrc/wgrt_trace.hip JonesKernels; host only: no GPU, no scene): the
 * kernel table is indexed [mode][byte locator][64-bit cells][fused][single wavelength][AMP], modes in TraceMode's order
 * (csrc/wgrt_trace_mode.h), every other index 0 or 1.  built[i] becomes 1 where entry i, in that order, is an
 * instantiation the library was built with, and 0 where it is not; n must be the table's modes * 32 entries. */
wgrt_status wgrt_debug_trace_kernels(uint8_t *built, int64_t n);
/* The table entry the scene's last launch looked its kernel up at, as the six indices above; all -1 when that launch
 * ran a grid or exact-lane kernel (variant 1), or when the scene has launched nothing.  Recorded on the host when the
 * launch is issued (a fused chain of variant 1 launches records each), so it says which kernel was asked for, without
 * waiting for it. */
wgrt_status wgrt_debug_last_trace_kernel(const wgrt_scene *scene, int32_t idx[6]);

#ifdef __cplusplus
}
#endif
#endif /* WGRT_DEBUG_H */
