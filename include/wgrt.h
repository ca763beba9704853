/*
 * wgrt.h -- C ABI of the MI355X waveguide ray-tracing engine (libwgrt.so).
 *
 * Drop-in boundary for the reference's hot path, the Numba kernel call
 *
 *   process_rays_kernel_pro_fullColor[blocks, threads](
 *       x_v, y_v, gap_x_v, gap_y_v, pol_v, azi_v, m_v, n_v, lmd_num, te_v, tm_v, delta_phase_v,
 *       rng_states, IC, FC, FC_offset, OC, OC_offset, n_g,
 *       eff_reg1, eff_reg2, eff_reg_FOV, eff_reg_FOV_range,
 *       lut_ic1, lut_ic2, lut_ic3, lut_fc1, lut_fc2, lut_oc1, lut_oc2, lut_TIR, lut_gap, matrix_EB)
 *
 * (reference GPU_ray_tracing_functions.py:833-841, launched at
 * gpu_ray_tracing_pro_fullColor.py:169-177).  The 33 arguments split into
 *   - the scene (geometry + LUTs, 19 arguments, constant across launches):
 *       wgrt_scene_create()  -- replaces the cuda.to_device uploads at MAIN:40-57
 *   - the per-launch ray batch, RNG state and eyebox grid (14 arguments):
 *       wgrt_trace_fullcolor() -- replaces one kernel launch (MAIN:170)
 *
 * Conventions (same as the reference's): the caller owns every buffer; the
 * trace call allocates nothing, accumulates into matrix_EB (never zeroes it),
 * mutates rng_states, leaves the ray arrays untouched, and is asynchronous on
 * the given HIP stream (the caller synchronises, MAIN:178).  Differences: every
 * entry point validates its arguments and returns a wgrt_status instead of
 * silently corrupting memory; out-of-range m / n / lmd_num rays are skipped
 * and counted (wgrt_trace_stats.bad_rays) rather than read out of bounds.
 *
 * All pointers passed to wgrt_trace_* are DEVICE pointers (hipMalloc'd or torch
 * ROCm tensors); all pointers in wgrt_scene_desc are HOST pointers.
 *
 * Devices: a scene lives on the HIP device it was created on.  Every entry point
 * that takes a scene allocates and launches on that device, and every entry point
 * leaves the calling thread's current device (hipGetDevice) as it found it, so one
 * host thread may drive scenes on several GPUs.  wgrt_rays_init and
 * wgrt_selftest_math launch on their stream's device (the current one for the null
 * stream).  A stream passed with a scene must belong to the scene's device.
 */
#ifndef WGRT_H
#define WGRT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WGRT_ABI_VERSION 9

typedef enum {
    WGRT_OK = 0,
    WGRT_ERR_INVALID_ARGUMENT = 1,
    WGRT_ERR_HIP = 2,
    WGRT_ERR_OUT_OF_MEMORY = 3,
    WGRT_ERR_UNSUPPORTED = 4,
} wgrt_status;

/* Geometry + look-up tables, exactly the arrays couplers_coor_full_color() and the
 * seven lut_*_fullColor.npy files provide (reference couplers_coor.py:740-750,
 * gpu_ray_tracing_pro_fullColor.py:19-34).  Host pointers, C-contiguous. */
typedef struct {
    const double *IC;                 /* [n_ic, 2]                                   */
    int64_t n_ic;
    const double *FC;                 /* [FC_offset[n_fc_slices], 2]                  */
    const int64_t *FC_offset;         /* [n_fc_slices + 1]                            */
    int64_t n_fc_slices;
    const double *OC;                 /* [OC_offset[n_oc_slices], 2]                  */
    const int64_t *OC_offset;         /* [n_oc_slices + 1]                            */
    int64_t n_oc_slices;
    double n_g;                       /* substrate index                              */
    const double *eff_reg1;           /* [n_eff_reg1, 2] whole effective region       */
    int64_t n_eff_reg1;
    const double *eff_reg2;           /* [n_eff_reg2, 2] IC+FC effective region       */
    int64_t n_eff_reg2;
    const double *eff_reg_FOV;        /* [nx, ny, 4, 2] per-FoV eyebox rectangle      */
    const double *eff_reg_FOV_range;  /* [nx, ny, 4] = xmin, xmax, ymin, ymax         */
    /* complex128 tables, interleaved (re, im); channel counts ch5 (>= 41), ch3 (>= 20) */
    const double *lut_ic1, *lut_ic2, *lut_ic3;   /* [num_lmd, nx, ny, ch5]              */
    const double *lut_fc1, *lut_fc2;             /* [n_fc_slices, num_lmd, nx, ny, ch3] */
    const double *lut_oc1, *lut_oc2;             /* [n_oc_slices, num_lmd, nx, ny, ch5] */
    int32_t ch5, ch3;
    const double *lut_TIR;            /* [num_lmd, nx, ny, 4]                         */
    const double *lut_gap;            /* [num_lmd, nx, ny, 8]                         */
    int32_t num_lmd, nx, ny;
} wgrt_scene_desc;

typedef struct wgrt_scene wgrt_scene;   /* opaque, device-resident */

/* The twelve per-ray float32 columns of the reference (MAIN:65-76), device pointers.
 * Columns the kernel never reads (gap_x, gap_y, pol, azi: overwritten before use at
 * GRTF:872-894) may be NULL. */
typedef struct {
    const float *x, *y, *gap_x, *gap_y, *pol, *azi, *m, *n, *lmd_num, *te, *tm, *delta_phase;
} wgrt_rays;

/* The same twelve columns as outputs (wgrt_rays_init). */
typedef struct {
    float *x, *y, *gap_x, *gap_y, *pol, *azi, *m, *n, *lmd_num, *te, *tm, *delta_phase;
} wgrt_ray_columns;

typedef struct {
    uint64_t bounces;          /* ray-bounce events: 1 in-coupling + loop iterations, per ray      */
    uint64_t bad_rays;         /* rays skipped for out-of-range m / n / lmd_num                    */
    uint64_t eyebox_hits;      /* rays accumulated into matrix_EB                                  */
    uint64_t replayed;         /* Jones-vector variants: rays abandoned on an uncertain decision and
                                  re-traced with the reference arithmetic (included in the counts above) */
    uint64_t handoff_giveups;  /* fused launches (num_iter > 1): traces given up because the previous
                                  trace of their ray never handed over within the bound of
                                  wgrt_launch_opts.num_iter.  Never in a correct
                                  run: a nonzero count means the eyebox grid and the RNG states of
                                  this call are wrong, and the Python layer raises on it.           */
    uint64_t interactions;     /* ABI 5.  Monte-Carlo interactions of the bounce loop (the iterations of
                                  GRTF:905 that draw: coupler hits in R0..R5).  The other bounces are the
                                  in-coupling events (one per traced ray, GRTF:860-904) and the iterations
                                  without a draw: miss hops, R3 -> R4 switches, terminations.          */
    uint64_t libm_rays;        /* ABI 7.  Traces decided in the ener-underflow regime: a guard product
                                  ener * e_k (GRTF:1020, 1073, 1136, ...) of a nonzero efficiency fell below
                                  2^-1000, where whether it rounds to zero -- and so the ray's path --
                                  depends on the last bits of cos / sin / atan2 (glibc vs the device libm),
                                  not on the reference's formula alone.  Such traces are decided by the
                                  reference arithmetic (the Jones-vector lane abandons them to it), and
                                  are counted here; the Python layer warns (LUTPrecisionWarning) when the
                                  count is nonzero.  0 on every BASELINE configuration. */
} wgrt_trace_stats;

typedef struct {
    int64_t tile_bytes;        /* packed per-(lambda, FoV) LUT tile                   */
    int64_t tiles;             /* num_lmd * nx * ny                                   */
    int64_t grid_cells_x, grid_cells_y;
    double grid_cell_mm;
    int64_t grid_edge_cells;   /* cells whose class needs the exact polygon test      */
    int32_t n_polygons;
    int32_t device;
    int64_t jtile_bytes;       /* Jones-vector tile per (lambda, FoV) (variants 7 / 9)  */
    int64_t nonunitary_blocks; /* ABI 7.  Interaction blocks whose taken branches' Jones matrices are not
                                  scaled-unitary (kappa^2 > 1 + 1e-6): the Jones-vector variants then run
                                  their amplification-tracked certification             */
} wgrt_scene_info;

/* Build the device-resident scene (packs LUT tiles, builds the exact polygon
 * locator) on HIP device `device`.  Replaces MAIN:40-57. */
wgrt_status wgrt_scene_create(const wgrt_scene_desc *desc, int device, wgrt_scene **out);

/* Scene build options (wgrt_scene_create uses the defaults). */
typedef struct {
    double cell_mm;   /* locator grid cell (mm); 0 = default 1/128 mm (fastest on C3) */
    int host_build;   /* 1: build the cell words and tiles on the host (the reference the device build
                         is checked against; slow); 0: on the device                              */
    int lut_f32_angles;   /* ABI 4.  Bit k set: LUT k (lut_ic1, ic2, ic3, fc1, fc2, oc1, oc2) was a
                             complex64 table in the reference's run (MAIN:28-34 loads the .npy files as
                             stored).  Compiled numba takes math.cos of a complex64 table's float32 .real
                             in single precision (GRTF:866-869 and every cos ratio after it), so the
                             scene's cosines of that table's angles are cosf of the float32 angle,
                             widened.  The coefficients themselves enter E_field_cal widened exactly, as
                             numba promotes complex64 x complex128.  0: double-precision cos (complex128).
                             ABI 5: only 0 and 0x7f (all seven tables complex64) are accepted; a mixed set
                             is WGRT_ERR_UNSUPPORTED (numba would carry the ray's angle as complex128 while a
                             complex64 table's own cosine stays float32: see wgrt_scene_create_ex). */
} wgrt_scene_opts;
wgrt_status wgrt_scene_create_ex(const wgrt_scene_desc *desc, int device, const wgrt_scene_opts *opts,
                                 wgrt_scene **out);
wgrt_status wgrt_scene_destroy(wgrt_scene *scene);
wgrt_status wgrt_scene_get_info(const wgrt_scene *scene, wgrt_scene_info *info);

/* One launch of the full-colour bounce kernel over rays [0, n_rays) whose global
 * ray index is gid_offset + i (gid seeds the zero-state RNG fix-up, GRTF:28-29, and
 * keeps results independent of sharding).  rng_states[n_rays] is read and written;
 * matrix_EB [num_lmd, ny, nx, 80, 120] float32 is accumulated into.
 *   stats:          optional DEVICE pointer to a wgrt_trace_stats that is ADDED to
 *                   (zero it yourself);
 *   per_ray_bounces: optional DEVICE uint32[n_rays] of per-ray bounce counts;
 *   stream:         hipStream_t (NULL = default stream).
 * Replaces gpu_ray_tracing_pro_fullColor.py:170 (GRTF:833-1246). */
wgrt_status wgrt_trace_fullcolor(const wgrt_scene *scene, const wgrt_rays *rays, int64_t n_rays,
                                 int64_t gid_offset, uint32_t *rng_states, float *matrix_EB,
                                 wgrt_trace_stats *stats, uint32_t *per_ray_bounces, void *stream);

/* Same as wgrt_trace_fullcolor with launch tuning: kernel variant and workgroup
 * count for the persistent variants (0 = automatic).  variant:
 *   0 auto (7 when the scene has <= 16 polygons, else 9; 1 beyond 2^32 - 1 rays);
 *   1 one ray per lane over a ceil(N / 256) x 256 grid (the reference's launch shape) with the
 *     reference's arithmetic;
 *   7 the persistent wave loop over the Jones-vector state with certified decisions, 32-bit
 *     locator cell words (<= 16 polygons, else WGRT_ERR_UNSUPPORTED);
 *   9 the same with 64-bit cell words (<= 32 polygons).
 * Variants 7 / 9 re-trace the rays whose decision they cannot certify with the reference
 * arithmetic in a second kernel on the same stream (wgrt_trace_stats.replayed counts them); the
 * first such launch on a stream allocates per-stream scratch (see wgrt_scene_reserve).  Other
 * values (the retired variants 2-6 and 8 of ABI 1) are WGRT_ERR_INVALID_ARGUMENT.  All variants
 * produce identical results. */
wgrt_status wgrt_trace_fullcolor_ex(const wgrt_scene *scene, const wgrt_rays *rays, int64_t n_rays,
                                    int64_t gid_offset, uint32_t *rng_states, float *matrix_EB,
                                    wgrt_trace_stats *stats, uint32_t *per_ray_bounces, void *stream,
                                    int variant, int workgroups);

/* One launch of the single-wavelength bounce kernel process_rays_kernel_pro
 * (reference GPU_ray_tracing_functions.py:419-831): the 32-argument form without the
 * lmd_num column, LUTs [nx, ny, ch] / [n_slices, nx, ny, ch] (a wgrt_scene_desc with
 * num_lmd = 1 has exactly that memory layout), matrix_EB [ny, nx, 80, 120], and the
 * R2..R5 branch guard ener * efficiency > 1e-15 (GRTF:444) instead of > 0.
 * rays->lmd_num is ignored and may be NULL.  WGRT_ERR_INVALID_ARGUMENT if the scene has
 * num_lmd != 1.  Everything else as wgrt_trace_fullcolor / _ex. */
wgrt_status wgrt_trace_single(const wgrt_scene *scene, const wgrt_rays *rays, int64_t n_rays, int64_t gid_offset,
                              uint32_t *rng_states, float *matrix_EB, wgrt_trace_stats *stats,
                              uint32_t *per_ray_bounces, void *stream);
wgrt_status wgrt_trace_single_ex(const wgrt_scene *scene, const wgrt_rays *rays, int64_t n_rays,
                                 int64_t gid_offset, uint32_t *rng_states, float *matrix_EB,
                                 wgrt_trace_stats *stats, uint32_t *per_ray_bounces, void *stream, int variant,
                                 int workgroups);

/* Launch options for wgrt_trace_opts. */
typedef struct wgrt_debug_opts wgrt_debug_opts;   /* include/wgrt_debug.h (test / profiling hooks) */
typedef struct {
    int kernel;          /* 0 process_rays_kernel_pro_fullColor, 1 process_rays_kernel_pro (single lambda) */
    int variant;         /* as wgrt_trace_fullcolor_ex (0 auto)                                           */
    int workgroups;      /* persistent variants: resident workgroups (0 auto)                             */
    /* Persistent variants: order in which the 64-ray chunks [64 c, 64 c + 64) are handed to
     * the waves -- a DEVICE int32 permutation of 0 .. ceil(n_rays / 64) - 1, or NULL for
     * ascending order.  Results do not depend on it (rays are independent).  The permutation
     * is not validated on the device. */
    const int32_t *chunk_order;
    int64_t n_chunk_order;
    /* Chained traces per call (0 or 1: one).  num_iter = K gives exactly the results of K
     * successive launches over the same rays (the reference's num_iter loop, MAIN:169-177):
     * every ray is traced K times, each trace starting from the RNG state the previous one
     * left, all out-couplings binned into matrix_EB, rng_states left at the last trace's
     * states, stats summed over the K traces.  Variants 7-9 run the K traces in ONE
     * persistent launch (one iteration's straggler tail overlaps the next one's bulk);
     * the others issue K launches.  1 <= num_iter <= 255; num_iter > 1 needs
     * per_ray_bounces == NULL and chunk_order == NULL. */
    int num_iter;
    /* Global ray ids of a shard made of several FoV x wavelength block ranges (multi-GPU
     * interleaved sharding): when gid_blocks (DEVICE int64[ceil(n_rays / gid_block_rays)]) is
     * non-NULL, local ray i has global id gid_blocks[i / gid_block_rays] + i % gid_block_rays
     * and the call's gid_offset must be 0; NULL: global id gid_offset + i.  The global id seeds
     * the zero-state RNG fix-up (GRTF:28-29) and nothing else, so results equal a single trace
     * of the whole batch whatever the assignment. */
    const int64_t *gid_blocks;
    int64_t gid_block_rays;
    const wgrt_debug_opts *debug;   /* NULL in production (include/wgrt_debug.h) */
    /* ABI 5.  Single traces (num_iter <= 1) with workgroups == 0: the persistent grid is
     * ceil(grid_sqrt_k * sqrt(work items)) workgroups, at most the resident grid (a single trace
     * ends with the drain of its longest ray chains, which run faster on a less crowded chip;
     * DESIGN.md §5.4).  0 = the default 6.5; a negative value = the resident grid. */
    double grid_sqrt_k;
} wgrt_launch_opts;

/* One launch of either bounce kernel with launch options (everything else as
 * wgrt_trace_fullcolor / wgrt_trace_single). */
wgrt_status wgrt_trace_opts(const wgrt_scene *scene, const wgrt_rays *rays, int64_t n_rays, int64_t gid_offset,
                            uint32_t *rng_states, float *matrix_EB, wgrt_trace_stats *stats,
                            uint32_t *per_ray_bounces, void *stream, const wgrt_launch_opts *opts);

/* Pre-allocates the launch scratch the Jones-vector variants (7-9) use on `stream` for
 * launches of up to n_rays rays x num_iter chained traces (work-queue heads, replay list,
 * out-coupling queue, fused-launch hand-off words), so that no later launch within those
 * sizes allocates or synchronises.  Optional: a launch grows the scratch itself.  Not part
 * of the reference (its launches allocate nothing on the device). */
wgrt_status wgrt_scene_reserve(const wgrt_scene *scene, int64_t n_rays, int num_iter, void *stream);

/* Device-side ray setup (replaces the host loop MAIN:59-115 and the seeding at MAIN:158):
 * fills FoV x wavelength blocks [block_lo, block_hi) of the batch -- block b =
 * (ii * ny + jj) * n_lambdas + k, rays [b * R, (b + 1) * R) -- into DEVICE columns of
 * (block_hi - block_lo) * R floats, i.e. one rank's shard at local index 0:
 *   x, y = points[r] (first R/2 rays, TE: te 1, tm 0) / points[r - R/2] (TM: te 0, tm 1),
 *   m = ii, n = jj, lmd_num = lambdas[k] (HOST int32[n_lambdas], n_lambdas <= 8;
 *   MAIN uses 0..2), gap_x = gap_y = pol = azi = delta_phase = 0.
 * points: DEVICE float64 [R / 2, 2] (generate_points_in_polygon, GRTF:12-23), rounded to
 * float32 as numpy assignment does.  Odd R: the last ray of each block is all-zero, as in
 * MAIN.  rng_states (optional, DEVICE uint32) = 0x9E3779B9 * (gid + 1) with global gid =
 * block_lo * R + i.  Any column may be NULL (not written).  Asynchronous on stream. */
wgrt_status wgrt_rays_init(const double *points, int64_t rays_per_fov, int32_t nx, int32_t ny,
                           const int32_t *lambdas, int32_t n_lambdas, int64_t block_lo, int64_t block_hi,
                           const wgrt_ray_columns *out, uint32_t *rng_states, void *stream);

/* Multi-GPU eyebox collection (the strong-scaling gather of distributed.EyeboxGather; the reference
 * runs one GPU and accumulates matrix_EB in place, MAIN:167-178).  Each rank traces its own FoV x
 * wavelength blocks, so it owns whole (lambda, n, m) slabs of 80 x 120 floats of matrix_EB, plus -- by
 * the compiled-numba aliasing of an out-coupling exactly on the eyebox's top edge (GRTF:154-165) -- the
 * first WGRT_EB_SPILL floats of the slab after an owned one.  A rank's payload is one flat float
 * buffer of wgrt_eyebox_payload_floats(nb) floats: nb slab rows of WGRT_EB_SLAB floats, then nb spill
 * rows of WGRT_EB_SPILL floats (16-B aligned: the spill part is padded to 4 floats).
 *   pack:     row j (j < n) <- slab slabs[j]; spill row j <- the first WGRT_EB_SPILL floats of slab
 *             next[j], times spill_mask[j] (0 or 1); rows n .. nb-1 untouched.
 *   assemble: eb slab dst[r * nb + j] <- slab row j of rank r's payload (recv + r * payload floats),
 *             for every dst >= 0; then the spill rows with spill_dst[r * nb + j] >= 0 are ADDED to the
 *             first WGRT_EB_SPILL floats of that slab (after every copy).  Slabs no dst names are left
 *             as they are.
 * Every pointer is DEVICE memory (slabs / next / dst / spill_dst int64, spill_mask float); both
 * launch on `stream` (its device) and are asynchronous.  Not part of the reference. */
#define WGRT_EB_SLAB 9600
#define WGRT_EB_SPILL 121
int64_t wgrt_eyebox_payload_floats(int64_t nb);
wgrt_status wgrt_eyebox_pack(const float *eb, int64_t n_slabs, const int64_t *slabs, const int64_t *next,
                             const float *spill_mask, int64_t n, int64_t nb, float *payload, void *stream);
wgrt_status wgrt_eyebox_assemble(float *eb, int64_t n_slabs, const float *recv, int32_t world, int64_t nb,
                                 const int64_t *dst, const int64_t *spill_dst, void *stream);

/* ABI 8.  Per-slab reduction of the eyebox grid (replaces the host passes of MAIN:186-198 / EVAL:66-109).
 * For row j < n, slab s = slabs ? slabs[j] : j of eb [n_slabs, 80, 120]:
 *   out[j * W + 0]                 = sum of the slab
 *   out[j * W + 1 + iy * npx + ix] = sum over (r, c) in [0, ms)^2 of mask[r * ms + c] * eb[s, iy*step_y + r, ix*step_x + c]
 * with npy = (80 - ms) / step_y + 1, npx = (120 - ms) / step_x + 1, W = 1 + npy * npx
 * (ms = 30, steps 8 / 12: npy = 7, npx = 8, W = 57 -- the reference's eye positions).
 * Accumulated in float64 in a fixed order (no float atomics): the same input gives the same bits on every
 * run, and an integer-valued grid gives the exact integers.  Rows whose s is outside [0, n_slabs) are
 * zero-filled.  eb (16-B aligned), slabs (int64, or NULL), mask (float32 [ms * ms]) and out (float64 [n * W])
 * are DEVICE pointers; asynchronous on stream, on the stream's device (as wgrt_eyebox_pack).  1 <= ms <= 80,
 * step_y, step_x >= 1, n <= 2^31 - 1, else WGRT_ERR_INVALID_ARGUMENT.  n == 0 is WGRT_OK without a launch.
 * Not part of the reference. */
wgrt_status wgrt_eyebox_window_sums(const float *eb, int64_t n_slabs, const int64_t *slabs, int64_t n,
                                    const float *mask, int32_t ms, int32_t step_y, int32_t step_x,
                                    double *out, void *stream);

/* ABI 9.  Evaluation of the window-sum table on the device (replaces the host colour math of EVAL:112-163):
 * the three merit figures and, optionally, the evaluated image, from what wgrt_eyebox_window_sums wrote.
 *   sums     float64 [3 * n_fov, 1 + n_pos], rows ordered (lambda, FoV) -- the whole three-wavelength grid's
 *            table; column 0 (the slab total) is ignored;
 *   divisor  perceive = sum / divisor (R * num_iter, MAIN:197); finite and > 0;
 *   wl       HOST float64 [3]: inv(M_SENSOR) . (1, 1, 1), the per-wavelength weights of the white image
 *            (EVAL:47-52, 112-118); lab_d65: HOST float64 [3], the CIELAB reference white (EVAL:53-57);
 *   out      float64 [3 + n_pos]: delta_e, U_fov, U_EB (EVAL:160-163), then U_EB[i, j] of every eye position
 *            before the final min / max (0 for a position with a dark pixel, EVAL:150-157);
 *   image    float32, or NULL for none.  image_pos = -1: every position, [n_fov, 3, n_pos] (the reference's
 *            output_image [NY, NX, 3, npy, npx]); image_pos = p >= 0: position p alone, [n_fov, 3];
 *   workspace  wgrt_eyebox_evaluate_workspace_bytes(n_fov, n_pos) bytes (-1 for a shape the call rejects),
 *            8-B aligned, overwritten.
 * Each pixel (FoV, position) is evaluated as AR_system_evaluation_functions.evaluation_from_perceive does, operation
 * by operation (csrc/wgrt_colour.h): float64 colour side, float32 HSV normalisation.  No float atomics; every sum
 * is taken in an order fixed by (n_fov, n_pos), so the same input gives the same bits on every run.  sums, out,
 * image and workspace are DEVICE pointers; the call allocates nothing and is asynchronous on stream, on the
 * stream's device (as wgrt_eyebox_window_sums, whose table may be fed on the same stream without a sync).
 * n_fov >= 1, 1 <= n_pos <= 2^20, 3 * n_fov * (1 + n_pos) <= 2^31 - 1 (the index arithmetic's limit: a 17 GB
 * table), -1 <= image_pos < n_pos, sums / out / workspace 8-B and image 4-B aligned, else
 * WGRT_ERR_INVALID_ARGUMENT.  Not part of the reference. */
int64_t wgrt_eyebox_evaluate_workspace_bytes(int64_t n_fov, int64_t n_pos);
wgrt_status wgrt_eyebox_evaluate(const double *sums, int64_t n_fov, int64_t n_pos, double divisor, const double *wl,
                                 const double *lab_d65, double *out, float *image, int64_t image_pos,
                                 void *workspace, void *stream);

/* Host-only replica of wgrt_eyebox_evaluate (no GPU needed; test hook): the same arguments with HOST pointers,
 * the same pixel function and the same order of every sum, on the CPU.  Differs from the device only by the
 * host libm's last places in pow / cbrt / hypot / atan2 / sin / cos / exp. */
wgrt_status wgrt_eyebox_evaluate_host(const double *sums, int64_t n_fov, int64_t n_pos, double divisor,
                                      const double *wl, const double *lab_d65, double *out, float *image,
                                      int64_t image_pos, void *workspace);

/* The window-table sink (new symbols within ABI 9: no existing struct or signature changed, so
 * WGRT_ABI_VERSION stays 9; a caller finds out whether a library has them by looking the symbols up).
 *
 * What anyone reads from an 80 x 120 slab of matrix_EB is its total and its pupil-window sums, the
 * [n_slabs, W] table of wgrt_eyebox_window_sums.  wgrt_trace_windows counts every out-coupling straight into
 * that table, so a job that only evaluates never allocates the grid (38.4 KB per slab against 8 W bytes).
 * An out-coupling into flat grid offset off -- computed as for the grid, aliasing included (GRTF:164): the
 * negative-index wrap, ix == 120 into the next row, iy == 80 into the next slab, dropped outside the
 * buffer -- lies in slab s = off / 9600, row r = off % 9600 / 120, column c = off % 120, and adds 1 to
 * table[s, 0] and to table[s, 1 + wy * npx + wx] of every window (wy, wx) with wy * step_y <= r <
 * wy * step_y + ms, wx * step_x <= c < wx * step_x + ms and the tap mask[r - wy * step_y, c - wx * step_x]
 * set (npy, npx, W as in wgrt_eyebox_window_sums).  The counts are integers and the window sums linear in
 * the grid, so the table a trace leaves equals wgrt_eyebox_window_sums of the grid the same trace would have
 * left, bit for bit, and feeds wgrt_eyebox_evaluate unchanged.
 *
 * A plan is the mask and the steps, on one device.  mask is a HOST float32 [ms * ms]; 1 <= ms <= 80, steps
 * >= 1, and every tap exactly 0.0f or 1.0f (the sink adds exactly 1.0 per tap, so the sums are exact integers
 * in any order; wgrt_eyebox_window_sums keeps serving other masks from a grid), else
 * WGRT_ERR_INVALID_ARGUMENT with the reason in wgrt_last_error.  The device holds the mask as one bit per tap. */
typedef struct wgrt_window_plan wgrt_window_plan;   /* opaque, device-resident */
wgrt_status wgrt_window_plan_create(const float *mask, int32_t ms, int32_t step_y, int32_t step_x, int device,
                                    wgrt_window_plan **out);
wgrt_status wgrt_window_plan_destroy(wgrt_window_plan *plan);
int64_t wgrt_window_plan_width(const wgrt_window_plan *plan);   /* W = 1 + npy * npx; -1 for NULL */

/* wgrt_trace_opts with the window table as a second sink.  table: DEVICE float64 [n_slabs, W], n_slabs =
 * num_lmd * ny * nx slabs in matrix_EB's order, accumulated into by f64 atomic adds and never zeroed; plan: a
 * plan on the scene's device.  matrix_EB may be NULL (the table alone); with both, the same hits are written
 * to both.  table == NULL: exactly wgrt_trace_opts (matrix_EB required, plan ignored).  Every kernel,
 * variant and option of wgrt_trace_opts; wgrt_trace_stats.eyebox_hits counts the same hits; the call
 * allocates nothing more and is asynchronous on stream.  Not part of the reference. */
wgrt_status wgrt_trace_windows(const wgrt_scene *scene, const wgrt_rays *rays, int64_t n_rays, int64_t gid_offset,
                               uint32_t *rng_states, float *matrix_EB, wgrt_trace_stats *stats,
                               uint32_t *per_ray_bounces, void *stream, const wgrt_launch_opts *opts,
                               const wgrt_window_plan *plan, double *table);

/* Chained single launches (new symbols within ABI 9, looked up by name).  A chain is a run of single traces
 * (num_iter = 1 each) of one batch, every trace starting from the RNG states the previous one left -- what the
 * same number of wgrt_trace_windows calls would compute, bit for bit (rng_states, matrix_EB / table, stats) --
 * issued so that one launch's drain overlaps the next launch's bulk: the steps alternate between the caller's
 * stream and one library-owned non-blocking side stream, and step k + 1 takes ray i's state from the granule
 * step k's trace of ray i published (the fused launches' per-ray hand-off, across the kernel boundary).
 *   begin  takes the arguments of wgrt_trace_windows (no per_ray_bounces; plan / table may be NULL), copies
 *          them (opts and its debug record included; the device buffers must stay alive until end) and sizes
 *          both sides' launch scratch, so that no step allocates or synchronises;
 *   step   enqueues one trace: its own kernel launch, with the arguments a plain launch would get;
 *   end    joins the side stream into the caller's, leaves rng_states at the last step's states and frees the
 *          chain.  After it returns, `stream` is ordered after every step, as if they had been plain launches.
 * Between begin and end the caller enqueues nothing on `stream` that touches rng_states, matrix_EB, the table
 * or stats, starts no other chain or trace of the scene on it, and begins no graph capture on it while steps are
 * in flight (a chain looks at the stream's capture state at begin and whenever it opens a segment).  Steps that cannot be chained run as plain
 * launches on `stream`, after a join: a launch that still learns the scene's tile table, variant 1, a
 * single-wavelength scene, num_iter > 1, chunk_order, a debug timeline, a stream under capture, and a batch so
 * large that one launch's grid is the kernel's resident grid (it fills the chip alone: nothing to overlap)
 * (wgrt_debug_chain_plan states the rule).  wgrt_trace_stats.handoff_giveups counts hand-offs given up
 * (a bug: the results of the chain are then invalid), as for fused launches. */
typedef struct wgrt_chain wgrt_chain;
wgrt_status wgrt_chain_begin(const wgrt_scene *scene, const wgrt_rays *rays, int64_t n_rays, int64_t gid_offset,
                             uint32_t *rng_states, float *matrix_EB, wgrt_trace_stats *stats, void *stream,
                             const wgrt_launch_opts *opts, const wgrt_window_plan *plan, double *table,
                             wgrt_chain **out);
wgrt_status wgrt_chain_step(wgrt_chain *chain);
wgrt_status wgrt_chain_end(wgrt_chain *chain);

/* A gathering chain: opt-in, for a caller that calls its steps back to back and reads nothing before end (new
 * symbol within ABI 9, looked up by name).  A chain fixes every argument at begin, so steps not yet launched are a
 * count, and a count of k steps is a fused launch (num_iter = k) -- the launch shape with one drain per launch, not
 * one per step.  Called between begin and the first step, it changes how that chain's steps are issued:
 *   - a step called when `stream` has finished everything the chain issued before is launched at once, as the
 *     plain launch it is (hold != 0: it is counted like the others);
 *   - a step called while the stream is still busy is counted, not enqueued; the count goes out as ONE fused launch
 *     when a later step finds the stream idle, when it reaches the cap, before a step that must run as a plain
 *     launch, and at end.  "Finds idle" is an event query: no call waits for the device.
 * What the caller gives up against a plain chain, and must be able to afford:
 *   - a counted step's work starts no earlier than a later step or end call, however long the caller takes to make
 *     it: a caller that does host work between steps leaves the GPU idle with steps pending, and an event it
 *     records on `stream` after a step does not follow that step's work.  Only end orders the stream after every
 *     step.
 *   - memory: this call grows the stream's launch scratch to the cap (24 bytes per ray and step of the cap), and the
 *     stream keeps it.  The cap is max_steps (2 .. 64; 0: as many as 1 GiB of scratch allows, at most 64, at least
 *     2); when the allocation fails the cap is halved until it succeeds, and WGRT_ERR_HIP is returned only when
 *     a cap of 2 fails too.  The call may synchronise the stream.
 *   - wgrt_trace_stats.replayed: a fused launch counts a ray it abandons once and finishes its remaining traces
 *     on the exact lane, so on LUTs and bounds that abandon rays the count is at most the plain launches' per-trace
 *     count.  rng_states, matrix_EB / table and every other counter stay bit for bit what plain launches leave.
 * Steps that a plain chain runs as plain launches still do (the rule above), behind what has been gathered.  On a
 * chain that stays serial for one of those reasons the call succeeds and changes nothing.  After the first step it
 * is WGRT_ERR_INVALID_ARGUMENT.  wgrt_debug_chain_report (wgrt_debug.h) says what a chain has launched. */
wgrt_status wgrt_chain_gather(wgrt_chain *chain, int max_steps, int hold);

/* Where every ray ends: per-ray fates and the per-tile census (new symbols within ABI 9, looked up by name).
 *
 * A ray's fate is the code 10 * region + reason of the place its trace ended (csrc/wgrt_fate.h states it once;
 * it is the CPU oracle's code): region the state R0..R5 the ray was in, 9 for the in-coupling event; reason
 *   1 left eff_reg1 (left the plate)      2 Monte-Carlo loss (the draw took no branch)
 *   3 out-coupled inside the FoV's eyebox rectangle   4 out-coupled outside it
 *   5 missed every out-coupler slice in R5            6 the in-coupler's second order left the in-coupler
 *   7 ran out of bounces (range(100000) exhausted).
 * 27 codes can occur: 92 96; 01 02 06 07; 11 12 16 17; 21 22 27; 31 32 37; 41 42 43 44 47; 51 52 53 54 55 57.
 * 0 means "not traced" (an m / n / lmd_num outside the scene).  An out-coupling whose aliased grid offset is
 * dropped (GRTF:164) is still reason 3, so per tile the reason-3 count is the number of rays of THAT tile that
 * reached its eyebox, while matrix_EB counts a hit in the slab its aliased offset falls into.
 *
 * wgrt_trace_fate is wgrt_trace_windows plus fate, a DEVICE uint8 [n_rays]: after the launch fate[i], i < n_rays,
 * has been written exactly once, by whichever lane finished ray i's trace (the Jones-vector lane, or the exact
 * lane for variant 1 and for a replayed ray); both give the same code.  fate == NULL is exactly
 * wgrt_trace_windows.  matrix_EB, rng_states, the window table and stats come out bit-identical with and without
 * fate.  fate != NULL with opts->num_iter > 1 is WGRT_ERR_INVALID_ARGUMENT (a fused launch's retire sites
 * publish hand-off granules; trace the iterations one call each), and wgrt_chain_begin takes no fates.  What a
 * fate launch routes around: it runs the fate-storing kernel instantiation, which has no learning and no timeline
 * twin, so a fate launch never learns the scene's tile table (the automatic issue order learns from the next plain
 * launch instead; results do not depend on the order), and fate with wgrt_debug_opts.timeline is
 * WGRT_ERR_UNSUPPORTED.  A launch without fate runs the kernels it ran before this entry point existed. */
#define WGRT_FATE_COLS 56      /* column = 8 * min(code / 10, 6) + code % 10; column 0 reserved */
wgrt_status wgrt_trace_fate(const wgrt_scene *scene, const wgrt_rays *rays, int64_t n_rays, int64_t gid_offset,
                            uint32_t *rng_states, float *matrix_EB, wgrt_trace_stats *stats,
                            uint32_t *per_ray_bounces, void *stream, const wgrt_launch_opts *opts,
                            const wgrt_window_plan *plan, double *table, uint8_t *fate);

/* The census: ray i with valid code c and tile s = (l * ny + n) * nx + m (matrix_EB's slab order; m, n, lmd_num
 * the batch's DEVICE columns, lmd_num == NULL: l = 0) adds 1 to table[s, column(c)], table a DEVICE int64
 * [num_lmd * ny * nx, WGRT_FATE_COLS] that is ADDED to and never zeroed.  A ray is counted nowhere if its code is
 * 0 or none of the codes above, or if its tile lies outside the scene; nothing outside the table is touched.
 * Integer atomics: the table is the same on every run and for any ray order.  Asynchronous on stream, allocates
 * nothing; n_rays == 0 is WGRT_OK without a launch. */
wgrt_status wgrt_fate_census(const uint8_t *fate, const float *m, const float *n, const float *lmd_num,
                             int64_t n_rays, int32_t nx, int32_t ny, int32_t num_lmd, int64_t *table, void *stream);
/* Host-only twins (no GPU needed): the same census over HOST pointers through the same validity rule and column
 * function; the column of a code (-1 for a code that is not one of the 27); a reason's name (1..7, else NULL). */
wgrt_status wgrt_fate_census_host(const uint8_t *fate, const float *m, const float *n, const float *lmd_num,
                                  int64_t n_rays, int32_t nx, int32_t ny, int32_t num_lmd, int64_t *table);
int32_t wgrt_fate_col(int code);
int32_t wgrt_fate_cols(void);   /* WGRT_FATE_COLS of the library */
const char *wgrt_fate_reason_name(int reason);

/* Monte-Carlo error bars: replica window tables and their fold (new symbols within ABI 9, looked up by name).
 *
 * wgrt_trace_replicas is wgrt_trace_windows plus replicas = B: table becomes a DEVICE float64 [B, n_slabs, W]
 * (B copies of the table of wgrt_trace_windows, one after the other), ADDED to and never zeroed, and an
 * out-coupling of the ray with global id g -- gid_offset + i, or the id opts->gid_blocks gives ray i -- counts into
 * copy g % B, through the membership rule above: the slab still comes from the aliased offset, and an offset
 * outside the buffer is still dropped.  The counts are integers, so the B copies add up, bit for bit, to the table
 * wgrt_trace_windows leaves; with matrix_EB also given the grid gets the same hits as ever; rng_states and stats
 * do not depend on replicas.  Because the replica is the global id's, the tables of the shards of one batch add up
 * to the whole batch's tables.
 *   replicas 0 or 1     exactly wgrt_trace_windows (table [n_slabs, W], or NULL);
 *   2 <= replicas <= WGRT_MAX_REPLICAS   table required, else WGRT_ERR_INVALID_ARGUMENT;
 *   anything else       WGRT_ERR_INVALID_ARGUMENT.
 * A replica launch is a single launch, as a fate launch is: opts->num_iter > 1 is WGRT_ERR_INVALID_ARGUMENT (trace
 * the iterations one call each), wgrt_chain_begin takes no replicas, and there is no entry point that takes both
 * replicas and fates.  It runs kernel instantiations of its own (variants 7 / 9), which have no learning and no
 * timeline twin: a replica launch never learns the scene's tile table (the next plain launch does; results do not
 * depend on the order), and replicas with wgrt_debug_opts.timeline is WGRT_ERR_UNSUPPORTED.  Those kernels carry
 * the replica in the top byte of their out-coupling queue entry, so variants 7 / 9 refuse a scene of 2^24 tiles or
 * more with WGRT_ERR_UNSUPPORTED (variant 1 has no such limit).  The call allocates nothing and is asynchronous on
 * stream.  A launch without replicas runs the kernels it ran before this entry point existed. */
#define WGRT_MAX_REPLICAS 64
wgrt_status wgrt_trace_replicas(const wgrt_scene *scene, const wgrt_rays *rays, int64_t n_rays, int64_t gid_offset,
                                uint32_t *rng_states, float *matrix_EB, wgrt_trace_stats *stats,
                                uint32_t *per_ray_bounces, void *stream, const wgrt_launch_opts *opts,
                                const wgrt_window_plan *plan, double *table, int replicas);

/* The fold: from reps, DEVICE float64 [B, n] (n = n_slabs * W entries per replica), out, DEVICE float64
 * [1 + B, n]:  out[0] = sum over b of reps[b], added in ascending b from 0.0;  out[1 + b] = out[0] - reps[b], the
 * leave-one-out tables of the delete-a-group jackknife.  One thread per entry pair, a fixed order and no atomics:
 * the same input gives the same bits, and integer counts come out as exact integers.  Every row of out is a table
 * wgrt_eyebox_evaluate takes unchanged: row 0 with the divisor rays-per-tile * launches, a leave-one-out row with
 * that times (B - 1) / B.  2 <= B <= WGRT_MAX_REPLICAS and n >= 0, else WGRT_ERR_INVALID_ARGUMENT; n == 0 is
 * WGRT_OK without a launch; reps and out must not overlap.  Asynchronous on stream, allocates nothing.  The _host
 * twin is the same loop over HOST pointers (no GPU needed). */
wgrt_status wgrt_window_replicas_fold(const double *reps, int32_t B, int64_t n, double *out, void *stream);
wgrt_status wgrt_window_replicas_fold_host(const double *reps, int32_t B, int64_t n, double *out);

/* The expected-value (collision) estimator of the eyebox (new symbols within ABI 9, looked up by name).
 *
 * wgrt_trace_windows counts a ray when its last draw out-couples it inside its FoV's eyebox rectangle.
 * wgrt_trace_expected makes the same walk -- the same draws and branches, so rng_states, per_ray_bounces and every
 * field of stats come out bit-identical to wgrt_trace_windows' (eyebox_hits keeps counting the walk's analog hits)
 * -- but scores every out-coupler interaction (R4 / R5) inside that rectangle: it adds the probability q that the
 * interaction's draw out-couples the ray to table[s, 0] and to every window holding the bin under the ray, through
 * the membership rule above (the aliased offset gives the slab, an offset outside the buffer is dropped).  The
 * out-coupling itself adds nothing more than its interaction's q.  With e1, e2, e3 the interaction's efficiencies,
 * en_k = ener * e_k and t the scene's threshold (0 full colour, 1e-15 one wavelength), the weight is the length of the
 * set of draws in [0, 1] for which the reference's if / elif / elif chain takes the out-coupling branch:
 *     w = 0 if !(en3 > t);  lo = en2 > t ? e1 + e2 : en1 > t ? e1 : 0;  w = max(0, min(e1 + e2 + e3, 1) - min(lo, 1)),
 * and q = rint(w * 2^32) * 2^-32 (ties to even; 1.0 for w == 1; q == 0 adds nothing).  Every table entry has the
 * expectation wgrt_trace_windows' has.  Sums of multiples of 2^-32 are exact in float64 while an entry stays below
 * 2^21: below that the table is the same bits on every run and for every work split, and shards and replicas add
 * up exactly.  The efficiencies are the exact lane's (variant 1, replays) or the Jones lane's double-precision
 * evaluation (variants 7 / 9), which differ from the reference's by far less than 2^-32: a q may differ from the
 * reference arithmetic's by one quantum.
 *   table      required: DEVICE float64 [n_slabs, W], or [B, n_slabs, W] for 2 <= replicas = B <= WGRT_MAX_REPLICAS,
 *              the ray with global id g scoring into copy g % B as in wgrt_trace_replicas; ADDED to, never zeroed;
 *   replicas   0 or 1: the one table; below 0 or above WGRT_MAX_REPLICAS: WGRT_ERR_INVALID_ARGUMENT.
 * There is no matrix_EB: a float32 grid cannot hold the fixed-point sums.  An expected-value launch is a single
 * launch, as fate and replica launches are: opts->num_iter > 1 is WGRT_ERR_INVALID_ARGUMENT, wgrt_chain_begin takes
 * none, no entry point combines it with fates, wgrt_debug_opts.timeline is WGRT_ERR_UNSUPPORTED, it never learns
 * the scene's tile table, and variants 7 / 9 refuse a scene of 2^24 tiles or more with WGRT_ERR_UNSUPPORTED (the
 * visit's entry carries the replica above the tile index).  A ray the Jones lane abandons is re-traced by the exact
 * lane past the visits already scored, so none is scored twice.  The call allocates nothing and is asynchronous on
 * stream.  A launch through any other entry point runs the kernels it ran before this one existed. */
wgrt_status wgrt_trace_expected(const wgrt_scene *scene, const wgrt_rays *rays, int64_t n_rays, int64_t gid_offset,
                                uint32_t *rng_states, wgrt_trace_stats *stats, uint32_t *per_ray_bounces, void *stream,
                                const wgrt_launch_opts *opts, const wgrt_window_plan *plan, double *table, int replicas);
/* Host-only (no GPU needed): q of the rule above, through the code the kernels run (csrc/wgrt_expected.h). */
double wgrt_expected_weight_host(double e1, double e2, double e3, double en1, double en2, double en3, double threshold);

/* Where on the plate: interaction and out-coupling footprint maps (new symbols within ABI 9, looked up by name).
 *
 * wgrt_trace_footprint is wgrt_trace_windows that also counts, per wavelength, where on the plate the rays interact,
 * are lost and leave: map is DEVICE int64 [num_lmd, WGRT_FOOTPRINT_CHANNELS, ny_cells, nx_cells], ADDED to, never
 * zeroed.  The plan is passed by value; a point (x, y) counts into the cell
 *     ix = (int64_t)floor((x - x0) / cell_x),   iy = (int64_t)floor((y - y0) / cell_y)
 * at the flat offset ((l * 9 + c) * ny_cells + iy) * nx_cells + ix, and is dropped when ix is outside [0, nx_cells),
 * iy outside [0, ny_cells) or a coordinate is not finite.  The position is always the ray's at the draw, before the
 * taken branch moves it.  Channels 0..5: every Monte-Carlo draw of the bounce loop in state R0..R5 (4 after the
 * R3 -> R4 switch) -- exactly the draws wgrt_trace_stats.interactions counts; the in-coupling event is not counted.
 * Channel 6: the draws that took no branch (fate reason 2).  Channel 7 / 8: the draws that out-coupled the ray inside /
 * outside its FoV's eyebox rectangle (reasons 3 / 4: the rectangle test, not the aliased store).  The counts are
 * integers: the map is the same bits on every run and for every work split, and the maps of shards add up exactly.
 *   fp    cell sizes > 0 and finite, a finite origin, 1 <= nx_cells, ny_cells <= 4096, else WGRT_ERR_INVALID_ARGUMENT;
 *   map   NULL: the call is exactly wgrt_trace_windows (fp is then not looked at).
 * With a map, rng_states, matrix_EB, the window table, per_ray_bounces and every field of stats come out bit-identical
 * to the launch without it.  A footprint launch is a single launch, as fate launches are: opts->num_iter > 1 is
 * WGRT_ERR_INVALID_ARGUMENT, wgrt_chain_begin takes none, no entry point combines it with fates, replicas or the
 * expected-value estimator, wgrt_debug_opts.timeline is WGRT_ERR_UNSUPPORTED, and it never learns the scene's tile
 * table.  A ray the Jones lane abandons is re-traced by the exact lane past the draws already counted, so none is
 * counted twice.  The call allocates nothing beyond the stream's launch scratch (wgrt_scene_reserve) and is
 * asynchronous on stream.  A launch through any other entry point runs the kernels it ran before this one existed. */
#define WGRT_FOOTPRINT_CHANNELS 9
typedef struct wgrt_footprint_plan {
    double x0, y0, cell_x, cell_y;
    int32_t nx_cells, ny_cells;
} wgrt_footprint_plan;
wgrt_status wgrt_trace_footprint(const wgrt_scene *scene, const wgrt_rays *rays, int64_t n_rays, int64_t gid_offset,
                                 uint32_t *rng_states, float *matrix_EB, wgrt_trace_stats *stats,
                                 uint32_t *per_ray_bounces, void *stream, const wgrt_launch_opts *opts,
                                 const wgrt_window_plan *plan, double *table, const wgrt_footprint_plan *fp,
                                 int64_t *map);
/* Host-only (no GPU needed) through the same rule (csrc/wgrt_footprint.h): _validate is wgrt_trace_footprint's plan
 * check alone; _bin_host ADDS the n points (HOST x, y float64; l, channel int32) to the HOST map of num_lmd
 * wavelengths: a point whose l is outside [0, num_lmd) or whose channel is outside [0, 9) is dropped like one
 * outside the plan; _channel_name names channel c ("R0" .. "R5", "lost", "eyebox", "beside_eyebox"; NULL otherwise). */
wgrt_status wgrt_footprint_plan_validate(const wgrt_footprint_plan *fp);
wgrt_status wgrt_footprint_bin_host(const wgrt_footprint_plan *fp, const double *x, const double *y, const int32_t *l,
                                    const int32_t *channel, int64_t n, int32_t num_lmd, int64_t *map);
const char *wgrt_footprint_channel_name(int c);

/* Keep every out-coupling: a hit list, and eyebox grids of any resolution from it (new symbols within ABI 9, looked up
 * by name).
 *
 * wgrt_trace_hits is wgrt_trace_windows that also appends one record per out-coupling of the launch -- a draw that
 * took the out-coupling branch (fate reasons 3 and 4), inside its FoV's eyebox rectangle or beside it, whether its
 * aliased grid offset was stored or dropped -- to hits, DEVICE wgrt_hit [capacity], 16-byte aligned.
 *   count     DEVICE uint64[1], ADDED to, never zeroed: it grows by the launch's out-couplings.  A record whose reserved
 *             index (the counter's value when it was reserved) is below capacity is stored at hits[index]; the others
 *             are counted and not stored.  Nothing at or beyond hits + capacity is written.  Several launches may
 *             append to one list; the tag tells them apart.  The order of the records is unspecified; (tag, gid) is
 *             unique per record, because a trace out-couples at most once.
 *   hits      NULL: the call is exactly wgrt_trace_windows (capacity, count and tag are not looked at).  Otherwise
 *             count != NULL, capacity >= 0 (0 only counts), tag <= 65535 and an aligned hits, else
 *             WGRT_ERR_INVALID_ARGUMENT.
 * With a list, rng_states, matrix_EB, the window table, per_ray_bounces and every field of stats come out bit-identical
 * to the launch without it.  A hits launch is a single launch, as fate launches are: opts->num_iter > 1 is
 * WGRT_ERR_INVALID_ARGUMENT, wgrt_chain_begin takes none, no entry point combines it with fates, replicas, the
 * expected-value estimator or footprints, wgrt_debug_opts.timeline is WGRT_ERR_UNSUPPORTED, and it never learns the
 * scene's tile table.  A ray the Jones lane abandons has appended nothing (a record is appended at the terminal
 * out-coupling only), so its re-trace on the exact lane appends its record exactly once.  The call allocates nothing
 * beyond the stream's launch scratch and is asynchronous on stream.  A launch through any other entry point runs the
 * kernels it ran before this one existed. */
typedef struct __attribute__((aligned(16))) wgrt_hit {   /* 32 bytes */
    double x, y;               /* the out-coupling position: the ray's position at its last draw */
    int64_t gid;               /* global ray id: gid_offset + i, or the id opts->gid_blocks gives ray i */
    uint32_t tile;             /* (lambda * nx + m) * ny + n */
    uint32_t flags;            /* bit 0: inside the FoV's eyebox rectangle (fate reason 3; clear: reason 4);
                                  bits 16..31: the call's tag; every other bit 0 */
} wgrt_hit;
wgrt_status wgrt_trace_hits(const wgrt_scene *scene, const wgrt_rays *rays, int64_t n_rays, int64_t gid_offset,
                            uint32_t *rng_states, float *matrix_EB, wgrt_trace_stats *stats, uint32_t *per_ray_bounces,
                            void *stream, const wgrt_launch_opts *opts, const wgrt_window_plan *plan, double *table,
                            wgrt_hit *hits, int64_t capacity, uint64_t *count, uint32_t tag);
int32_t wgrt_hit_bytes(void);   /* sizeof(wgrt_hit) of the library */
/* A list binned into an eyebox grid on the device: grid is DEVICE float32 [num_lmd, ny, nx, H, W], laid out as
 * matrix_EB with (80, 120) replaced by (H, W), ADDED to, never zeroed; hits DEVICE wgrt_hit [n].  Record k's tile gives
 * (l, m, n); a record whose tile is >= num_lmd * nx * ny is dropped.
 *   ranges == NULL  the range (xmin, xmax, ymin, ymax) is the scene's eff_reg_FOV_range[m, n], and the record counts
 *                   iff flag bit 0 is set.
 *   ranges != NULL  DEVICE float64 [NX, NY, 4] in eff_reg_FOV_range's layout; the record counts iff
 *                   xmin <= x <= xmax && ymin <= y <= ymax, the flag ignored: a beside-the-eyebox out-coupling gets
 *                   into a larger or moved eyebox without a re-trace.
 * The bin is the trace's own (csrc/wgrt_hits.h): dx = (xmax - xmin) / W, ix = (int64_t)floor((x - xmin) / dx), a
 * negative index wraps once, an index equal to the axis length aliases through the flat offset, and the offset is
 * guarded by 0 <= off < total -- so at ranges == NULL, H = 80, W = 120 the grid equals matrix_EB of the same launches
 * bit for bit.  1 <= H, W <= 4096 and at most 2^31 floats, else WGRT_ERR_INVALID_ARGUMENT; n == 0 is WGRT_OK without a
 * launch.  One thread per record, +1.0f atomics: counts are integers, so the grid is the same bits for any record
 * order while a bin stays below 2^24.  Asynchronous on stream.
 * _host is the twin over HOST pointers through the same header (no GPU needed): the scene is stated by nx, ny,
 * num_lmd and scene_ranges, HOST float64 [nx, ny, 4] (eff_reg_FOV_range). */
wgrt_status wgrt_hits_grid(const wgrt_scene *scene, const wgrt_hit *hits, int64_t n, const double *ranges, int32_t H,
                           int32_t W, float *grid, void *stream);
wgrt_status wgrt_hits_grid_host(int32_t nx, int32_t ny, int32_t num_lmd, const double *scene_ranges, const wgrt_hit *hits,
                                int64_t n, const double *ranges, int32_t H, int32_t W, float *grid);

/* Source what-ifs: a hit list re-weighted for K projector pupils, and counted per entry class (new symbols within ABI 9,
 * looked up by name; the rule is stated once in csrc/wgrt_sources.h).
 *
 * A ray's entry point and input polarisation are a pure function of its global id: with R rays per FoV x wavelength
 * block, ray gid has the block index r = gid mod R, starts at points[r mod (R / 2)] and is TE for r < R / 2, TM
 * otherwise (wgrt_rays_init).  Rays are independent, so a source that emits class r with relative radiance w[r] delivers
 * exactly the table in which every out-coupling deposits w[gid mod R] instead of 1.  A record with gid < 0 is dropped.
 *
 * wgrt_hits_source_counts: counts is DEVICE int64 [num_lmd, 2, R], 8-B aligned, ADDED to.  A record whose tile is below
 * num_lmd * nx * ny adds 1 to counts[l][0][gid mod R] when its flag bit 0 is set (inside its FoV's eyebox rectangle) and
 * to counts[l][1][gid mod R] when it is clear (beside it), l = tile / (nx * ny): the flag decides, not whether the
 * aliased grid offset was stored.  One thread per record, 64-bit integer atomics: the same bits for any record order.
 * R < 1, n < 0, a NULL or misaligned pointer are WGRT_ERR_INVALID_ARGUMENT; n == 0 is WGRT_OK without a launch.
 *
 * wgrt_hits_reweight_sources:
 *   weights  DEVICE float64 [K, R], 8-B aligned: source k emits class r with relative radiance weights[k][r].  Finite
 *            and 0 <= w <= 1024; the device entry point does not look (the host twin and the Python layer do): a
 *            weight outside gives a table without meaning, never a write out of bounds.
 *   out      DEVICE float64 [K, n_slabs, W], ADDED to: a record that counts -- flag bit 0 set, tile below
 *            num_lmd * nx * ny, gid >= 0 -- deposits q = rint(w * 2^32) * 2^-32, w = weights[k][gid mod R], into table k
 *            at the entries wgrt_trace_windows adds 1 to for that out-coupling: its bin is the trace's own (the scene's
 *            range, 80 x 120, the aliasing and the [0, total) guard of wgrt_hits_grid at ranges == NULL), its slab comes
 *            from the offset.  Sums on the 2^-32 grid are exact and order-free while an entry stays below 2^21, and a
 *            weight of 1 deposits exactly 1.0: a row of ones gives the launches' window table bit for bit.  q == 0
 *            deposits nothing.
 *   wsums    NULL, or DEVICE int64 [K, 2, num_lmd], 8-B aligned, ADDED to, as wgrt_visits_reweight_many keeps them:
 *            every depositing record adds rint(q * 2^32) to wsums[k][0][l] and rint(q * q * 2^32) to wsums[k][1][l].
 * A workgroup reads a record once for a chunk of 64 sources, a lane per source.  The call allocates and frees on `stream`
 * the quantised, transposed weights [R, 64 * ceil(K / 64)] (float64) and one chunk's deposits [n_slabs * W, 64], which a
 * second kernel adds into the chunk's tables.  A plan on another device than the scene, K < 1, R < 1, n < 0, a NULL or
 * misaligned pointer, more than 2^31 * 64 records or 65535 chunks are WGRT_ERR_INVALID_ARGUMENT.  n == 0 is WGRT_OK
 * without a launch.  Asynchronous on stream.
 * The _host twins run the same rule over HOST pointers (no GPU needed) and give the same bits: the scene is stated by
 * nx, ny, num_lmd and scene_ranges (HOST float64 [nx, ny, 4], eff_reg_FOV_range), the plan by its mask, as
 * wgrt_visits_reweight_many_host states them.  wgrt_hits_reweight_sources_host also refuses a weight that is not finite
 * or outside [0, 1024]. */
wgrt_status wgrt_hits_source_counts(const wgrt_scene *scene, const wgrt_hit *hits, int64_t n, int64_t R, int64_t *counts,
                                    void *stream);
wgrt_status wgrt_hits_source_counts_host(int32_t nx, int32_t ny, int32_t num_lmd, const wgrt_hit *hits, int64_t n,
                                         int64_t R, int64_t *counts);
wgrt_status wgrt_hits_reweight_sources(const wgrt_scene *scene, const wgrt_window_plan *plan, const wgrt_hit *hits,
                                       int64_t n, const double *weights, int64_t R, int32_t K, double *out,
                                       int64_t *wsums, void *stream);
wgrt_status wgrt_hits_reweight_sources_host(int32_t nx, int32_t ny, int32_t num_lmd, const double *scene_ranges,
                                            const float *mask, int32_t ms, int32_t step_y, int32_t step_x,
                                            const wgrt_hit *hits, int64_t n, const double *weights, int64_t R, int32_t K,
                                            double *out, int64_t *wsums);

/* Ray paths: every draw of selected rays as a record, and a path list reduced to a footprint map (new symbols within
 * ABI 9, looked up by name; the rule is stated once in csrc/wgrt_paths.h).
 *
 * wgrt_trace_paths is wgrt_trace_windows that also appends, for every selected ray, one record per Monte-Carlo draw of
 * the bounce loop -- exactly the draws wgrt_trace_stats.interactions and footprint channels 0..5 count; the
 * in-coupling event is not one -- at the ray's position before the taken branch moves it, draw k of the trace with
 * step = k (0-based); and, for a trace that ends by the loop-top eff_reg1 test or by an R5 miss (fate reasons 1, 5),
 * one more END record at the ray's position there, whose step is the number of draws the trace made.  A trace that
 * ends at the bounce cap (reason 7) or at the in-coupling event appends no end record.  A draw at which the
 * in-coupler's second order leaves the in-coupler (reason 6) is kind 0.  So (tag, gid, step) is unique per record, a
 * ray's records sorted by step are its polyline after the start point, and the number of draw records of a ray is its
 * interaction count.
 *   paths     DEVICE wgrt_path_vertex [capacity], 16-byte aligned.  NULL: the call is exactly wgrt_trace_windows
 *             (capacity, count, tag and select are not looked at).  Otherwise count != NULL, capacity >= 0 (0 only
 *             counts), tag <= 65535, else WGRT_ERR_INVALID_ARGUMENT; so is a scene of more than 256 wavelengths.
 *   count     DEVICE uint64[1], ADDED to, never zeroed.  A record whose reserved index is below capacity is stored at
 *             paths[index]; the others are counted and not stored.  Nothing at or beyond paths + capacity is written.
 *             The order of the records is unspecified: sort by (tag, gid, step).
 *   select    DEVICE uint8 [n_rays]: nonzero records the ray; NULL: every ray.  The walk is a pure function of the RNG
 *             states, so a first launch (wgrt_trace_fate on a copy of the states) can choose the rays of a second.
 * Every other output -- rng_states, matrix_EB, the window table, per_ray_bounces, every field of stats -- is the bytes
 * of the same launch through wgrt_trace_windows.  A paths launch is a single launch, as a hits launch is:
 * opts->num_iter > 1 is WGRT_ERR_INVALID_ARGUMENT, wgrt_chain_begin takes no list, no entry point combines it with
 * fates, replicas, the expected-value estimator, footprints or hit lists, wgrt_debug_opts.timeline is
 * WGRT_ERR_UNSUPPORTED, and it never learns the scene's tile table.  The Jones lane records a draw once its decision
 * is certified; a ray it abandons is re-traced on the exact lane, which passes over the draws already recorded and
 * appends the rest, the end record included, exactly once.  Asynchronous on stream.  A launch through any other entry
 * point runs the kernels it ran before this one existed. */
typedef struct __attribute__((aligned(16))) wgrt_path_vertex {   /* 32 bytes */
    double x, y;               /* the ray's position at the event (at a draw: before the taken branch moves it) */
    int64_t gid;               /* global ray id: gid_offset + i, or the id opts->gid_blocks gives ray i */
    uint32_t step;             /* ordinal of the record within the ray's trace */
    uint32_t flags;            /* bits 0..2: state R0..R5 (4 after the R3 -> R4 switch, as the fate code's region);
                                  bits 4..7: kind -- 0 draw, the trace goes on; 2 draw, Monte-Carlo loss; 3 / 4 draw,
                                  out-coupled inside / beside the FoV's eyebox rectangle; 1 end record, left eff_reg1;
                                  5 end record, R5 miss; bits 8..15: wavelength index; bits 16..31: the call's tag */
} wgrt_path_vertex;
wgrt_status wgrt_trace_paths(const wgrt_scene *scene, const wgrt_rays *rays, int64_t n_rays, int64_t gid_offset,
                             uint32_t *rng_states, float *matrix_EB, wgrt_trace_stats *stats, uint32_t *per_ray_bounces,
                             void *stream, const wgrt_launch_opts *opts, const wgrt_window_plan *plan, double *table,
                             wgrt_path_vertex *paths, int64_t capacity, uint64_t *count, uint32_t tag,
                             const uint8_t *select);
int32_t wgrt_path_vertex_bytes(void);   /* sizeof(wgrt_path_vertex) of the library */
/* A path list added into a footprint map on the device: map is DEVICE int64 [num_lmd, 9, fp->ny_cells, fp->nx_cells]
 * (wgrt_trace_footprint's), ADDED to, never zeroed; paths DEVICE wgrt_path_vertex [n], 16-byte aligned.  A draw record
 * counts into the channel of its state through the footprint's own cell rule, one of kind 2 / 3 / 4 also into channel
 * 6 / 7 / 8; end records and records whose wavelength index is >= num_lmd count nothing.  The list of launches with
 * select == NULL gives wgrt_trace_footprint's map of the same launches bit for bit; a fate-selected list gives the
 * conditional footprint.  Each workgroup takes a contiguous span of records and merges equal offsets in a per-wave
 * counter cache before they reach the map (wgrt_debug_set_footprint_aggregate(0): one atomic per count).  n == 0 is
 * WGRT_OK without a launch.  Asynchronous on stream (the current device's).
 * _host is the twin over HOST pointers through the same header (no GPU needed). */
wgrt_status wgrt_paths_footprint(const wgrt_path_vertex *paths, int64_t n, int32_t num_lmd,
                                 const wgrt_footprint_plan *fp, int64_t *map, void *stream);
wgrt_status wgrt_paths_footprint_host(const wgrt_path_vertex *paths, int64_t n, int32_t num_lmd,
                                      const wgrt_footprint_plan *fp, int64_t *map);

/* Branch visit counts: design sensitivities and what-if window tables from one ordinary trace (new symbols within ABI
 * 9, looked up by name; the channel table and the rule are stated once in csrc/wgrt_visits.h).
 *
 * A channel is (state, coupler slice, branch) -- one quadruple of Jones coefficients of one LUT; a scene has
 * C = wgrt_visit_channels(scene) = 6 + 4 n_fc_slices + 6 n_oc_slices of them: 0, 1 the in-coupling event's two
 * branches; 2, 3 R0's; 4, 5 R1's; 6 + 4 i + {0, 1} R2's and + {2, 3} R3's in fold-coupler slice i; B + 6 i + {0, 1, 2}
 * R4's and + {3, 4, 5} R5's in out-coupler slice i (B = 6 + 4 n_fc_slices; the third branch is the out-coupling).
 *
 * wgrt_trace_visits is wgrt_trace_windows that also counts the branches of counted rays.  Ray i is counted into row
 * slot ? slot[i] : i; a negative slot: the ray is not counted.  The device does not validate slots: every non-negative
 * one must be below n_rows.
 *   counts    DEVICE uint32 [n_rows, C].  Every Monte-Carlo draw of a counted ray that takes a branch, the in-coupling
 *             event's included, adds 1 to counts[row, c] of its channel; a draw that loses the ray adds nothing; a draw
 *             whose second in-coupler branch leaves the in-coupler (fate reason 6) still counts its b2.  ADDED to, never
 *             zeroed.  NULL: the call is exactly wgrt_trace_windows (slot, n_rows and ends are not looked at).
 *   ends      DEVICE wgrt_visit_end [n_rows], 16-byte aligned, required with counts.  Written once, as two 16-byte
 *             stores, when a counted ray's last draw out-couples: the position before the move (wgrt_hit's), the global
 *             id, the tile index, flags bit 1 (out-coupled) and bit 0 (inside the FoV's eyebox rectangle).  The row of a
 *             ray that did not out-couple is not touched: the caller zeroes the array.
 * Every other output -- rng_states, matrix_EB, the window table, per_ray_bounces, every field of stats -- is the bytes
 * of the same launch without counts.  A visits launch is a single launch, as hits and paths launches are:
 * opts->num_iter > 1 is WGRT_ERR_INVALID_ARGUMENT, wgrt_chain_begin takes none, no entry point combines it with fates,
 * replicas, the expected-value estimator, footprints, hit lists or path lists, wgrt_debug_opts.timeline is
 * WGRT_ERR_UNSUPPORTED, and it never learns the scene's tile table; n_rows < 0 and a misaligned ends are
 * WGRT_ERR_INVALID_ARGUMENT.  It works with opts->gid_blocks (rows are local) and with wgrt_trace_single scenes.  The
 * Jones lane counts a draw once its decision is certified; a ray it abandons is re-traced on the exact lane, which
 * passes over the draws already counted, so every branch is counted exactly once.  The counts are unsigned adds whose
 * result is not used.  Asynchronous on stream.  A launch through any other entry point runs the kernels it ran before
 * this one existed. */
typedef struct __attribute__((aligned(16))) wgrt_visit_end {   /* 32 bytes */
    double x, y;               /* the out-coupling position: the ray's position at its last draw */
    int64_t gid;               /* global ray id: gid_offset + i, or the id opts->gid_blocks gives ray i */
    uint32_t tile;             /* (lambda * nx + m) * ny + n */
    uint32_t flags;            /* bit 0: inside the FoV's eyebox rectangle (delivered); bit 1: out-coupled */
} wgrt_visit_end;
int32_t wgrt_visit_channels(const wgrt_scene *scene);   /* C; -1 for a NULL scene */
wgrt_status wgrt_trace_visits(const wgrt_scene *scene, const wgrt_rays *rays, int64_t n_rays, int64_t gid_offset,
                              uint32_t *rng_states, float *matrix_EB, wgrt_trace_stats *stats, uint32_t *per_ray_bounces,
                              void *stream, const wgrt_launch_opts *opts, const wgrt_window_plan *plan, double *table,
                              const int32_t *slot, int64_t n_rows, uint32_t *counts, wgrt_visit_end *ends);
/* The two reductions of a table of counted rays, on the scene's device.  A row is delivered when flag bit 0 of its end
 * record is set; its eyebox bin is computed from x, y and the tile exactly as the trace computes it, and a deposit goes
 * to column 0 of the bin's slab and to every window of `plan` that holds the bin -- the window sink's own membership
 * (an aliased offset gives the slab; an offset outside the buffer is dropped).
 *   _sensitivity  sens DEVICE float64 [C, n_slabs, W], ADDED to: for every delivered row and every c with
 *                 counts[row, c] > 0, the count is deposited into sens[c].  One wave per row, the lanes striding over the
 *                 channels.  Integer sums: exact and order-free below 2^53.  d table / d log s_c, binned as the table.
 *   _reweight     lnscale DEVICE float64 [C]; out DEVICE float64 [n_slabs, W], ADDED to: per delivered row
 *                 a = sum_c counts[row, c] * lnscale[c] (ascending c, one fma each), w = exp(a), and
 *                 q = rint(w * 2^32) * 2^-32 is deposited.  One thread per row.  With lnscale all zero, out is the
 *                 launch's window table bit for bit; with lnscale[c] = log s_c, the table of the design whose channel c
 *                 is scaled by s_c, from the same rays.
 * n_rows == 0 is WGRT_OK without a launch.  Asynchronous on stream.
 * _host are the twins over HOST pointers through the same header (no GPU needed): the scene is stated by nx, ny,
 * num_lmd, its channel count and scene_ranges, HOST float64 [nx, ny, 4] (eff_reg_FOV_range); the plan by its mask.
 * wgrt_visit_channel_host is the channel table itself: the index of branch `branch` (0-based) of `state` (9: the
 * in-coupling event; 0..5: R0..R5) in slice `slice`, or -1; wgrt_visit_channel_count_host is C. */
wgrt_status wgrt_visits_sensitivity(const wgrt_scene *scene, const wgrt_window_plan *plan, const uint32_t *counts,
                                    const wgrt_visit_end *ends, int64_t n_rows, double *sens, void *stream);
wgrt_status wgrt_visits_reweight(const wgrt_scene *scene, const wgrt_window_plan *plan, const uint32_t *counts,
                                 const wgrt_visit_end *ends, int64_t n_rows, const double *lnscale, double *out,
                                 void *stream);
wgrt_status wgrt_visits_sensitivity_host(int32_t nx, int32_t ny, int32_t num_lmd, int32_t n_channels,
                                         const double *scene_ranges, const float *mask, int32_t ms, int32_t step_y,
                                         int32_t step_x, const uint32_t *counts, const wgrt_visit_end *ends,
                                         int64_t n_rows, double *sens);
wgrt_status wgrt_visits_reweight_host(int32_t nx, int32_t ny, int32_t num_lmd, int32_t n_channels,
                                      const double *scene_ranges, const float *mask, int32_t ms, int32_t step_y,
                                      int32_t step_x, const uint32_t *counts, const wgrt_visit_end *ends, int64_t n_rows,
                                      const double *lnscale, double *out);
int32_t wgrt_visit_channel_host(int32_t n_fc_slices, int32_t n_oc_slices, int32_t state, int32_t slice, int32_t branch);
int32_t wgrt_visit_channel_count_host(int32_t n_fc_slices, int32_t n_oc_slices);
/* Design ensembles: K re-weighted tables from one pass over the rows (new symbols within ABI 9, looked up by name; the
 * rule is stated once in csrc/wgrt_visits.h).
 *   lnscale  DEVICE float64 [K, C], 8-B aligned: design k's log-scales are lnscale + k * C.  Finite values only.
 *   out      DEVICE float64 [K, n_slabs, W], ADDED to: table k is exactly what wgrt_visits_reweight adds with
 *            lnscale + k * C -- per delivered row the same chain of fmas in ascending c (the kernel walks the row's
 *            non-zero counts only, which gives the same bits), the same exp, q = rint(w * 2^32) * 2^-32 deposited
 *            through the same window membership -- so on one device table k equals the single call's bit for bit, and
 *            with lnscale row k all zero it is the launch's window table.  A row that deposits nothing in the single
 *            call deposits nothing for any design.
 *   wsums    NULL, or DEVICE int64 [K, 2, num_lmd], 8-B aligned, ADDED to, in quanta of 2^-32: every depositing row
 *            adds rint(q * 2^32) to wsums[k][0][l] and rint(q * q * 2^32) to wsums[k][1][l], l = tile / (nx * ny).  A
 *            value that is not below 2^62 (an overflowed weight) adds 2^62 instead.  Integer adds: exact, order-free
 *            and additive over shards at any size.  The effective sample size of design k at wavelength l is
 *            s1^2 / s2 of the two sums.
 * A workgroup reads a row once for a chunk of 64 designs, a lane per design.  The deposits go either straight into out
 * or into a stream-ordered scratch [n_slabs * W, 64] (n_slabs * W * 512 bytes, allocated and freed on `stream` by the
 * call) that a second kernel adds into the chunk's tables; both give the same bits
 * (wgrt_debug_set_reweight_layout).  K < 1, a NULL or misaligned lnscale and a misaligned wsums are
 * WGRT_ERR_INVALID_ARGUMENT, as is whatever wgrt_visits_reweight refuses; a scene with more than 126 channels is
 * WGRT_ERR_UNSUPPORTED (the chunk's log-scales must fit in 64 KiB of LDS).  n_rows == 0 is WGRT_OK without a launch.
 * Asynchronous on stream.  _host is the twin over HOST pointers through the same header, the scene and the plan stated
 * as for wgrt_visits_reweight_host.  wgrt_visit_wavelengths is the scene's num_lmd, the last extent of wsums (-1 for a
 * NULL scene). */
int32_t wgrt_visit_wavelengths(const wgrt_scene *scene);
wgrt_status wgrt_visits_reweight_many(const wgrt_scene *scene, const wgrt_window_plan *plan, const uint32_t *counts,
                                      const wgrt_visit_end *ends, int64_t n_rows, const double *lnscale, int32_t K,
                                      double *out, int64_t *wsums, void *stream);
wgrt_status wgrt_visits_reweight_many_host(int32_t nx, int32_t ny, int32_t num_lmd, int32_t n_channels,
                                           const double *scene_ranges, const float *mask, int32_t ms, int32_t step_y,
                                           int32_t step_x, const uint32_t *counts, const wgrt_visit_end *ends,
                                           int64_t n_rows, const double *lnscale, int32_t K, double *out, int64_t *wsums);

/* Polarisation of the delivered light: Stokes window tables (new symbols within ABI 9, looked up by name; the rule is
 * stated once in csrc/wgrt_stokes.h).
 *
 * wgrt_trace_stokes is wgrt_trace_windows that also keeps the polarisation state of every out-coupling the window table
 * counts.  With a / b the complex TE / TM amplitudes of the out-coupled order's field (the reference's third
 * E_field_cal of the R4 / R5 interaction), S0 = |a|^2 + |b|^2, s1 = (|a|^2 - |b|^2) / S0, s2 = 2 Re(a conj b) / S0,
 * s3 = 2 Im(conj a b) / S0, a deposit is the three int32 quanta q_k = rint(s_k * 2^30) ((0, 0, 0) unless S0 is positive
 * and finite).  The basis is the TE / TM basis of that FoV's out-coupled order, exactly as the reference's LUTs define
 * it; nothing rotates it into a frame common to the FoVs.
 *   stokes  DEVICE int64 [3, n_slabs, W], 8-B aligned, caller-owned, ADDED to: an out-coupling inside its FoV's eyebox
 *           rectangle whose aliased offset lies in the buffer adds q_k to table k at exactly the entries of `table` it
 *           adds 1 to (the slab's total and every window holding the bin).  Out-couplings beside the rectangle deposit
 *           nothing.  Integer atomics: order-independent, the same bits on every run, shards add exactly; exact while
 *           an entry has fewer than 2^33 deposits.
 * `table` and `plan` are required; matrix_EB stays optional.  rng_states, matrix_EB, table, per_ray_bounces and every
 * field of stats are the bytes of the launch without the tables.  A single launch: num_iter > 1 is
 * WGRT_ERR_INVALID_ARGUMENT, the debug timeline WGRT_ERR_UNSUPPORTED, a chain takes no tables, the launch never learns
 * the tile table, and no entry point combines it with another sink or with replicas.  stokes == NULL is exactly
 * wgrt_trace_windows.
 * wgrt_stokes_quanta_host is the rule itself over one field (no GPU needed): q HOST int32 [3]. */
wgrt_status wgrt_trace_stokes(const wgrt_scene *scene, const wgrt_rays *rays, int64_t n_rays, int64_t gid_offset,
                              uint32_t *rng_states, float *matrix_EB, wgrt_trace_stats *stats, uint32_t *per_ray_bounces,
                              void *stream, const wgrt_launch_opts *opts, const wgrt_window_plan *plan, double *table,
                              int64_t *stokes);
void wgrt_stokes_quanta_host(double a_re, double a_im, double b_re, double b_im, int32_t *q);

/* Host-only (no GPU needed; test hooks) through the same membership code (csrc/wgrt_window.h):
 * _validate is wgrt_window_plan_create's argument check alone; _table_host ADDS the n hits at flat grid
 * offsets offsets[n] (HOST int64; those outside [0, n_slabs * 9600) are dropped, as the grid's guard drops
 * them) to the HOST table [n_slabs, W]. */
wgrt_status wgrt_window_plan_validate(const float *mask, int32_t ms, int32_t step_y, int32_t step_x);
wgrt_status wgrt_window_table_host(const float *mask, int32_t ms, int32_t step_y, int32_t step_x,
                                   const int64_t *offsets, int64_t n, int64_t n_slabs, double *table);

/* Polygon membership of n points (DEVICE xy[n, 2]) through the scene's locator:
 * bit k of out_mask[i] = is_inside_or_on_edge(point i, polygon k) with polygon order
 * 0 eff_reg1, 1 eff_reg2, 2 IC, 3.. FC slices, then OC slices (GRTF:63-71).  Bit 63 is set
 * if the two exact fallbacks the kernels use (CSR row lists, 128-B band records) disagreed
 * for any polygon.  Test hook. */
wgrt_status wgrt_scene_classify(const wgrt_scene *scene, const double *xy, int64_t n,
                                uint64_t *out_mask, void *stream);

/* Host-only replica of the locator (no GPU needed; test hook): builds the scene's
 * locator with cell size cell_mm and classifies n HOST points exactly as the kernels do. */
wgrt_status wgrt_locator_classify_host(const wgrt_scene_desc *desc, double cell_mm, const double *xy, int64_t n,
                                       uint64_t *out_mask);

/* Host-only build of the byte locator's tables (no GPU needed; test hook; a new symbol within ABI 9, looked up
 * by name): the locator grid of cell size cell_mm (ncx x ncy cells; grid[3]: the origin x0, y0 and the cell
 * size in use, so that cell (ix, iy) covers [x0 + ix h, x0 + (ix + 1) h) x [y0 + iy h, ...)), the count of its distinct cell words
 * (saturating at 2048), and -- when that count is at most 256 and at most the debug cap
 * (wgrt_debug_set_palette_cap), i.e. when a scene of this descriptor gets a byte grid -- the palette (256
 * words: the distinct words strictly ascending, zero past the count) and the byte grid (each cell's palette
 * index); byte_grid says whether.  cells: the word grid itself.  Every output may be NULL; cells8 / cells hold n_cells = ncx * ncy
 * entries (call once with both NULL to learn the size).  Without a byte grid, palette and cells8 are not
 * written. */
wgrt_status wgrt_locator_palette_host(const wgrt_scene_desc *desc, double cell_mm, int64_t *ncx, int64_t *ncy,
                                      double *grid, int *distinct_words, int *byte_grid, uint64_t *palette, uint8_t *cells8,
                                      uint64_t *cells, int64_t n_cells);

/* The test / profiling hooks (certification shadow, scene copies, wave timeline, launch
 * overrides) are declared in include/wgrt_debug.h. */

/* Device math self-test (test hook): for i < n, out[k * n + i] holds
 * k=0 sqrt(a), 1 a / b, 2 hypot_cr(a, b), 3 atan2(a, b), 4 sin(a), 5 cos(a), 6 wrap(a). */
wgrt_status wgrt_selftest_math(const double *a, const double *b, int64_t n, double *out, void *stream);

const char *wgrt_status_string(wgrt_status s);
const char *wgrt_last_error(void);   /* detail of the last failure on this thread */
int wgrt_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* WGRT_H */
