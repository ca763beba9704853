// wgrt_torch.cpp -- the bounce kernel as PyTorch-ROCm operators: torch.ops.wgrt.trace and, with the pupil-window
// table as a second sink (wgrt_trace_windows), torch.ops.wgrt.trace_windows.
//
// The launch path the Python layer takes for torch tensors (engine.trace_fullcolor / trace_single):
// one call of process_rays_kernel_pro_fullColor[blocks, tpb](...) or process_rays_kernel_pro[...]
// (GRTF:833-1246 / 419-831, launched at MAIN:167-177) on device tensors, forwarded to the C ABI's
// wgrt_trace_opts (include/wgrt.h) on the caller's stream.  The operator holds no state and does
// no arithmetic: it checks every tensor against the scene (device, dtype, layout, length), builds
// the wgrt_rays / wgrt_launch_opts records and returns the library's status; the Python layer
// raises on a nonzero status with wgrt_last_error()'s detail.  Tensor misuse raises here
// (c10::Error) even for callers that skip the Python checks.
//
// libwgrt.so is not a link dependency: its symbols resolve against the global scope, where the
// Python layer loaded it (RTLD_GLOBAL, _lib.load) -- the in-tree build or the one WGRT_LIB names,
// so the operator and the ctypes entry points always share one library and one set of scenes.  The
// extension is linked with -z now, so loading it without libwgrt fails at load time, not mid-call.
// The window sink's entry points arrived within ABI 9 and are looked up by name at the first trace_windows
// call (as _lib.load binds them), so the operator library still loads over an earlier ABI-9 build of libwgrt
// (tools/with_lib.py), where trace keeps working and trace_windows raises.  The same holds for the chained launches'
// entry points (wgrt_chain_*; torch.ops.wgrt.chain_begin / chain_step / chain_end, engine.TraceChain) and for
// wgrt_trace_fate (torch.ops.wgrt.trace_fate: the launch that also stores every ray's fate code) and wgrt_trace_replicas
// (torch.ops.wgrt.trace_replicas: the launch into replica window tables).
#include <torch/library.h>

#include <ATen/core/Tensor.h>
#include <c10/core/DeviceGuard.h>

#include <dlfcn.h>

#include <algorithm>
#include <cstdint>
#include <optional>

#include "wgrt.h"

namespace {

using at::Tensor;

struct Ctx {
    c10::Device dev;
    int64_t rays;   // length of every ray column (the batch)
};

void on_device(const Tensor &t, const char *name, const Ctx &c) {
    TORCH_CHECK(t.device() == c.dev, "wgrt.trace: ", name, " must be on ", c.dev, ", got ", t.device());
    TORCH_CHECK(t.is_contiguous(), "wgrt.trace: ", name, " must be contiguous");
}

const float *column(const Tensor &t, const char *name, const Ctx &c) {
    on_device(t, name, c);
    TORCH_CHECK(t.scalar_type() == at::kFloat, "wgrt.trace: ray column ", name, " must be float32");
    TORCH_CHECK(t.numel() == c.rays, "wgrt.trace: ray column ", name, " has ", t.numel(), " rays, x has ", c.rays);
    return static_cast<const float *>(t.const_data_ptr());
}

// uint32 buffers arrive as uint32 tensors or as int32 views of them
void *u32(const Tensor &t, const char *name, const Ctx &c, int64_t need) {
    on_device(t, name, c);
    TORCH_CHECK(t.scalar_type() == at::kInt || t.scalar_type() == at::kUInt32, "wgrt.trace: ", name,
                " must be uint32 (or an int32 view)");
    TORCH_CHECK(t.numel() >= need, "wgrt.trace: ", name, " holds ", t.numel(), " entries, needs ", need);
    return t.data_ptr();
}

// wgrt_trace_windows / wgrt_window_plan_width of the loaded libwgrt.so (global scope), or an error.
struct WindowAbi {
    decltype(&wgrt_trace_windows) trace;
    decltype(&wgrt_window_plan_width) width;
};
const WindowAbi &window_abi() {
    static const WindowAbi abi{reinterpret_cast<decltype(&wgrt_trace_windows)>(dlsym(RTLD_DEFAULT, "wgrt_trace_windows")),
                               reinterpret_cast<decltype(&wgrt_window_plan_width)>(
                                   dlsym(RTLD_DEFAULT, "wgrt_window_plan_width"))};
    TORCH_CHECK(abi.trace && abi.width, "wgrt.trace_windows: the loaded libwgrt.so has no wgrt_trace_windows (a build "
                                        "from before the window-table sink)");
    return abi;
}

// The chain's entry points (wgrt_chain_*), new within ABI 9 as well: looked up at the first chain_begin.
struct ChainAbi {
    decltype(&wgrt_chain_begin) begin;
    decltype(&wgrt_chain_step) step;
    decltype(&wgrt_chain_end) end;
};
const ChainAbi &chain_abi() {
    static const ChainAbi abi{reinterpret_cast<decltype(&wgrt_chain_begin)>(dlsym(RTLD_DEFAULT, "wgrt_chain_begin")),
                              reinterpret_cast<decltype(&wgrt_chain_step)>(dlsym(RTLD_DEFAULT, "wgrt_chain_step")),
                              reinterpret_cast<decltype(&wgrt_chain_end)>(dlsym(RTLD_DEFAULT, "wgrt_chain_end"))};
    TORCH_CHECK(abi.begin && abi.step && abi.end, "wgrt.chain_begin: the loaded libwgrt.so has no wgrt_chain_begin (a "
                                                  "build from before the chained launches)");
    return abi;
}

// wgrt_trace_fate (per-ray fate codes), new within ABI 9 too: looked up at the first trace_fate call.
decltype(&wgrt_trace_fate) fate_abi() {
    static const auto fn = reinterpret_cast<decltype(&wgrt_trace_fate)>(dlsym(RTLD_DEFAULT, "wgrt_trace_fate"));
    TORCH_CHECK(fn, "wgrt.trace_fate: the loaded libwgrt.so has no wgrt_trace_fate (a build from before the ray fates)");
    return fn;
}

// wgrt_trace_replicas (replica window tables), new within ABI 9 too: looked up at the first trace_replicas call.
decltype(&wgrt_trace_replicas) replicas_abi() {
    static const auto fn = reinterpret_cast<decltype(&wgrt_trace_replicas)>(dlsym(RTLD_DEFAULT, "wgrt_trace_replicas"));
    TORCH_CHECK(fn, "wgrt.trace_replicas: the loaded libwgrt.so has no wgrt_trace_replicas (a build from before the "
                    "replica tables)");
    return fn;
}

// wgrt_trace_expected (the expected-value estimator), new within ABI 9 too: looked up at the first trace_expected call.
decltype(&wgrt_trace_expected) expected_abi() {
    static const auto fn = reinterpret_cast<decltype(&wgrt_trace_expected)>(dlsym(RTLD_DEFAULT, "wgrt_trace_expected"));
    TORCH_CHECK(fn, "wgrt.trace_expected: the loaded libwgrt.so has no wgrt_trace_expected (a build from before the "
                    "expected-value estimator)");
    return fn;
}

// wgrt_trace_footprint (the footprint maps), new within ABI 9 too: looked up at the first trace_footprint call.
decltype(&wgrt_trace_footprint) footprint_abi() {
    static const auto fn = reinterpret_cast<decltype(&wgrt_trace_footprint)>(dlsym(RTLD_DEFAULT, "wgrt_trace_footprint"));
    TORCH_CHECK(fn, "wgrt.trace_footprint: the loaded libwgrt.so has no wgrt_trace_footprint (a build from before the "
                    "footprint maps)");
    return fn;
}

// wgrt_trace_hits (the hit list), new within ABI 9 too: looked up at the first trace_hits call.
decltype(&wgrt_trace_hits) hits_abi() {
    static const auto fn = reinterpret_cast<decltype(&wgrt_trace_hits)>(dlsym(RTLD_DEFAULT, "wgrt_trace_hits"));
    TORCH_CHECK(fn, "wgrt.trace_hits: the loaded libwgrt.so has no wgrt_trace_hits (a build from before the hit list)");
    return fn;
}

// wgrt_trace_paths and wgrt_paths_footprint (ray paths), new within ABI 9 too: looked up at the first call of either.
struct PathsAbi {
    decltype(&wgrt_trace_paths) trace;
    decltype(&wgrt_paths_footprint) footprint;
};
const PathsAbi &paths_abi() {
    static const PathsAbi abi{reinterpret_cast<decltype(&wgrt_trace_paths)>(dlsym(RTLD_DEFAULT, "wgrt_trace_paths")),
                              reinterpret_cast<decltype(&wgrt_paths_footprint)>(dlsym(RTLD_DEFAULT, "wgrt_paths_footprint"))};
    TORCH_CHECK(abi.trace && abi.footprint,
                "wgrt.trace_paths: the loaded libwgrt.so has no wgrt_trace_paths (a build from before the ray paths)");
    return abi;
}

// wgrt_trace_visits and the two reductions (branch visit counts), new within ABI 9 too: looked up at the first call.
struct VisitsAbi {
    decltype(&wgrt_trace_visits) trace;
    decltype(&wgrt_visits_sensitivity) sensitivity;
    decltype(&wgrt_visits_reweight) reweight;
    decltype(&wgrt_visit_channels) channels;
};
const VisitsAbi &visits_abi() {
    static const VisitsAbi abi{
        reinterpret_cast<decltype(&wgrt_trace_visits)>(dlsym(RTLD_DEFAULT, "wgrt_trace_visits")),
        reinterpret_cast<decltype(&wgrt_visits_sensitivity)>(dlsym(RTLD_DEFAULT, "wgrt_visits_sensitivity")),
        reinterpret_cast<decltype(&wgrt_visits_reweight)>(dlsym(RTLD_DEFAULT, "wgrt_visits_reweight")),
        reinterpret_cast<decltype(&wgrt_visit_channels)>(dlsym(RTLD_DEFAULT, "wgrt_visit_channels"))};
    TORCH_CHECK(abi.trace && abi.sensitivity && abi.reweight && abi.channels,
                "wgrt.trace_visits: the loaded libwgrt.so has no wgrt_trace_visits (a build from before the visit counts)");
    return abi;
}

// A visits launch's rows (trace_visits): counts int32 [n_rows, C] (the library's uint32 words), ends uint8 [n_rows, 32],
// slot int32 [n_rays] or none.
struct VisitRows {
    const std::optional<Tensor> &slot;
    Tensor counts, ends;
    int64_t n_rows;
};

// All three launching operators: trace (the grid alone: plan 0, no table), trace_windows (the grid, the window
// table of plan `plan` -- a wgrt_window_plan handle -- or both) and, with `chain`, chain_begin: the same checks and
// records handed to wgrt_chain_begin, which launches nothing and leaves the chain's handle in *chain.
int64_t trace_core(int64_t scene, const Tensor &x, const Tensor &y, const Tensor &m, const Tensor &n,
                   const std::optional<Tensor> &lmd_num, const Tensor &te, const Tensor &tm, const Tensor &delta_phase,
                   Tensor rng_states, std::optional<Tensor> matrix_EB, std::optional<Tensor> stats,
                   std::optional<Tensor> per_ray_bounces, int64_t n_rays, int64_t gid_offset, int64_t stream,
                   int64_t kernel, int64_t variant, int64_t workgroups, const std::optional<Tensor> &chunk_order,
                   int64_t num_iter, const std::optional<Tensor> &gid_blocks, int64_t gid_block_rays, int64_t debug,
                   double grid_sqrt_k, int64_t plan, std::optional<Tensor> table, wgrt_chain **chain,
                   std::optional<Tensor> fate = std::nullopt, int64_t replicas = 0, bool expected = false,
                   const wgrt_footprint_plan *fp = nullptr, std::optional<Tensor> fp_map = std::nullopt,
                   std::optional<Tensor> hits = std::nullopt, int64_t hit_capacity = 0,
                   std::optional<Tensor> hit_count = std::nullopt, int64_t hit_tag = 0, bool as_paths = false,
                   const std::optional<Tensor> &select = std::nullopt, const VisitRows *visits = nullptr) {
    const wgrt_scene *s = reinterpret_cast<const wgrt_scene *>(static_cast<uintptr_t>(scene));
    TORCH_CHECK(s != nullptr, "wgrt.trace: NULL scene");
    wgrt_scene_info info{};
    const wgrt_status st = wgrt_scene_get_info(s, &info);
    if (st != WGRT_OK) return st;
    const Ctx c{c10::Device(c10::DeviceType::CUDA, static_cast<c10::DeviceIndex>(info.device)), x.numel()};
    // the scene's device is current for the call (the library selects it too, include/wgrt.h) and the
    // caller's comes back on return
    const c10::DeviceGuard guard(c.dev);
    TORCH_CHECK(n_rays >= 0 && n_rays <= c.rays, "wgrt.trace: n_rays=", n_rays, " out of range for ", c.rays, " rays");
    TORCH_CHECK(kernel == 0 || kernel == 1, "wgrt.trace: kernel must be 0 (full colour) or 1 (single wavelength)");

    wgrt_rays r{};
    r.x = column(x, "x", c);
    r.y = column(y, "y", c);
    r.m = column(m, "m", c);
    r.n = column(n, "n", c);
    if (kernel == 0) {
        TORCH_CHECK(lmd_num.has_value(), "wgrt.trace: the full-colour kernel needs lmd_num");
        r.lmd_num = column(*lmd_num, "lmd_num", c);
    }
    r.te = column(te, "te", c);
    r.tm = column(tm, "tm", c);
    r.delta_phase = column(delta_phase, "delta_phase", c);

    uint32_t *rng = static_cast<uint32_t *>(u32(rng_states, "rng_states", c, c.rays));
    TORCH_CHECK(matrix_EB.has_value() || table.has_value(), "wgrt.trace: needs matrix_EB, a window table, or both");
    float *eb = nullptr;
    if (matrix_EB) {
        on_device(*matrix_EB, "matrix_EB", c);
        TORCH_CHECK(matrix_EB->scalar_type() == at::kFloat, "wgrt.trace: matrix_EB must be float32");
        const int64_t eb_want = (int64_t)info.tiles * 80 * 120;   // [L,] NY, NX, 80, 120
        TORCH_CHECK(matrix_EB->numel() == eb_want, "wgrt.trace: matrix_EB holds ", matrix_EB->numel(),
                    " floats, the scene's grid has ", eb_want);
        eb = matrix_EB->data_ptr<float>();
    }
    const wgrt_window_plan *wp = reinterpret_cast<const wgrt_window_plan *>(static_cast<uintptr_t>(plan));
    double *tab = nullptr;
    if (table) {
        const int64_t W = window_abi().width(wp);
        TORCH_CHECK(W > 0, "wgrt.trace: a window table needs its plan");
        on_device(*table, "table", c);
        TORCH_CHECK(table->scalar_type() == at::kDouble, "wgrt.trace: table must be float64");
        if (replicas >= 2) {   // trace_replicas: one table per replica (the library checks the count's range)
            TORCH_CHECK(table->dim() == 3 && table->size(0) == replicas && table->size(1) == info.tiles && table->size(2) == W,
                        "wgrt.trace_replicas: table must have shape [", replicas, ", ", info.tiles, ", ", W, "], got ",
                        table->sizes());
        } else {
            TORCH_CHECK(table->dim() == 2 && table->size(0) == info.tiles && table->size(1) == W,
                        "wgrt.trace: table must have shape [", info.tiles, ", ", W, "], got ", table->sizes());
        }
        tab = table->data_ptr<double>();
    }
    wgrt_trace_stats *stp = nullptr;
    if (stats) {
        on_device(*stats, "stats", c);
        TORCH_CHECK(stats->scalar_type() == at::kLong && stats->numel() * 8 == (int64_t)sizeof(wgrt_trace_stats),
                    "wgrt.trace: stats must be int64[", sizeof(wgrt_trace_stats) / 8, "]");
        stp = static_cast<wgrt_trace_stats *>(stats->data_ptr());
    }
    uint32_t *per = per_ray_bounces ? static_cast<uint32_t *>(u32(*per_ray_bounces, "per_ray_bounces", c, c.rays))
                                    : nullptr;

    wgrt_launch_opts o{};
    o.kernel = (int)kernel;
    o.variant = (int)variant;
    o.workgroups = (int)workgroups;
    if (chunk_order) {
        on_device(*chunk_order, "chunk_order", c);
        const int64_t chunks = (n_rays + 63) / 64;
        TORCH_CHECK(chunk_order->scalar_type() == at::kInt && chunk_order->numel() == chunks,
                    "wgrt.trace: chunk_order must be int32[", chunks, "]");
        o.chunk_order = static_cast<const int32_t *>(chunk_order->const_data_ptr());
        o.n_chunk_order = chunks;
    }
    o.num_iter = (int)num_iter;
    if (gid_blocks) {
        on_device(*gid_blocks, "gid_blocks", c);
        TORCH_CHECK(gid_block_rays >= 1, "wgrt.trace: gid_blocks needs gid_block_rays >= 1");
        const int64_t blocks = (n_rays + gid_block_rays - 1) / gid_block_rays;
        TORCH_CHECK(gid_blocks->scalar_type() == at::kLong && gid_blocks->numel() >= blocks,
                    "wgrt.trace: gid_blocks must be int64 with >= ", blocks, " entries");
        o.gid_blocks = static_cast<const int64_t *>(gid_blocks->const_data_ptr());
        o.gid_block_rays = gid_block_rays;
    }
    // test / profiling hooks: the address of a wgrt_debug_opts record the caller keeps alive (0: none)
    o.debug = reinterpret_cast<const wgrt_debug_opts *>(static_cast<uintptr_t>(debug));
    o.grid_sqrt_k = grid_sqrt_k;
    void *const hip_stream = reinterpret_cast<void *>(static_cast<uintptr_t>(stream));
    if (chain) {
        TORCH_CHECK(!per, "wgrt.chain_begin: a chain takes no per_ray_bounces");
        return chain_abi().begin(s, &r, n_rays, gid_offset, rng, eb, stp, hip_stream, &o, tab ? wp : nullptr, tab, chain);
    }
    if (visits) {   // trace_visits: the rows' counts and end records, and the batch's slots
        TORCH_CHECK(!hits && !fp_map && !fate && replicas == 0 && !expected,
                    "wgrt.trace_visits: takes no fate, replicas, expected, footprint map or list");
        const int64_t C = visits_abi().channels(s);
        on_device(visits->counts, "counts", c);
        on_device(visits->ends, "ends", c);
        // (a negative n_rows is the library's to refuse; the rows must lie inside both buffers)
        TORCH_CHECK(visits->counts.scalar_type() == at::kInt && visits->counts.is_contiguous() &&
                        visits->counts.numel() >= std::max<int64_t>(visits->n_rows, 0) * C,
                    "wgrt.trace_visits: counts must be contiguous int32 with >= n_rows * ", C, " entries");
        TORCH_CHECK(visits->ends.scalar_type() == at::kByte && visits->ends.is_contiguous() &&
                        visits->ends.numel() >= std::max<int64_t>(visits->n_rows, 0) * (int64_t)sizeof(wgrt_visit_end),
                    "wgrt.trace_visits: ends must be contiguous uint8 with >= n_rows * 32 bytes");
        const int32_t *slot = nullptr;
        if (visits->slot) {
            on_device(*visits->slot, "slot", c);
            TORCH_CHECK(visits->slot->scalar_type() == at::kInt && visits->slot->is_contiguous() &&
                            visits->slot->numel() >= n_rays,
                        "wgrt.trace_visits: slot must be contiguous int32 with >= ", n_rays, " entries");
            slot = static_cast<const int32_t *>(visits->slot->const_data_ptr());
        }
        return visits_abi().trace(s, &r, n_rays, gid_offset, rng, eb, stp, per, hip_stream, &o, tab ? wp : nullptr, tab, slot,
                                  visits->n_rows, static_cast<uint32_t *>(visits->counts.data_ptr()),
                                  static_cast<wgrt_visit_end *>(visits->ends.data_ptr()));
    }
    if (hits) {   // trace_hits / trace_paths: the record buffer (uint8, 32 bytes per record), its capacity, the counter
                  // and the tag; trace_paths (as_paths) also the batch's select bytes
        static_assert(sizeof(wgrt_hit) == sizeof(wgrt_path_vertex), "both lists hold 32-byte records");
        const char *const op = as_paths ? "wgrt.trace_paths" : "wgrt.trace_hits";
        TORCH_CHECK(!fp_map && !fate && replicas == 0 && !expected, op, ": takes no fate, replicas, expected or footprint map");
        on_device(*hits, "list", c);
        TORCH_CHECK(hits->scalar_type() == at::kByte && hits->is_contiguous(), op, ": the list must be contiguous uint8");
        // (a negative capacity is the library's to refuse; a positive one must lie inside the buffer)
        TORCH_CHECK(hit_capacity <= 0 || hit_capacity <= hits->numel() / (int64_t)sizeof(wgrt_hit), op, ": capacity ",
                    hit_capacity, " exceeds the buffer's ", hits->numel() / (int64_t)sizeof(wgrt_hit), " records");
        uint64_t *cnt = nullptr;
        if (hit_count) {
            on_device(*hit_count, "count", c);
            TORCH_CHECK(hit_count->scalar_type() == at::kLong && hit_count->numel() == 1, op, ": count must be int64[1]");
            cnt = static_cast<uint64_t *>(hit_count->data_ptr());
        }
        // (out of uint32 range: a tag the library refuses)
        const uint32_t tag = hit_tag < 0 || hit_tag > 0xffffffffll ? 0xffffffffu : static_cast<uint32_t>(hit_tag);
        if (as_paths) {
            const uint8_t *sel = nullptr;
            if (select) {
                on_device(*select, "select", c);
                TORCH_CHECK(select->scalar_type() == at::kByte && select->is_contiguous() && select->numel() >= n_rays,
                            "wgrt.trace_paths: select must be contiguous uint8 with >= ", n_rays, " entries");
                sel = static_cast<const uint8_t *>(select->const_data_ptr());
            }
            return paths_abi().trace(s, &r, n_rays, gid_offset, rng, eb, stp, per, hip_stream, &o, tab ? wp : nullptr, tab,
                                     static_cast<wgrt_path_vertex *>(hits->data_ptr()), hit_capacity, cnt, tag, sel);
        }
        return hits_abi()(s, &r, n_rays, gid_offset, rng, eb, stp, per, hip_stream, &o, tab ? wp : nullptr, tab,
                          static_cast<wgrt_hit *>(hits->data_ptr()), hit_capacity, cnt, tag);
    }
    if (fp_map) {   // trace_footprint: int64 [num_lmd, 9, ny_cells, nx_cells], added to by every counted draw
        TORCH_CHECK(fp && !fate && replicas == 0 && !expected, "wgrt.trace_footprint: takes no fate, replicas or expected");
        on_device(*fp_map, "map", c);
        TORCH_CHECK(fp_map->scalar_type() == at::kLong, "wgrt.trace_footprint: map must be int64");
        // (a plan the library refuses has no size to compare with: the library's check answers first)
        // (the scene's info has its tile count, num_lmd * nx * ny: the Python layer checks the first axis exactly)
        const bool sized = fp->nx_cells >= 1 && fp->nx_cells <= 4096 && fp->ny_cells >= 1 && fp->ny_cells <= 4096;
        TORCH_CHECK(!sized || (fp_map->is_contiguous() && fp_map->dim() == 4 && fp_map->size(0) >= 1 &&
                               info.tiles % fp_map->size(0) == 0 && fp_map->size(1) == WGRT_FOOTPRINT_CHANNELS &&
                               fp_map->size(2) == fp->ny_cells && fp_map->size(3) == fp->nx_cells),
                    "wgrt.trace_footprint: map must be contiguous [num_lmd, ", WGRT_FOOTPRINT_CHANNELS, ", ", fp->ny_cells,
                    ", ", fp->nx_cells, "], got ", fp_map->sizes());
        return footprint_abi()(s, &r, n_rays, gid_offset, rng, eb, stp, per, hip_stream, &o, tab ? wp : nullptr, tab, fp,
                               static_cast<int64_t *>(fp_map->data_ptr()));
    }
    if (expected) {   // trace_expected: the window table alone (its shape checked above: [tiles, W], or one per replica)
        TORCH_CHECK(tab && !eb && !fate, "wgrt.trace_expected: needs a window table and takes no matrix_EB or fate");
        return expected_abi()(s, &r, n_rays, gid_offset, rng, stp, per, hip_stream, &o, wp, tab,
                              static_cast<int>(std::max<int64_t>(-1, std::min<int64_t>(replicas, 1 << 20))));
    }
    if (replicas != 0) {   // trace_replicas (0: the call is trace_windows, below)
        TORCH_CHECK(!fate, "wgrt.trace_replicas: takes no fate");
        return replicas_abi()(s, &r, n_rays, gid_offset, rng, eb, stp, per, hip_stream, &o, tab ? wp : nullptr, tab,
                              static_cast<int>(std::max<int64_t>(-1, std::min<int64_t>(replicas, 1 << 20))));
    }
    if (fate) {   // trace_fate: one uint8 per ray of the batch, written by the lane that ends the ray's trace
        on_device(*fate, "fate", c);
        TORCH_CHECK(fate->scalar_type() == at::kByte, "wgrt.trace_fate: fate must be uint8");
        TORCH_CHECK(fate->numel() == c.rays, "wgrt.trace_fate: fate holds ", fate->numel(), " entries, the batch has ", c.rays);
        return fate_abi()(s, &r, n_rays, gid_offset, rng, eb, stp, per, hip_stream, &o, tab ? wp : nullptr, tab,
                          static_cast<uint8_t *>(fate->data_ptr()));
    }
    if (!tab) return wgrt_trace_opts(s, &r, n_rays, gid_offset, rng, eb, stp, per, hip_stream, &o);
    return window_abi().trace(s, &r, n_rays, gid_offset, rng, eb, stp, per, hip_stream, &o, wp, tab);
}

int64_t trace_impl(int64_t scene, const Tensor &x, const Tensor &y, const Tensor &m, const Tensor &n,
                   const std::optional<Tensor> &lmd_num, const Tensor &te, const Tensor &tm, const Tensor &delta_phase,
                   Tensor rng_states, std::optional<Tensor> matrix_EB, std::optional<Tensor> stats,
                   std::optional<Tensor> per_ray_bounces, int64_t n_rays, int64_t gid_offset, int64_t stream,
                   int64_t kernel, int64_t variant, int64_t workgroups, const std::optional<Tensor> &chunk_order,
                   int64_t num_iter, const std::optional<Tensor> &gid_blocks, int64_t gid_block_rays, int64_t debug,
                   double grid_sqrt_k, int64_t plan, std::optional<Tensor> table) {
    return trace_core(scene, x, y, m, n, lmd_num, te, tm, delta_phase, rng_states, matrix_EB, stats, per_ray_bounces,
                      n_rays, gid_offset, stream, kernel, variant, workgroups, chunk_order, num_iter, gid_blocks,
                      gid_block_rays, debug, grid_sqrt_k, plan, table, nullptr);
}

// trace_fate: trace_windows' arguments and the fate buffer (wgrt_trace_fate).
int64_t trace_fate(int64_t scene, const Tensor &x, const Tensor &y, const Tensor &m, const Tensor &n,
                   const std::optional<Tensor> &lmd_num, const Tensor &te, const Tensor &tm, const Tensor &delta_phase,
                   Tensor rng_states, std::optional<Tensor> matrix_EB, std::optional<Tensor> stats,
                   std::optional<Tensor> per_ray_bounces, int64_t n_rays, int64_t gid_offset, int64_t stream,
                   int64_t kernel, int64_t variant, int64_t workgroups, const std::optional<Tensor> &chunk_order,
                   int64_t num_iter, const std::optional<Tensor> &gid_blocks, int64_t gid_block_rays, int64_t debug,
                   double grid_sqrt_k, int64_t plan, std::optional<Tensor> table, Tensor fate) {
    return trace_core(scene, x, y, m, n, lmd_num, te, tm, delta_phase, rng_states, matrix_EB, stats, per_ray_bounces,
                      n_rays, gid_offset, stream, kernel, variant, workgroups, chunk_order, num_iter, gid_blocks,
                      gid_block_rays, debug, grid_sqrt_k, plan, table, nullptr, fate);
}

// trace_replicas: trace_windows' arguments and the replica count (wgrt_trace_replicas): table float64
// [replicas, tiles, W] for replicas >= 2.
int64_t trace_replicas(int64_t scene, const Tensor &x, const Tensor &y, const Tensor &m, const Tensor &n,
                       const std::optional<Tensor> &lmd_num, const Tensor &te, const Tensor &tm, const Tensor &delta_phase,
                       Tensor rng_states, std::optional<Tensor> matrix_EB, std::optional<Tensor> stats,
                       std::optional<Tensor> per_ray_bounces, int64_t n_rays, int64_t gid_offset, int64_t stream,
                       int64_t kernel, int64_t variant, int64_t workgroups, const std::optional<Tensor> &chunk_order,
                       int64_t num_iter, const std::optional<Tensor> &gid_blocks, int64_t gid_block_rays, int64_t debug,
                       double grid_sqrt_k, int64_t plan, std::optional<Tensor> table, int64_t replicas) {
    return trace_core(scene, x, y, m, n, lmd_num, te, tm, delta_phase, rng_states, matrix_EB, stats, per_ray_bounces,
                      n_rays, gid_offset, stream, kernel, variant, workgroups, chunk_order, num_iter, gid_blocks,
                      gid_block_rays, debug, grid_sqrt_k, plan, table, nullptr, std::nullopt, replicas);
}

// trace_expected: trace_replicas' arguments without the grid (wgrt_trace_expected): table float64 [tiles, W] for
// replicas 0 / 1, [replicas, tiles, W] otherwise.
int64_t trace_expected(int64_t scene, const Tensor &x, const Tensor &y, const Tensor &m, const Tensor &n,
                       const std::optional<Tensor> &lmd_num, const Tensor &te, const Tensor &tm, const Tensor &delta_phase,
                       Tensor rng_states, std::optional<Tensor> stats, std::optional<Tensor> per_ray_bounces,
                       int64_t n_rays, int64_t gid_offset, int64_t stream, int64_t kernel, int64_t variant,
                       int64_t workgroups, const std::optional<Tensor> &chunk_order, int64_t num_iter,
                       const std::optional<Tensor> &gid_blocks, int64_t gid_block_rays, int64_t debug,
                       double grid_sqrt_k, int64_t plan, Tensor table, int64_t replicas) {
    return trace_core(scene, x, y, m, n, lmd_num, te, tm, delta_phase, rng_states, std::nullopt, stats, per_ray_bounces,
                      n_rays, gid_offset, stream, kernel, variant, workgroups, chunk_order, num_iter, gid_blocks,
                      gid_block_rays, debug, grid_sqrt_k, plan, table, nullptr, std::nullopt, replicas, true);
}

// trace_footprint: trace_windows' arguments, the footprint plan's fields and the map (wgrt_trace_footprint).
int64_t trace_footprint(int64_t scene, const Tensor &x, const Tensor &y, const Tensor &m, const Tensor &n,
                        const std::optional<Tensor> &lmd_num, const Tensor &te, const Tensor &tm, const Tensor &delta_phase,
                        Tensor rng_states, std::optional<Tensor> matrix_EB, std::optional<Tensor> stats,
                        std::optional<Tensor> per_ray_bounces, int64_t n_rays, int64_t gid_offset, int64_t stream,
                        int64_t kernel, int64_t variant, int64_t workgroups, const std::optional<Tensor> &chunk_order,
                        int64_t num_iter, const std::optional<Tensor> &gid_blocks, int64_t gid_block_rays, int64_t debug,
                        double grid_sqrt_k, int64_t plan, std::optional<Tensor> table, double fp_x0, double fp_y0,
                        double fp_cell_x, double fp_cell_y, int64_t fp_nx_cells, int64_t fp_ny_cells, Tensor map) {
    wgrt_footprint_plan fp{};
    fp.x0 = fp_x0;
    fp.y0 = fp_y0;
    fp.cell_x = fp_cell_x;
    fp.cell_y = fp_cell_y;
    // (out of int32 range: a count the library refuses)
    fp.nx_cells = static_cast<int32_t>(std::max<int64_t>(-1, std::min<int64_t>(fp_nx_cells, 1 << 20)));
    fp.ny_cells = static_cast<int32_t>(std::max<int64_t>(-1, std::min<int64_t>(fp_ny_cells, 1 << 20)));
    return trace_core(scene, x, y, m, n, lmd_num, te, tm, delta_phase, rng_states, matrix_EB, stats, per_ray_bounces,
                      n_rays, gid_offset, stream, kernel, variant, workgroups, chunk_order, num_iter, gid_blocks,
                      gid_block_rays, debug, grid_sqrt_k, plan, table, nullptr, std::nullopt, 0, false, &fp, map);
}

// trace_hits: trace_windows' arguments, the record buffer, its capacity in records, the counter and the tag
// (wgrt_trace_hits).
int64_t trace_hits(int64_t scene, const Tensor &x, const Tensor &y, const Tensor &m, const Tensor &n,
                   const std::optional<Tensor> &lmd_num, const Tensor &te, const Tensor &tm, const Tensor &delta_phase,
                   Tensor rng_states, std::optional<Tensor> matrix_EB, std::optional<Tensor> stats,
                   std::optional<Tensor> per_ray_bounces, int64_t n_rays, int64_t gid_offset, int64_t stream,
                   int64_t kernel, int64_t variant, int64_t workgroups, const std::optional<Tensor> &chunk_order,
                   int64_t num_iter, const std::optional<Tensor> &gid_blocks, int64_t gid_block_rays, int64_t debug,
                   double grid_sqrt_k, int64_t plan, std::optional<Tensor> table, Tensor hits, int64_t capacity,
                   std::optional<Tensor> count, int64_t tag) {
    return trace_core(scene, x, y, m, n, lmd_num, te, tm, delta_phase, rng_states, matrix_EB, stats, per_ray_bounces,
                      n_rays, gid_offset, stream, kernel, variant, workgroups, chunk_order, num_iter, gid_blocks,
                      gid_block_rays, debug, grid_sqrt_k, plan, table, nullptr, std::nullopt, 0, false, nullptr,
                      std::nullopt, hits, capacity, count, tag);
}

// trace_paths: trace_hits' arguments over a path list, and the batch's select bytes (wgrt_trace_paths).
int64_t trace_paths(int64_t scene, const Tensor &x, const Tensor &y, const Tensor &m, const Tensor &n,
                    const std::optional<Tensor> &lmd_num, const Tensor &te, const Tensor &tm, const Tensor &delta_phase,
                    Tensor rng_states, std::optional<Tensor> matrix_EB, std::optional<Tensor> stats,
                    std::optional<Tensor> per_ray_bounces, int64_t n_rays, int64_t gid_offset, int64_t stream,
                    int64_t kernel, int64_t variant, int64_t workgroups, const std::optional<Tensor> &chunk_order,
                    int64_t num_iter, const std::optional<Tensor> &gid_blocks, int64_t gid_block_rays, int64_t debug,
                    double grid_sqrt_k, int64_t plan, std::optional<Tensor> table, Tensor paths, int64_t capacity,
                    std::optional<Tensor> count, int64_t tag, const std::optional<Tensor> &select) {
    return trace_core(scene, x, y, m, n, lmd_num, te, tm, delta_phase, rng_states, matrix_EB, stats, per_ray_bounces,
                      n_rays, gid_offset, stream, kernel, variant, workgroups, chunk_order, num_iter, gid_blocks,
                      gid_block_rays, debug, grid_sqrt_k, plan, table, nullptr, std::nullopt, 0, false, nullptr,
                      std::nullopt, paths, capacity, count, tag, true, select);
}

// trace_visits: trace_windows' arguments, the batch's slots (or None), the rows there are, their counts and their end
// records (wgrt_trace_visits).
int64_t trace_visits(int64_t scene, const Tensor &x, const Tensor &y, const Tensor &m, const Tensor &n,
                     const std::optional<Tensor> &lmd_num, const Tensor &te, const Tensor &tm, const Tensor &delta_phase,
                     Tensor rng_states, std::optional<Tensor> matrix_EB, std::optional<Tensor> stats,
                     std::optional<Tensor> per_ray_bounces, int64_t n_rays, int64_t gid_offset, int64_t stream,
                     int64_t kernel, int64_t variant, int64_t workgroups, const std::optional<Tensor> &chunk_order,
                     int64_t num_iter, const std::optional<Tensor> &gid_blocks, int64_t gid_block_rays, int64_t debug,
                     double grid_sqrt_k, int64_t plan, std::optional<Tensor> table, const std::optional<Tensor> &slot,
                     int64_t n_rows, Tensor counts, Tensor ends) {
    const VisitRows rows{slot, counts, ends, n_rows};
    return trace_core(scene, x, y, m, n, lmd_num, te, tm, delta_phase, rng_states, matrix_EB, stats, per_ray_bounces,
                      n_rays, gid_offset, stream, kernel, variant, workgroups, chunk_order, num_iter, gid_blocks,
                      gid_block_rays, debug, grid_sqrt_k, plan, table, nullptr, std::nullopt, 0, false, nullptr,
                      std::nullopt, std::nullopt, 0, std::nullopt, 0, false, std::nullopt, &rows);
}

// visits_reduce: the first n_rows rows of a visits table reduced on the scene's device: without lnscale into the
// sensitivity tables out [C, n_slabs, W] (wgrt_visits_sensitivity), with lnscale float64 [C] into the re-weighted window
// table out [n_slabs, W] (wgrt_visits_reweight).  Both add to out.
int64_t visits_reduce(int64_t scene, int64_t plan, const Tensor &counts, const Tensor &ends, int64_t n_rows,
                      const std::optional<Tensor> &lnscale, Tensor out, int64_t stream) {
    const wgrt_scene *s = reinterpret_cast<const wgrt_scene *>(static_cast<uintptr_t>(scene));
    const wgrt_window_plan *wp = reinterpret_cast<const wgrt_window_plan *>(static_cast<uintptr_t>(plan));
    TORCH_CHECK(s != nullptr && wp != nullptr, "wgrt.visits_reduce: NULL scene / plan");
    wgrt_scene_info info{};
    const wgrt_status st = wgrt_scene_get_info(s, &info);
    if (st != WGRT_OK) return st;
    const c10::Device dev(c10::DeviceType::CUDA, static_cast<c10::DeviceIndex>(info.device));
    const int64_t C = visits_abi().channels(s), W = window_abi().width(wp);
    TORCH_CHECK(W > 0, "wgrt.visits_reduce: a bad window plan");
    TORCH_CHECK(counts.device() == dev && ends.device() == dev && out.device() == dev,
                "wgrt.visits_reduce: counts, ends and out must be on the scene's device");
    TORCH_CHECK(n_rows >= 0 && counts.scalar_type() == at::kInt && counts.is_contiguous() && counts.numel() >= n_rows * C,
                "wgrt.visits_reduce: counts must be contiguous int32 with >= n_rows * ", C, " entries");
    TORCH_CHECK(ends.scalar_type() == at::kByte && ends.is_contiguous() &&
                    ends.numel() >= n_rows * (int64_t)sizeof(wgrt_visit_end),
                "wgrt.visits_reduce: ends must be contiguous uint8 with >= n_rows * 32 bytes");
    TORCH_CHECK(out.scalar_type() == at::kDouble && out.is_contiguous() &&
                    out.numel() == (lnscale ? 1 : C) * (int64_t)info.tiles * W,
                "wgrt.visits_reduce: out must be contiguous float64 [", lnscale ? "" : "C, ", info.tiles, ", ", W, "]");
    const c10::DeviceGuard guard(dev);
    void *const hip_stream = reinterpret_cast<void *>(static_cast<uintptr_t>(stream));
    const uint32_t *cnt = static_cast<const uint32_t *>(counts.const_data_ptr());
    const wgrt_visit_end *e = static_cast<const wgrt_visit_end *>(ends.const_data_ptr());
    if (!lnscale) return visits_abi().sensitivity(s, wp, cnt, e, n_rows, out.data_ptr<double>(), hip_stream);
    TORCH_CHECK(lnscale->device() == dev && lnscale->scalar_type() == at::kDouble && lnscale->is_contiguous() &&
                    lnscale->numel() == C,
                "wgrt.visits_reduce: lnscale must be contiguous float64 [", C, "] on the scene's device");
    return visits_abi().reweight(s, wp, cnt, e, n_rows, lnscale->const_data_ptr<double>(), out.data_ptr<double>(),
                                 hip_stream);
}

// paths_footprint: the first n records of a path list added into a footprint map on the list's device
// (wgrt_paths_footprint).
int64_t paths_footprint(const Tensor &paths, int64_t n, int64_t num_lmd, double fp_x0, double fp_y0, double fp_cell_x,
                        double fp_cell_y, int64_t fp_nx_cells, int64_t fp_ny_cells, Tensor map, int64_t stream) {
    TORCH_CHECK(paths.is_cuda() && map.is_cuda() && paths.device() == map.device(),
                "wgrt.paths_footprint: the list and the map must be on one GPU");
    TORCH_CHECK(paths.scalar_type() == at::kByte && paths.is_contiguous(), "wgrt.paths_footprint: the list must be contiguous uint8");
    TORCH_CHECK(n >= 0 && n <= paths.numel() / (int64_t)sizeof(wgrt_path_vertex), "wgrt.paths_footprint: n = ", n,
                " exceeds the buffer's ", paths.numel() / (int64_t)sizeof(wgrt_path_vertex), " records");
    wgrt_footprint_plan fp{};
    fp.x0 = fp_x0;
    fp.y0 = fp_y0;
    fp.cell_x = fp_cell_x;
    fp.cell_y = fp_cell_y;
    fp.nx_cells = static_cast<int32_t>(std::max<int64_t>(-1, std::min<int64_t>(fp_nx_cells, 1 << 20)));
    fp.ny_cells = static_cast<int32_t>(std::max<int64_t>(-1, std::min<int64_t>(fp_ny_cells, 1 << 20)));
    const bool sized = fp.nx_cells >= 1 && fp.nx_cells <= 4096 && fp.ny_cells >= 1 && fp.ny_cells <= 4096;
    TORCH_CHECK(map.scalar_type() == at::kLong, "wgrt.paths_footprint: map must be int64");
    TORCH_CHECK(!sized || num_lmd < 1 ||
                    (map.is_contiguous() && map.dim() == 4 && map.size(0) == num_lmd &&
                     map.size(1) == WGRT_FOOTPRINT_CHANNELS && map.size(2) == fp.ny_cells && map.size(3) == fp.nx_cells),
                "wgrt.paths_footprint: map must be contiguous [", num_lmd, ", ", WGRT_FOOTPRINT_CHANNELS, ", ", fp.ny_cells,
                ", ", fp.nx_cells, "], got ", map.sizes());
    const c10::DeviceGuard guard(paths.device());
    return paths_abi().footprint(static_cast<const wgrt_path_vertex *>(paths.const_data_ptr()), n,
                                 static_cast<int32_t>(std::max<int64_t>(-1, std::min<int64_t>(num_lmd, 1 << 20))), &fp,
                                 static_cast<int64_t *>(map.data_ptr()), reinterpret_cast<void *>(static_cast<uintptr_t>(stream)));
}

// chain_begin: trace_windows' arguments -> the chain's handle (a user-space address: positive), or the negated
// wgrt_status of a failure (wgrt_last_error has the detail).  The
// Python layer keeps every tensor alive until chain_end (engine.TraceChain).
int64_t chain_begin(int64_t scene, const Tensor &x, const Tensor &y, const Tensor &m, const Tensor &n,
                    const std::optional<Tensor> &lmd_num, const Tensor &te, const Tensor &tm, const Tensor &delta_phase,
                    Tensor rng_states, std::optional<Tensor> matrix_EB, std::optional<Tensor> stats,
                    std::optional<Tensor> per_ray_bounces, int64_t n_rays, int64_t gid_offset, int64_t stream,
                    int64_t kernel, int64_t variant, int64_t workgroups, const std::optional<Tensor> &chunk_order,
                    int64_t num_iter, const std::optional<Tensor> &gid_blocks, int64_t gid_block_rays, int64_t debug,
                    double grid_sqrt_k, int64_t plan, std::optional<Tensor> table) {
    wgrt_chain *ch = nullptr;
    const int64_t st = trace_core(scene, x, y, m, n, lmd_num, te, tm, delta_phase, rng_states, matrix_EB, stats,
                                  per_ray_bounces, n_rays, gid_offset, stream, kernel, variant, workgroups, chunk_order,
                                  num_iter, gid_blocks, gid_block_rays, debug, grid_sqrt_k, plan, table, &ch);
    return st == WGRT_OK ? static_cast<int64_t>(reinterpret_cast<uintptr_t>(ch)) : -st;
}
int64_t chain_step(int64_t chain) {
    return chain_abi().step(reinterpret_cast<wgrt_chain *>(static_cast<uintptr_t>(chain)));
}
int64_t chain_end(int64_t chain) {
    return chain_abi().end(reinterpret_cast<wgrt_chain *>(static_cast<uintptr_t>(chain)));
}

int64_t trace(int64_t scene, const Tensor &x, const Tensor &y, const Tensor &m, const Tensor &n,
              const std::optional<Tensor> &lmd_num, const Tensor &te, const Tensor &tm, const Tensor &delta_phase,
              Tensor rng_states, Tensor matrix_EB, std::optional<Tensor> stats, std::optional<Tensor> per_ray_bounces,
              int64_t n_rays, int64_t gid_offset, int64_t stream, int64_t kernel, int64_t variant, int64_t workgroups,
              const std::optional<Tensor> &chunk_order, int64_t num_iter, const std::optional<Tensor> &gid_blocks,
              int64_t gid_block_rays, int64_t debug, double grid_sqrt_k) {
    return trace_impl(scene, x, y, m, n, lmd_num, te, tm, delta_phase, rng_states, matrix_EB, stats, per_ray_bounces,
                      n_rays, gid_offset, stream, kernel, variant, workgroups, chunk_order, num_iter, gid_blocks,
                      gid_block_rays, debug, grid_sqrt_k, 0, std::nullopt);
}

}  // namespace

TORCH_LIBRARY(wgrt, m) {
    m.def("trace(int scene, Tensor x, Tensor y, Tensor m, Tensor n, Tensor? lmd_num, Tensor te, Tensor tm, "
          "Tensor delta_phase, Tensor(a!) rng_states, Tensor(b!) matrix_EB, Tensor(c!)? stats, "
          "Tensor(d!)? per_ray_bounces, int n_rays, int gid_offset, int stream, int kernel, int variant, "
          "int workgroups, Tensor? chunk_order, int num_iter, Tensor? gid_blocks, int gid_block_rays, int debug, "
          "float grid_sqrt_k) -> int",
          &trace);
    // the same launch with the window table as a second sink (wgrt_trace_windows): matrix_EB optional, plan a
    // wgrt_window_plan handle, table float64 [tiles, W]
    m.def("trace_windows(int scene, Tensor x, Tensor y, Tensor m, Tensor n, Tensor? lmd_num, Tensor te, Tensor tm, "
          "Tensor delta_phase, Tensor(a!) rng_states, Tensor(b!)? matrix_EB, Tensor(c!)? stats, "
          "Tensor(d!)? per_ray_bounces, int n_rays, int gid_offset, int stream, int kernel, int variant, "
          "int workgroups, Tensor? chunk_order, int num_iter, Tensor? gid_blocks, int gid_block_rays, int debug, "
          "float grid_sqrt_k, int plan, Tensor(e!)? table) -> int",
          &trace_impl);
    // a chain of single launches (wgrt_chain_*): begin takes trace_windows' arguments and returns the handle
    m.def("chain_begin(int scene, Tensor x, Tensor y, Tensor m, Tensor n, Tensor? lmd_num, Tensor te, Tensor tm, "
          "Tensor delta_phase, Tensor(a!) rng_states, Tensor(b!)? matrix_EB, Tensor(c!)? stats, "
          "Tensor(d!)? per_ray_bounces, int n_rays, int gid_offset, int stream, int kernel, int variant, "
          "int workgroups, Tensor? chunk_order, int num_iter, Tensor? gid_blocks, int gid_block_rays, int debug, "
          "float grid_sqrt_k, int plan, Tensor(e!)? table) -> int",
          &chain_begin);
    // the same launch storing every ray's fate code (wgrt_trace_fate): fate uint8 [rays]
    m.def("trace_fate(int scene, Tensor x, Tensor y, Tensor m, Tensor n, Tensor? lmd_num, Tensor te, Tensor tm, "
          "Tensor delta_phase, Tensor(a!) rng_states, Tensor(b!)? matrix_EB, Tensor(c!)? stats, "
          "Tensor(d!)? per_ray_bounces, int n_rays, int gid_offset, int stream, int kernel, int variant, "
          "int workgroups, Tensor? chunk_order, int num_iter, Tensor? gid_blocks, int gid_block_rays, int debug, "
          "float grid_sqrt_k, int plan, Tensor(e!)? table, Tensor(f!) fate) -> int",
          &trace_fate);
    // the same launch into replica window tables (wgrt_trace_replicas): table float64 [replicas, tiles, W]
    m.def("trace_replicas(int scene, Tensor x, Tensor y, Tensor m, Tensor n, Tensor? lmd_num, Tensor te, Tensor tm, "
          "Tensor delta_phase, Tensor(a!) rng_states, Tensor(b!)? matrix_EB, Tensor(c!)? stats, "
          "Tensor(d!)? per_ray_bounces, int n_rays, int gid_offset, int stream, int kernel, int variant, "
          "int workgroups, Tensor? chunk_order, int num_iter, Tensor? gid_blocks, int gid_block_rays, int debug, "
          "float grid_sqrt_k, int plan, Tensor(e!)? table, int replicas) -> int",
          &trace_replicas);
    // the expected-value estimator (wgrt_trace_expected): no grid; table float64 [tiles, W] or [replicas, tiles, W]
    m.def("trace_expected(int scene, Tensor x, Tensor y, Tensor m, Tensor n, Tensor? lmd_num, Tensor te, Tensor tm, "
          "Tensor delta_phase, Tensor(a!) rng_states, Tensor(c!)? stats, Tensor(d!)? per_ray_bounces, int n_rays, "
          "int gid_offset, int stream, int kernel, int variant, int workgroups, Tensor? chunk_order, int num_iter, "
          "Tensor? gid_blocks, int gid_block_rays, int debug, float grid_sqrt_k, int plan, Tensor(e!) table, "
          "int replicas) -> int",
          &trace_expected);
    // the same launch counting every draw into the footprint maps (wgrt_trace_footprint): map int64
    // [num_lmd, 9, ny_cells, nx_cells]
    m.def("trace_footprint(int scene, Tensor x, Tensor y, Tensor m, Tensor n, Tensor? lmd_num, Tensor te, Tensor tm, "
          "Tensor delta_phase, Tensor(a!) rng_states, Tensor(b!)? matrix_EB, Tensor(c!)? stats, "
          "Tensor(d!)? per_ray_bounces, int n_rays, int gid_offset, int stream, int kernel, int variant, "
          "int workgroups, Tensor? chunk_order, int num_iter, Tensor? gid_blocks, int gid_block_rays, int debug, "
          "float grid_sqrt_k, int plan, Tensor(e!)? table, float fp_x0, float fp_y0, float fp_cell_x, float fp_cell_y, "
          "int fp_nx_cells, int fp_ny_cells, Tensor(f!) map) -> int",
          &trace_footprint);
    // the same launch appending one record per out-coupling to a hit list (wgrt_trace_hits): hits uint8, 32 bytes
    // per record, capacity in records; count int64[1], added to
    m.def("trace_hits(int scene, Tensor x, Tensor y, Tensor m, Tensor n, Tensor? lmd_num, Tensor te, Tensor tm, "
          "Tensor delta_phase, Tensor(a!) rng_states, Tensor(b!)? matrix_EB, Tensor(c!)? stats, "
          "Tensor(d!)? per_ray_bounces, int n_rays, int gid_offset, int stream, int kernel, int variant, "
          "int workgroups, Tensor? chunk_order, int num_iter, Tensor? gid_blocks, int gid_block_rays, int debug, "
          "float grid_sqrt_k, int plan, Tensor(e!)? table, Tensor(f!) hits, int capacity, Tensor(g!)? count, int tag) -> int",
          &trace_hits);
    // the same launch appending one record per draw of the selected rays to a path list (wgrt_trace_paths): paths uint8,
    // 32 bytes per record, capacity in records; count int64[1], added to; select uint8 [n_rays] or None (every ray)
    m.def("trace_paths(int scene, Tensor x, Tensor y, Tensor m, Tensor n, Tensor? lmd_num, Tensor te, Tensor tm, "
          "Tensor delta_phase, Tensor(a!) rng_states, Tensor(b!)? matrix_EB, Tensor(c!)? stats, "
          "Tensor(d!)? per_ray_bounces, int n_rays, int gid_offset, int stream, int kernel, int variant, "
          "int workgroups, Tensor? chunk_order, int num_iter, Tensor? gid_blocks, int gid_block_rays, int debug, "
          "float grid_sqrt_k, int plan, Tensor(e!)? table, Tensor(f!) paths, int capacity, Tensor(g!)? count, int tag, "
          "Tensor? select) -> int",
          &trace_paths);
    // a path list's first n records added into a footprint map (wgrt_paths_footprint)
    m.def("paths_footprint(Tensor paths, int n, int num_lmd, float fp_x0, float fp_y0, float fp_cell_x, float fp_cell_y, "
          "int fp_nx_cells, int fp_ny_cells, Tensor(a!) map, int stream) -> int",
          &paths_footprint);
    // the same launch counting the taken branches of the counted rays (wgrt_trace_visits): slot int32 [n_rays] or None (ray
    // i into row i), counts int32 [n_rows, C] added to, ends uint8 [n_rows, 32]
    m.def("trace_visits(int scene, Tensor x, Tensor y, Tensor m, Tensor n, Tensor? lmd_num, Tensor te, Tensor tm, "
          "Tensor delta_phase, Tensor(a!) rng_states, Tensor(b!)? matrix_EB, Tensor(c!)? stats, "
          "Tensor(d!)? per_ray_bounces, int n_rays, int gid_offset, int stream, int kernel, int variant, "
          "int workgroups, Tensor? chunk_order, int num_iter, Tensor? gid_blocks, int gid_block_rays, int debug, "
          "float grid_sqrt_k, int plan, Tensor(e!)? table, Tensor? slot, int n_rows, Tensor(f!) counts, Tensor(g!) ends) "
          "-> int",
          &trace_visits);
    // a visits table reduced into sensitivity tables (lnscale None) or a re-weighted window table
    m.def("visits_reduce(int scene, int plan, Tensor counts, Tensor ends, int n_rows, Tensor? lnscale, Tensor(a!) out, "
          "int stream) -> int",
          &visits_reduce);
    m.def("chain_step(int chain) -> int", &chain_step);
    m.def("chain_end(int chain) -> int", &chain_end);
}
