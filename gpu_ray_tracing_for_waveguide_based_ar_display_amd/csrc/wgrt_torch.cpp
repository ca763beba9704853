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
#include <string>
#include <variant>

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

// An entry point of the loaded libwgrt.so (global scope) that arrived within ABI 9, looked up by name at its first
// use (as _lib.load binds them): the operator library still loads over an earlier build, where the call raises.
// `lead` is the launching operator the entry point came with, `since` what that build is from before.
template <class Fn>
Fn lib_symbol(const char *name, const char *lead, const char *since) {
    const Fn fn = reinterpret_cast<Fn>(dlsym(RTLD_DEFAULT, name));
    TORCH_CHECK(fn, "wgrt.", lead, ": the loaded libwgrt.so has no wgrt_", lead, " (a build from before ", since, ")");
    return fn;
}
#define WGRT_SYM(fn, lead, since) \
    ([] { static const auto f = lib_symbol<decltype(&fn)>(#fn, lead, since); return f; }())
#define WINDOW_SYM(fn) WGRT_SYM(fn, "trace_windows", "the window-table sink")
#define CHAIN_SYM(fn) WGRT_SYM(fn, "chain_begin", "the chained launches")
#define PATHS_SYM(fn) WGRT_SYM(fn, "trace_paths", "the ray paths")
#define VISITS_SYM(fn) WGRT_SYM(fn, "trace_visits", "the visit counts")

// The arguments every launching operator shares, in the schemas' order, written once: as parameters, as the record
// trace_core takes, and as that record's initialiser.  (trace has no plan / table and trace_expected no matrix_EB:
// they declare the missing ones as locals.)
#define TRACE_HEAD_PARAMS                                                                                        \
    int64_t scene, const Tensor &x, const Tensor &y, const Tensor &m, const Tensor &n,                           \
        const std::optional<Tensor> &lmd_num, const Tensor &te, const Tensor &tm, const Tensor &delta_phase,     \
        Tensor rng_states
#define TRACE_TAIL_PARAMS                                                                                        \
    std::optional<Tensor> stats, std::optional<Tensor> per_ray_bounces, int64_t n_rays, int64_t gid_offset,      \
        int64_t stream, int64_t kernel, int64_t variant, int64_t workgroups,                                     \
        const std::optional<Tensor> &chunk_order, int64_t num_iter, const std::optional<Tensor> &gid_blocks,     \
        int64_t gid_block_rays, int64_t debug, double grid_sqrt_k
#define TRACE_PARAMS \
    TRACE_HEAD_PARAMS, std::optional<Tensor> matrix_EB, TRACE_TAIL_PARAMS, int64_t plan, std::optional<Tensor> table
#define TRACE_COMMON                                                                                             \
    Common {                                                                                                     \
        scene, x, y, m, n, lmd_num, te, tm, delta_phase, rng_states, matrix_EB, stats, per_ray_bounces, n_rays,  \
            gid_offset, stream, kernel, variant, workgroups, chunk_order, num_iter, gid_blocks, gid_block_rays,  \
            debug, grid_sqrt_k, plan, table                                                                      \
    }
struct Common {
    int64_t scene;
    const Tensor &x, &y, &m, &n;
    const std::optional<Tensor> &lmd_num;
    const Tensor &te, &tm, &delta_phase, &rng_states;
    const std::optional<Tensor> &matrix_EB, &stats, &per_ray_bounces;
    int64_t n_rays, gid_offset, stream, kernel, variant, workgroups;
    const std::optional<Tensor> &chunk_order;
    int64_t num_iter;
    const std::optional<Tensor> &gid_blocks;
    int64_t gid_block_rays, debug;
    double grid_sqrt_k;
    int64_t plan;
    const std::optional<Tensor> &table;
};

// What a launching operator adds to the shared arguments: its one sink's tensors (engine._launch_sink states the
// rule), the replica count of a launch into replica tables, or the chain a chain_begin opens.
struct NoSink {};   // trace, trace_windows
struct ChainSink {
    wgrt_chain **out;
};
struct FateSink {   // uint8 [rays]
    const Tensor &fate;
};
struct ReplicasSink {   // table float64 [replicas, tiles, W] for replicas >= 2
    int64_t replicas;
};
struct ExpectedSink {   // the same, no grid
    int64_t replicas;
};
struct FootprintSink {   // int64 [num_lmd, 9, ny_cells, nx_cells]
    wgrt_footprint_plan fp;
    const Tensor &map;
};
struct HitsSink {   // the record buffer (uint8, 32 bytes per record), its capacity in records, the counter and the tag
    const Tensor &list;
    int64_t capacity;
    const std::optional<Tensor> &count;
    int64_t tag;
};
struct PathsSink {   // the same over a path list, and the batch's select bytes
    HitsSink list;
    const std::optional<Tensor> &select;
};
struct VisitsSink {   // slot int32 [n_rays] or none, counts int32 [n_rows, C] (the library's uint32 words), ends uint8 [n_rows, 32]
    const std::optional<Tensor> &slot;
    int64_t n_rows;
    const Tensor &counts, &ends;
};
struct StokesSink {   // int64 [3, tiles, W], beside the window table
    const Tensor &stokes;
};
using OpSink = std::variant<NoSink, ChainSink, FateSink, ReplicasSink, ExpectedSink, FootprintSink, HitsSink, PathsSink, VisitsSink,
                            StokesSink>;

// The footprint plan of an operator's six fp_* arguments (out of int32 range: a count the library refuses).
wgrt_footprint_plan footprint_plan_of(double x0, double y0, double cell_x, double cell_y, int64_t nx_cells, int64_t ny_cells) {
    wgrt_footprint_plan fp{};
    fp.x0 = x0;
    fp.y0 = y0;
    fp.cell_x = cell_x;
    fp.cell_y = cell_y;
    fp.nx_cells = static_cast<int32_t>(std::max<int64_t>(-1, std::min<int64_t>(nx_cells, 1 << 20)));
    fp.ny_cells = static_cast<int32_t>(std::max<int64_t>(-1, std::min<int64_t>(ny_cells, 1 << 20)));
    return fp;
}

// A footprint map against its plan: int64, contiguous [num_lmd, 9, ny_cells, nx_cells].  With the scene's tile count,
// num_lmd * nx * ny, the first axis divides it (trace_footprint: the Python layer checks it exactly); else it is num_lmd.
// (a plan or a wavelength count the library refuses has no size to compare with: the library's check answers first)
void check_footprint_map(const char *op, const Tensor &map, const wgrt_footprint_plan &fp, int64_t num_lmd, int64_t tiles) {
    TORCH_CHECK(map.scalar_type() == at::kLong, op, ": map must be int64");
    const bool sized = fp.nx_cells >= 1 && fp.nx_cells <= 4096 && fp.ny_cells >= 1 && fp.ny_cells <= 4096;
    if (!sized || (!tiles && num_lmd < 1)) return;
    const bool first = map.dim() == 4 && (tiles ? map.size(0) >= 1 && tiles % map.size(0) == 0 : map.size(0) == num_lmd);
    TORCH_CHECK(first && map.is_contiguous() && map.size(1) == WGRT_FOOTPRINT_CHANNELS && map.size(2) == fp.ny_cells &&
                    map.size(3) == fp.nx_cells,
                op, ": map must be contiguous [", tiles ? "num_lmd" : std::to_string(num_lmd), ", ", WGRT_FOOTPRINT_CHANNELS,
                ", ", fp.ny_cells, ", ", fp.nx_cells, "], got ", map.sizes());
}

// A record list (trace_hits / trace_paths; both hold 32-byte records) against its capacity: the counter and the tag.
struct RecordList {
    void *buf;
    uint64_t *count;
    uint32_t tag;
};
RecordList record_list(const char *op, const HitsSink &k, const Ctx &c) {
    static_assert(sizeof(wgrt_hit) == sizeof(wgrt_path_vertex), "both lists hold 32-byte records");
    on_device(k.list, "list", c);
    TORCH_CHECK(k.list.scalar_type() == at::kByte && k.list.is_contiguous(), op, ": the list must be contiguous uint8");
    // (a negative capacity is the library's to refuse; a positive one must lie inside the buffer)
    TORCH_CHECK(k.capacity <= 0 || k.capacity <= k.list.numel() / (int64_t)sizeof(wgrt_hit), op, ": capacity ", k.capacity,
                " exceeds the buffer's ", k.list.numel() / (int64_t)sizeof(wgrt_hit), " records");
    uint64_t *cnt = nullptr;
    if (k.count) {
        on_device(*k.count, "count", c);
        TORCH_CHECK(k.count->scalar_type() == at::kLong && k.count->numel() == 1, op, ": count must be int64[1]");
        cnt = static_cast<uint64_t *>(k.count->data_ptr());
    }
    // (out of uint32 range: a tag the library refuses)
    return {k.list.data_ptr(), cnt, k.tag < 0 || k.tag > 0xffffffffll ? 0xffffffffu : static_cast<uint32_t>(k.tag)};
}

// Every launching operator: the shared arguments checked against the scene and made into the library's records, then
// the sink's own tensors checked and the sink's entry point called -- wgrt_trace_opts / wgrt_trace_windows without one,
// wgrt_chain_begin (which launches nothing and leaves the chain's handle) for a ChainSink.
int64_t trace_core(const Common &a, const OpSink &sink) {
    const wgrt_scene *s = reinterpret_cast<const wgrt_scene *>(static_cast<uintptr_t>(a.scene));
    TORCH_CHECK(s != nullptr, "wgrt.trace: NULL scene");
    wgrt_scene_info info{};
    const wgrt_status st = wgrt_scene_get_info(s, &info);
    if (st != WGRT_OK) return st;
    const Ctx c{c10::Device(c10::DeviceType::CUDA, static_cast<c10::DeviceIndex>(info.device)), a.x.numel()};
    // the scene's device is current for the call (the library selects it too, include/wgrt.h) and the
    // caller's comes back on return
    const c10::DeviceGuard guard(c.dev);
    const int64_t n_rays = a.n_rays;
    TORCH_CHECK(n_rays >= 0 && n_rays <= c.rays, "wgrt.trace: n_rays=", n_rays, " out of range for ", c.rays, " rays");
    TORCH_CHECK(a.kernel == 0 || a.kernel == 1, "wgrt.trace: kernel must be 0 (full colour) or 1 (single wavelength)");

    wgrt_rays r{};
    r.x = column(a.x, "x", c);
    r.y = column(a.y, "y", c);
    r.m = column(a.m, "m", c);
    r.n = column(a.n, "n", c);
    if (a.kernel == 0) {
        TORCH_CHECK(a.lmd_num.has_value(), "wgrt.trace: the full-colour kernel needs lmd_num");
        r.lmd_num = column(*a.lmd_num, "lmd_num", c);
    }
    r.te = column(a.te, "te", c);
    r.tm = column(a.tm, "tm", c);
    r.delta_phase = column(a.delta_phase, "delta_phase", c);

    uint32_t *rng = static_cast<uint32_t *>(u32(a.rng_states, "rng_states", c, c.rays));
    TORCH_CHECK(a.matrix_EB.has_value() || a.table.has_value(), "wgrt.trace: needs matrix_EB, a window table, or both");
    float *eb = nullptr;
    if (a.matrix_EB) {
        on_device(*a.matrix_EB, "matrix_EB", c);
        TORCH_CHECK(a.matrix_EB->scalar_type() == at::kFloat, "wgrt.trace: matrix_EB must be float32");
        const int64_t eb_want = (int64_t)info.tiles * 80 * 120;   // [L,] NY, NX, 80, 120
        TORCH_CHECK(a.matrix_EB->numel() == eb_want, "wgrt.trace: matrix_EB holds ", a.matrix_EB->numel(),
                    " floats, the scene's grid has ", eb_want);
        eb = a.matrix_EB->data_ptr<float>();
    }
    const wgrt_window_plan *wp = reinterpret_cast<const wgrt_window_plan *>(static_cast<uintptr_t>(a.plan));
    // the replica count describes the table: trace_replicas' and trace_expected's (the library checks its range)
    const ReplicasSink *const reps = std::get_if<ReplicasSink>(&sink);
    const ExpectedSink *const expected = std::get_if<ExpectedSink>(&sink);
    const int64_t replicas = reps ? reps->replicas : expected ? expected->replicas : 0;
    double *tab = nullptr;
    if (a.table) {
        const Tensor &table = *a.table;
        const int64_t W = WINDOW_SYM(wgrt_window_plan_width)(wp);
        TORCH_CHECK(W > 0, "wgrt.trace: a window table needs its plan");
        on_device(table, "table", c);
        TORCH_CHECK(table.scalar_type() == at::kDouble, "wgrt.trace: table must be float64");
        if (replicas >= 2) {   // one table per replica
            TORCH_CHECK(table.dim() == 3 && table.size(0) == replicas && table.size(1) == info.tiles && table.size(2) == W,
                        "wgrt.trace_replicas: table must have shape [", replicas, ", ", info.tiles, ", ", W, "], got ",
                        table.sizes());
        } else {
            TORCH_CHECK(table.dim() == 2 && table.size(0) == info.tiles && table.size(1) == W,
                        "wgrt.trace: table must have shape [", info.tiles, ", ", W, "], got ", table.sizes());
        }
        tab = table.data_ptr<double>();
    }
    wgrt_trace_stats *stp = nullptr;
    if (a.stats) {
        on_device(*a.stats, "stats", c);
        TORCH_CHECK(a.stats->scalar_type() == at::kLong && a.stats->numel() * 8 == (int64_t)sizeof(wgrt_trace_stats),
                    "wgrt.trace: stats must be int64[", sizeof(wgrt_trace_stats) / 8, "]");
        stp = static_cast<wgrt_trace_stats *>(a.stats->data_ptr());
    }
    uint32_t *per = a.per_ray_bounces ? static_cast<uint32_t *>(u32(*a.per_ray_bounces, "per_ray_bounces", c, c.rays))
                                      : nullptr;

    wgrt_launch_opts o{};
    o.kernel = (int)a.kernel;
    o.variant = (int)a.variant;
    o.workgroups = (int)a.workgroups;
    if (a.chunk_order) {
        on_device(*a.chunk_order, "chunk_order", c);
        const int64_t chunks = (n_rays + 63) / 64;
        TORCH_CHECK(a.chunk_order->scalar_type() == at::kInt && a.chunk_order->numel() == chunks,
                    "wgrt.trace: chunk_order must be int32[", chunks, "]");
        o.chunk_order = static_cast<const int32_t *>(a.chunk_order->const_data_ptr());
        o.n_chunk_order = chunks;
    }
    o.num_iter = (int)a.num_iter;
    if (a.gid_blocks) {
        on_device(*a.gid_blocks, "gid_blocks", c);
        TORCH_CHECK(a.gid_block_rays >= 1, "wgrt.trace: gid_blocks needs gid_block_rays >= 1");
        const int64_t blocks = (n_rays + a.gid_block_rays - 1) / a.gid_block_rays;
        TORCH_CHECK(a.gid_blocks->scalar_type() == at::kLong && a.gid_blocks->numel() >= blocks,
                    "wgrt.trace: gid_blocks must be int64 with >= ", blocks, " entries");
        o.gid_blocks = static_cast<const int64_t *>(a.gid_blocks->const_data_ptr());
        o.gid_block_rays = a.gid_block_rays;
    }
    // test / profiling hooks: the address of a wgrt_debug_opts record the caller keeps alive (0: none)
    o.debug = reinterpret_cast<const wgrt_debug_opts *>(static_cast<uintptr_t>(a.debug));
    o.grid_sqrt_k = a.grid_sqrt_k;
    void *const hip_stream = reinterpret_cast<void *>(static_cast<uintptr_t>(a.stream));
    // an entry point over trace_windows' arguments and the sink's own
    auto launch = [&](auto fn, auto... own) {
        return fn(s, &r, n_rays, a.gid_offset, rng, eb, stp, per, hip_stream, &o, tab ? wp : nullptr, tab, own...);
    };
    const int clamped = static_cast<int>(std::max<int64_t>(-1, std::min<int64_t>(replicas, 1 << 20)));

    if (const auto *k = std::get_if<ChainSink>(&sink)) {
        TORCH_CHECK(!per, "wgrt.chain_begin: a chain takes no per_ray_bounces");
        return CHAIN_SYM(wgrt_chain_begin)(s, &r, n_rays, a.gid_offset, rng, eb, stp, hip_stream, &o, tab ? wp : nullptr, tab,
                                           k->out);
    }
    if (const auto *k = std::get_if<VisitsSink>(&sink)) {
        const int64_t C = VISITS_SYM(wgrt_visit_channels)(s);
        on_device(k->counts, "counts", c);
        on_device(k->ends, "ends", c);
        // (a negative n_rows is the library's to refuse; the rows must lie inside both buffers)
        TORCH_CHECK(k->counts.scalar_type() == at::kInt && k->counts.is_contiguous() &&
                        k->counts.numel() >= std::max<int64_t>(k->n_rows, 0) * C,
                    "wgrt.trace_visits: counts must be contiguous int32 with >= n_rows * ", C, " entries");
        TORCH_CHECK(k->ends.scalar_type() == at::kByte && k->ends.is_contiguous() &&
                        k->ends.numel() >= std::max<int64_t>(k->n_rows, 0) * (int64_t)sizeof(wgrt_visit_end),
                    "wgrt.trace_visits: ends must be contiguous uint8 with >= n_rows * 32 bytes");
        const int32_t *slot = nullptr;
        if (k->slot) {
            on_device(*k->slot, "slot", c);
            TORCH_CHECK(k->slot->scalar_type() == at::kInt && k->slot->is_contiguous() && k->slot->numel() >= n_rays,
                        "wgrt.trace_visits: slot must be contiguous int32 with >= ", n_rays, " entries");
            slot = static_cast<const int32_t *>(k->slot->const_data_ptr());
        }
        return launch(VISITS_SYM(wgrt_trace_visits), slot, k->n_rows, static_cast<uint32_t *>(k->counts.data_ptr()),
                      static_cast<wgrt_visit_end *>(k->ends.data_ptr()));
    }
    if (const auto *k = std::get_if<StokesSink>(&sink)) {   // added to by every out-coupling the window table counts
        on_device(k->stokes, "stokes", c);
        TORCH_CHECK(tab, "wgrt.trace_stokes: the Stokes tables lie beside a window table: the launch needs the table and "
                         "its plan");
        const int64_t W = WINDOW_SYM(wgrt_window_plan_width)(wp);
        TORCH_CHECK(k->stokes.scalar_type() == at::kLong && k->stokes.is_contiguous() && k->stokes.dim() == 3 &&
                        k->stokes.size(0) == 3 && k->stokes.size(1) == info.tiles && k->stokes.size(2) == W,
                    "wgrt.trace_stokes: stokes must be contiguous int64 [3, ", info.tiles, ", ", W, "], got ",
                    k->stokes.sizes());
        return launch(WGRT_SYM(wgrt_trace_stokes, "trace_stokes", "the Stokes tables"),
                      static_cast<int64_t *>(k->stokes.data_ptr()));
    }
    if (const auto *k = std::get_if<PathsSink>(&sink)) {
        const RecordList l = record_list("wgrt.trace_paths", k->list, c);
        const uint8_t *sel = nullptr;
        if (k->select) {
            const Tensor &select = *k->select;
            on_device(select, "select", c);
            TORCH_CHECK(select.scalar_type() == at::kByte && select.is_contiguous() && select.numel() >= n_rays,
                        "wgrt.trace_paths: select must be contiguous uint8 with >= ", n_rays, " entries");
            sel = static_cast<const uint8_t *>(select.const_data_ptr());
        }
        return launch(PATHS_SYM(wgrt_trace_paths), static_cast<wgrt_path_vertex *>(l.buf), k->list.capacity, l.count, l.tag,
                      sel);
    }
    if (const auto *k = std::get_if<HitsSink>(&sink)) {
        const RecordList l = record_list("wgrt.trace_hits", *k, c);
        return launch(WGRT_SYM(wgrt_trace_hits, "trace_hits", "the hit list"), static_cast<wgrt_hit *>(l.buf), k->capacity,
                      l.count, l.tag);
    }
    if (const auto *k = std::get_if<FootprintSink>(&sink)) {   // added to by every counted draw
        on_device(k->map, "map", c);
        check_footprint_map("wgrt.trace_footprint", k->map, k->fp, 0, info.tiles);
        return launch(WGRT_SYM(wgrt_trace_footprint, "trace_footprint", "the footprint maps"), &k->fp,
                      static_cast<int64_t *>(k->map.data_ptr()));
    }
    if (expected)   // the window table alone (its shape checked above: [tiles, W], or one per replica)
        return WGRT_SYM(wgrt_trace_expected, "trace_expected", "the expected-value estimator")(
            s, &r, n_rays, a.gid_offset, rng, stp, per, hip_stream, &o, wp, tab, clamped);
    if (reps && replicas != 0)   // (0: the call is trace_windows, below)
        return launch(WGRT_SYM(wgrt_trace_replicas, "trace_replicas", "the replica tables"), clamped);
    if (const auto *k = std::get_if<FateSink>(&sink)) {   // one uint8 per ray of the batch, written by the lane that ends
        on_device(k->fate, "fate", c);                    // the ray's trace
        TORCH_CHECK(k->fate.scalar_type() == at::kByte, "wgrt.trace_fate: fate must be uint8");
        TORCH_CHECK(k->fate.numel() == c.rays, "wgrt.trace_fate: fate holds ", k->fate.numel(), " entries, the batch has ",
                    c.rays);
        return launch(WGRT_SYM(wgrt_trace_fate, "trace_fate", "the ray fates"), static_cast<uint8_t *>(k->fate.data_ptr()));
    }
    if (!tab) return wgrt_trace_opts(s, &r, n_rays, a.gid_offset, rng, eb, stp, per, hip_stream, &o);
    return WINDOW_SYM(wgrt_trace_windows)(s, &r, n_rays, a.gid_offset, rng, eb, stp, per, hip_stream, &o, wp, tab);
}

// trace_windows: the grid, the window table of plan `plan` -- a wgrt_window_plan handle -- or both.
int64_t trace_impl(TRACE_PARAMS) { return trace_core(TRACE_COMMON, NoSink{}); }

// trace: the grid alone (plan 0, no table).
int64_t trace(TRACE_HEAD_PARAMS, Tensor grid, TRACE_TAIL_PARAMS) {
    const std::optional<Tensor> matrix_EB(std::move(grid)), table;
    const int64_t plan = 0;
    return trace_core(TRACE_COMMON, NoSink{});
}

// chain_begin: trace_windows' arguments -> the chain's handle (a user-space address: positive), or the negated
// wgrt_status of a failure (wgrt_last_error has the detail).  The
// Python layer keeps every tensor alive until chain_end (engine.TraceChain).
int64_t chain_begin(TRACE_PARAMS) {
    wgrt_chain *ch = nullptr;
    const int64_t st = trace_core(TRACE_COMMON, ChainSink{&ch});
    return st == WGRT_OK ? static_cast<int64_t>(reinterpret_cast<uintptr_t>(ch)) : -st;
}
int64_t chain_step(int64_t chain) {
    return CHAIN_SYM(wgrt_chain_step)(reinterpret_cast<wgrt_chain *>(static_cast<uintptr_t>(chain)));
}
int64_t chain_end(int64_t chain) {
    return CHAIN_SYM(wgrt_chain_end)(reinterpret_cast<wgrt_chain *>(static_cast<uintptr_t>(chain)));
}

// trace_fate: trace_windows' arguments and the fate buffer (wgrt_trace_fate).
int64_t trace_fate(TRACE_PARAMS, Tensor fate) { return trace_core(TRACE_COMMON, FateSink{fate}); }

// trace_replicas: trace_windows' arguments and the replica count (wgrt_trace_replicas).
int64_t trace_replicas(TRACE_PARAMS, int64_t replicas) { return trace_core(TRACE_COMMON, ReplicasSink{replicas}); }

// trace_expected: trace_replicas' arguments without the grid (wgrt_trace_expected): table float64 [tiles, W] for
// replicas 0 / 1, [replicas, tiles, W] otherwise.
int64_t trace_expected(TRACE_HEAD_PARAMS, TRACE_TAIL_PARAMS, int64_t plan, Tensor window_table, int64_t replicas) {
    const std::optional<Tensor> matrix_EB, table(std::move(window_table));
    return trace_core(TRACE_COMMON, ExpectedSink{replicas});
}

// trace_footprint: trace_windows' arguments, the footprint plan's fields and the map (wgrt_trace_footprint).
int64_t trace_footprint(TRACE_PARAMS, double fp_x0, double fp_y0, double fp_cell_x, double fp_cell_y, int64_t fp_nx_cells,
                        int64_t fp_ny_cells, Tensor map) {
    return trace_core(TRACE_COMMON,
                      FootprintSink{footprint_plan_of(fp_x0, fp_y0, fp_cell_x, fp_cell_y, fp_nx_cells, fp_ny_cells), map});
}

// trace_hits: trace_windows' arguments, the record buffer, its capacity in records, the counter and the tag
// (wgrt_trace_hits).
int64_t trace_hits(TRACE_PARAMS, Tensor hits, int64_t capacity, std::optional<Tensor> count, int64_t tag) {
    return trace_core(TRACE_COMMON, HitsSink{hits, capacity, count, tag});
}

// trace_paths: trace_hits' arguments over a path list, and the batch's select bytes (wgrt_trace_paths).
int64_t trace_paths(TRACE_PARAMS, Tensor paths, int64_t capacity, std::optional<Tensor> count, int64_t tag,
                    const std::optional<Tensor> &select) {
    return trace_core(TRACE_COMMON, PathsSink{{paths, capacity, count, tag}, select});
}

// trace_visits: trace_windows' arguments, the batch's slots (or None), the rows there are, their counts and their end
// records (wgrt_trace_visits).
int64_t trace_visits(TRACE_PARAMS, const std::optional<Tensor> &slot, int64_t n_rows, Tensor counts, Tensor ends) {
    return trace_core(TRACE_COMMON, VisitsSink{slot, n_rows, counts, ends});
}

// trace_stokes: trace_windows' arguments and the Stokes tables (wgrt_trace_stokes).
int64_t trace_stokes(TRACE_PARAMS, Tensor stokes) { return trace_core(TRACE_COMMON, StokesSink{stokes}); }

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
    const int64_t C = VISITS_SYM(wgrt_visit_channels)(s), W = WINDOW_SYM(wgrt_window_plan_width)(wp);
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
    if (!lnscale) return VISITS_SYM(wgrt_visits_sensitivity)(s, wp, cnt, e, n_rows, out.data_ptr<double>(), hip_stream);
    TORCH_CHECK(lnscale->device() == dev && lnscale->scalar_type() == at::kDouble && lnscale->is_contiguous() &&
                    lnscale->numel() == C,
                "wgrt.visits_reduce: lnscale must be contiguous float64 [", C, "] on the scene's device");
    return VISITS_SYM(wgrt_visits_reweight)(s, wp, cnt, e, n_rows, lnscale->const_data_ptr<double>(), out.data_ptr<double>(),
                                            hip_stream);
}

// visits_reweight_many: the first n_rows rows re-weighted for K designs at once (wgrt_visits_reweight_many): lnscale
// float64 [K, C], out float64 [K, n_slabs, W], wsums int64 [K, 2, num_lmd] or None.  Both outputs are added to.
int64_t visits_reweight_many(int64_t scene, int64_t plan, const Tensor &counts, const Tensor &ends, int64_t n_rows,
                             const Tensor &lnscale, Tensor out, std::optional<Tensor> wsums, int64_t stream) {
    const wgrt_scene *s = reinterpret_cast<const wgrt_scene *>(static_cast<uintptr_t>(scene));
    const wgrt_window_plan *wp = reinterpret_cast<const wgrt_window_plan *>(static_cast<uintptr_t>(plan));
    TORCH_CHECK(s != nullptr && wp != nullptr, "wgrt.visits_reweight_many: NULL scene / plan");
    wgrt_scene_info info{};
    const wgrt_status st = wgrt_scene_get_info(s, &info);
    if (st != WGRT_OK) return st;
    const c10::Device dev(c10::DeviceType::CUDA, static_cast<c10::DeviceIndex>(info.device));
    const int64_t C = VISITS_SYM(wgrt_visit_channels)(s), W = WINDOW_SYM(wgrt_window_plan_width)(wp);
    const int64_t nl = WGRT_SYM(wgrt_visit_wavelengths, "visits_reweight_many", "the design ensembles")(s);
    TORCH_CHECK(W > 0, "wgrt.visits_reweight_many: a bad window plan");
    TORCH_CHECK(counts.device() == dev && ends.device() == dev && out.device() == dev && lnscale.device() == dev &&
                    (!wsums || wsums->device() == dev),
                "wgrt.visits_reweight_many: counts, ends, lnscale, out and wsums must be on the scene's device");
    TORCH_CHECK(n_rows >= 0 && counts.scalar_type() == at::kInt && counts.is_contiguous() && counts.numel() >= n_rows * C,
                "wgrt.visits_reweight_many: counts must be contiguous int32 with >= n_rows * ", C, " entries");
    TORCH_CHECK(ends.scalar_type() == at::kByte && ends.is_contiguous() &&
                    ends.numel() >= n_rows * (int64_t)sizeof(wgrt_visit_end),
                "wgrt.visits_reweight_many: ends must be contiguous uint8 with >= n_rows * 32 bytes");
    TORCH_CHECK(lnscale.scalar_type() == at::kDouble && lnscale.is_contiguous() && lnscale.dim() == 2 &&
                    lnscale.size(0) >= 1 && lnscale.size(0) <= INT32_MAX && lnscale.size(1) == C,
                "wgrt.visits_reweight_many: lnscale must be contiguous float64 [K >= 1, ", C, "]");
    const int64_t K = lnscale.size(0);
    TORCH_CHECK(out.scalar_type() == at::kDouble && out.is_contiguous() && out.dim() == 3 && out.size(0) == K &&
                    out.size(1) == (int64_t)info.tiles && out.size(2) == W,
                "wgrt.visits_reweight_many: out must be contiguous float64 [", K, ", ", info.tiles, ", ", W, "]");
    TORCH_CHECK(!wsums || (wsums->scalar_type() == at::kLong && wsums->is_contiguous() && wsums->dim() == 3 &&
                           wsums->size(0) == K && wsums->size(1) == 2 && wsums->size(2) == nl),
                "wgrt.visits_reweight_many: wsums must be contiguous int64 [", K, ", 2, ", nl, "]");
    const c10::DeviceGuard guard(dev);
    return WGRT_SYM(wgrt_visits_reweight_many, "visits_reweight_many", "the design ensembles")(
        s, wp, static_cast<const uint32_t *>(counts.const_data_ptr()),
        static_cast<const wgrt_visit_end *>(ends.const_data_ptr()), n_rows, lnscale.const_data_ptr<double>(), (int32_t)K,
        out.data_ptr<double>(), wsums ? wsums->data_ptr<int64_t>() : nullptr,
        reinterpret_cast<void *>(static_cast<uintptr_t>(stream)));
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
    const wgrt_footprint_plan fp = footprint_plan_of(fp_x0, fp_y0, fp_cell_x, fp_cell_y, fp_nx_cells, fp_ny_cells);
    check_footprint_map("wgrt.paths_footprint", map, fp, num_lmd, 0);
    const c10::DeviceGuard guard(paths.device());
    return PATHS_SYM(wgrt_paths_footprint)(static_cast<const wgrt_path_vertex *>(paths.const_data_ptr()), n,
                                           static_cast<int32_t>(std::max<int64_t>(-1, std::min<int64_t>(num_lmd, 1 << 20))),
                                           &fp, static_cast<int64_t *>(map.data_ptr()),
                                           reinterpret_cast<void *>(static_cast<uintptr_t>(stream)));
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
    // the same launch adding every counted out-coupling's Stokes quanta to the tables beside the window table
    // (wgrt_trace_stokes): stokes int64 [3, tiles, W], added to
    m.def("trace_stokes(int scene, Tensor x, Tensor y, Tensor m, Tensor n, Tensor? lmd_num, Tensor te, Tensor tm, "
          "Tensor delta_phase, Tensor(a!) rng_states, Tensor(b!)? matrix_EB, Tensor(c!)? stats, "
          "Tensor(d!)? per_ray_bounces, int n_rays, int gid_offset, int stream, int kernel, int variant, "
          "int workgroups, Tensor? chunk_order, int num_iter, Tensor? gid_blocks, int gid_block_rays, int debug, "
          "float grid_sqrt_k, int plan, Tensor(e!)? table, Tensor(f!) stokes) -> int",
          &trace_stokes);
    // a visits table reduced into sensitivity tables (lnscale None) or a re-weighted window table
    m.def("visits_reduce(int scene, int plan, Tensor counts, Tensor ends, int n_rows, Tensor? lnscale, Tensor(a!) out, "
          "int stream) -> int",
          &visits_reduce);
    // the same rows re-weighted for K designs at once, with the weights' sums in quanta of 2^-32
    m.def("visits_reweight_many(int scene, int plan, Tensor counts, Tensor ends, int n_rows, Tensor lnscale, "
          "Tensor(a!) out, Tensor(b!)? wsums, int stream) -> int",
          &visits_reweight_many);
    m.def("chain_step(int chain) -> int", &chain_step);
    m.def("chain_end(int chain) -> int", &chain_end);
}
