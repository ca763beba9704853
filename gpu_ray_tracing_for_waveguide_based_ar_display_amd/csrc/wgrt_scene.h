// wgrt_scene.h -- the device-resident scene behind the opaque wgrt_scene handle (include/wgrt.h),
// shared by the C-ABI translation units.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <map>
#include <mutex>
#include <string>

#include "wgrt_args.h"
#include "wgrt_host.h"
#include "wgrt_trace_mode.h"

struct wgrt_scene {
    int device = 0;
    int nx = 0, ny = 0, nl = 0, nfc = 0, noc = 0, tile_d = 0, npoly = 0;
    double n_g = 0;
    double *d_tiles = nullptr;
    double *d_jtiles = nullptr;
    int jtile_d = 0;
    uint64_t *d_cells = nullptr;
    uint32_t *d_cells32 = nullptr;   // 32-bit copy of the cell words (npoly <= 16), else NULL
    // The byte locator (wgrt_args.h ByteLocatorT): the scene's distinct cell words ascending (zero past palette_count;
    // kPaletteSlots entries, of which the kernels read the first kPaletteMax, and their 32-bit copy for npoly <= 16) and each cell's palette index.  All NULL when the
    // grid holds more distinct words than the palette (or the debug cap at creation) allows: such a scene runs the
    // word-form kernels.  palette_count: the distinct words, saturating at kPaletteSlots.
    uint64_t *d_palette = nullptr;
    uint32_t *d_palette32 = nullptr;
    uint8_t *d_cells8 = nullptr;
    int palette_count = 0;
    double *d_verts = nullptr;
    int32_t *d_poly_off = nullptr;
    int32_t *d_row_off = nullptr;
    int32_t *d_row_edges = nullptr;
    double *d_bands = nullptr;
    wgrt::LocatorHost loc_host;  // grid parameters (cells / verts vectors released after upload)
    int64_t tiles = 0;
    int64_t edge_cells = 0;        // locator cells with an EDGE class
    // resident 256-thread workgroups of the Jones kernels, by [mode][byte locator][64-bit cells][fused][single
    // wavelength] (wgrt_trace_mode.h; the smaller of the plain and the AMP instantiation's; 0: none is built) ...
    int jones_grid[wgrt::kTraceModes][2][2][2][2] = {};
    // ... and the most a chained step may use (wgrt_chain_*), by [byte locator][64-bit cells]: half the resident
    // grid less a margin (query_trace_grids)
    int jones_chain_grid[2][2] = {};
    // the kernel table's entry the last launch looked up, as the flat index of [mode][byte locator][64-bit cells]
    // [fused][single wavelength][AMP]; -1: none yet, or a grid / exact-lane kernel (wgrt_debug_last_trace_kernel;
    // host-side, read by nothing else)
    std::atomic<int> last_trace_kernel{-1};
    int64_t nonunitary_blocks = 0;  // Jones blocks whose branch matrices are not scaled-unitary (their launches
                                    // run the AMP instantiations: wgrt_jones_lane.h, the amplification step)
    // The automatic issue order's statistic (wgrt_order.h): per (wavelength, FoV) tile, the traces of the
    // learning launches that took more than kLongBounces bounces.  learned_rays / learn_gen (the rays those
    // launches traced, and how many there were) change under scratch_mu.
    uint32_t *d_tile_tail = nullptr;
    int64_t learned_rays = 0;
    uint32_t learn_gen = 0;
    // Jones-vector launches: per-stream launch scratch (launches on one stream are ordered, so
    // they may share it; launches on different streams never do)
    struct Scratch {
        // two counter sets (kHeads chunk heads kHeadStride apart, replay count, queue count,
        // full-block count), used by alternate launches: a launch's epilogue zeroes the other one
        unsigned long long *ctr = nullptr;
        uint32_t parity = 0;                 // the set the next launch uses
        bool dirty = false;                  // a launch failed half-way: both sets need zeroing
        uint32_t *full = nullptr;            // full-block list (qcap / kQBlock entries)
        uint32_t *list = nullptr;            // replay list; behind its cap entries, one more word per entry: the draws a
                                             // footprint launch had counted for the abandoned ray (TraceArgs::fp_seen)
        int64_t cap = 0;                     // replay list entries
        double2 *q_xy = nullptr;             // out-coupling queue: position, ray index
        uint32_t *q_i = nullptr;
        int64_t qcap = 0;
        uint32_t *q_ray = nullptr;           // a hits launch's third queue column, the entry's local ray index: grown
        int64_t qcap_ray = 0;                // by hits launches only (wgrt_trace_hits)
        int4 *q_stokes = nullptr;            // a Stokes launch's fourth queue column, the entry's three quanta (one
        int64_t qcap_stokes = 0;             // 16-byte store): grown by Stokes launches only (wgrt_trace_stokes)
        unsigned long long *part = nullptr;  // per-wave counter partials (kPartWords words per slot)
        int64_t part_slots = 0;
        uint64_t *rng64 = nullptr;           // fused launches: per-ray {state, tag} granules
        uint32_t iter_epoch = 0;             // < 2^23 (iter_tag)
        int64_t cap64 = 0;
        // the automatic issue order: the permutation, the sort's other buffer and the chunks' class keys
        // (order_cap chunks each), and what the permutation was built from
        int32_t *order = nullptr;
        int64_t order_cap = 0;
        int64_t order_rays = -1;             // -1: none built
        const float *order_m = nullptr, *order_n = nullptr, *order_l = nullptr;
        uint32_t order_gen = 0;
        // chained single launches (wgrt_chain_*, caller's stream S = this scratch's key): the library-owned
        // side stream T (hipStreamNonBlocking; its launch scratch is the map's entry for T), the events of a
        // segment's two ends, and the per-ray {state, tag} granules both sides hand over through -- the one
        // thing the two sides share.  chain_serial: the last tag serial handed out (chain_tag, wgrt_trace.hip);
        // it only grows while the granule array lives, so a stale granule never matches.
        hipStream_t chain_side = nullptr;
        hipEvent_t chain_ev_begin = nullptr, chain_ev_join = nullptr;
        uint64_t *chain_gran = nullptr;
        int64_t chain_cap = 0;
        uint32_t chain_serial = 0;
        bool chain_open = false;             // a wgrt_chain is between begin and end on this stream
        // a gathering chain (chain_step_gather, wgrt_trace.hip): recorded behind the chain's last launch on S and
        // queried, never waited for -- "is the stream still busy with what the chain has issued?"
        hipEvent_t chain_ev_busy = nullptr;
    };
    std::mutex scratch_mu;
    std::map<void *, Scratch> scratch;
};

namespace wgrt {

// What scene creation and destruction need from the trace unit (wgrt_trace.hip), the one place that
// instantiates the trace kernels and knows the launch scratch:
// the resident grid of every trace kernel instantiation (jones_grid, jones_chain_grid) from the occupancy queries ...
wgrt_status query_trace_grids(wgrt_scene *s);
// ... and the release of one stream's launch scratch (the scene's device is current)
void free_scratch(wgrt_scene::Scratch &sc);

inline Locator make_locator(const wgrt_scene *s) {
    Locator L;
    L.cells = s->d_cells;
    L.verts = s->d_verts;
    L.poly_off = s->d_poly_off;
    L.row_off = s->d_row_off;
    L.row_edges = s->d_row_edges;
    L.bands = s->d_bands;
    L.x0 = s->loc_host.x0;
    L.y0 = s->loc_host.y0;
    L.inv_h = s->loc_host.inv_h;
    L.ncx = s->loc_host.ncx;
    L.ncy = s->loc_host.ncy;
    return L;
}

template <class CellT>
inline ByteLocatorT<CellT> make_byte_locator(const wgrt_scene *s, const Locator &g, const CellT *palette) {
    ByteLocatorT<CellT> L;
    L.cells = s->d_cells8;
    L.palette = palette;
    L.verts = g.verts;
    L.poly_off = g.poly_off;
    L.row_off = g.row_off;
    L.row_edges = g.row_edges;
    L.bands = g.bands;
    L.x0 = g.x0, L.y0 = g.y0, L.inv_h = g.inv_h, L.ncx = g.ncx, L.ncy = g.ncy;
    return L;
}

inline LocatorT<uint32_t> make_locator32(const wgrt_scene *s) {
    const Locator g = make_locator(s);
    LocatorT<uint32_t> L;
    L.cells = s->d_cells32;
    L.verts = g.verts;
    L.poly_off = g.poly_off;
    L.row_off = g.row_off;
    L.row_edges = g.row_edges;
    L.bands = g.bands;
    L.x0 = g.x0, L.y0 = g.y0, L.inv_h = g.inv_h, L.ncx = g.ncx, L.ncy = g.ncy;
    return L;
}

}  // namespace wgrt
