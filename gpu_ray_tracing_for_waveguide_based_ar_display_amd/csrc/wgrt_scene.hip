// wgrt_scene.hip -- the device-resident scene (include/wgrt.h wgrt_scene_*): its build on the device
// (the locator's cell words, the LUT tiles), its release, and the locator classifiers the tests check
// the build with.  The trace kernels are not instantiated here: what scene creation needs of them
// comes through wgrt_scene.h (query_trace_grids, free_scratch).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/wgrt.h"
#include "../../include/wgrt_debug.h"
#include "wgrt_common.h"
#include "wgrt_locator.h"
#include "wgrt_scene.h"
#include "wgrt_scene_build.h"

using namespace wgrt;

namespace {

// Cell size (mm) of the global-memory locator grid (wgrt_scene_opts.cell_mm = 0): 1/128 mm, a 71 MB
// grid at C3; fewer EDGE-cell exact tests than coarser grids (fastest on C3).
#ifndef WGRT_CELL_MM
#define WGRT_CELL_MM 0.0078125
#endif
constexpr double kDefaultCellMm = WGRT_CELL_MM;

__global__ __launch_bounds__(256) void classify_kernel(Locator L, int npoly, const double *xy, int64_t n,
                                                       uint64_t *out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = xy[2 * i], y = xy[2 * i + 1];
    const Cell w = locate(L, x, y);
    const uint64_t ww = locate_w(L, x, y);
    uint64_t mask = 0, mism = 0;
    for (int k = 0; k < npoly; ++k) {
        const bool a = in_poly(L, w, k, x, y);      // CSR row lists (exact lane)
        const bool b = in_poly_w(L, ww, k, x, y);   // 128-B band records (Jones-vector lane)
        if (a) mask |= 1ull << k;
        if (a != b) mism = 1ull << 63;
    }
    out[i] = mask | mism;
}

// ---------------------------------------------------------------------------------------------
// Scene build on the device (wgrt_scene_create): the locator's cell words and the LUT tiles.
// ---------------------------------------------------------------------------------------------
// EDGE marks: one thread per (polygon edge, grid row); the row's cells the edge reaches get the
// polygon's bit (wgrt_pack.h edge_row_span, the host build's rule).
__global__ __launch_bounds__(256) void edge_mark_kernel(const double *verts, const int32_t *poly_off, int npoly,
                                                        double x0, double y0, double h, int ncx, int ncy,
                                                        uint32_t *mask) {
    const int e = blockIdx.y;   // global edge index: polygon k's edge (i - 1 -> i), i = e - poly_off[k]
    int k = 0;
    while (k + 1 < npoly && poly_off[k + 1] <= e) ++k;
    const int a = poly_off[k], nv = poly_off[k + 1] - a, i = e - a;
    if (nv <= 0 || i < 0 || i >= nv) return;
    const int j = i == 0 ? nv - 1 : i - 1;
    const double ax = verts[2 * (a + j)], ay = verts[2 * (a + j) + 1];
    const double bx = verts[2 * (a + i)], by = verts[2 * (a + i) + 1];
    int cy0, cy1;
    edge_rows(ay, by, y0, h, ncy, cy0, cy1);
    const int cy = cy0 + (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (cy > cy1) return;
    int cx0, cx1;
    if (!edge_row_span(ax, ay, bx, by, cy, x0, y0, h, ncx, cx0, cx1)) return;
    for (int cx = cx0; cx <= cx1; ++cx) atomicOr(mask + (size_t)cy * ncx + cx, 1u << k);
}

// Cell words: EDGE where marked, else the reference predicate's crossing parity at the cell
// centre over the row's edges (every edge crossing the row's centre line is in its band list).
__global__ __launch_bounds__(256) void classify_cells_kernel(const double *verts, const int32_t *poly_off, int npoly,
                                                             const int32_t *row_off, const int32_t *row_edges,
                                                             double x0, double y0, double h, int ncx, int ncy,
                                                             const uint32_t *mask, uint64_t *cells, uint32_t *cells32,
                                                             unsigned long long *edge_cells) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t edges = 0;
    if (c < (int64_t)ncx * ncy) {
        const int cy = (int)(c / ncx), cx = (int)(c % ncx);
        const double px = x0 + (cx + 0.5) * h, py = y0 + (cy + 0.5) * h;
        const uint32_t mk = mask[c];
        uint64_t w = 0;
        for (int k = 0; k < npoly; ++k) {
            uint64_t cls;
            if ((mk >> k) & 1u) {
                cls = 2;
                ++edges;
            } else {
                const int a = poly_off[k], nv = poly_off[k + 1] - a;
                const int r = k * ncy + cy;
                unsigned cnt = 0;
                for (int e = row_off[r]; e < row_off[r + 1]; ++e) {
                    const int i = row_edges[e], j = i == 0 ? nv - 1 : i - 1;
                    const double xi = verts[2 * (a + i)], yi = verts[2 * (a + i) + 1];
                    const double xj = verts[2 * (a + j)], yj = verts[2 * (a + j) + 1];
                    if ((yi > py) != (yj > py)) cnt += px < (xj - xi) * (py - yi) / (yj - yi + 1e-20) + xi;
                }
                cls = cnt & 1u;
            }
            w |= cls << (2 * k);
        }
        cells[c] = w;
        if (cells32) cells32[c] = (uint32_t)w;
    }
    edges = wave_sum(edges);
    if ((threadIdx.x & 63) == 0 && edges) atomicAdd(edge_cells, (unsigned long long)edges);
}

// ---------------------------------------------------------------------------------------------
// The byte locator's palette and byte grid on the device (wgrt_scene_build.h build_palette_host is the host
// build's; both are pure functions of the word grid, so the two builds agree byte for byte).
// ---------------------------------------------------------------------------------------------
constexpr unsigned long long kPalEmpty = ~0ull;   // no cell word: class 3 does not exist

// The distinct cell words into an open-addressing table of kPaletteSlots slots.  Only a cell whose word differs
// from its left neighbour's inserts (the first of a run; every distinct word starts at least one run), and an
// insert first looks: the atomics are as many as there are distinct words, give or take a race.  A word that finds
// the table full sets *overflow.
__global__ __launch_bounds__(256) void palette_collect_kernel(const uint64_t *cells, int64_t n, unsigned long long *table,
                                                              int *overflow) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const unsigned long long w = cells[c];
    if (c > 0 && cells[c - 1] == w) return;
    unsigned h = (unsigned)((w * 0x9E3779B97F4A7C15ull) >> 40) & (kPaletteSlots - 1);
    for (int probe = 0; probe < kPaletteSlots; ++probe, h = (h + 1) & (kPaletteSlots - 1)) {
        unsigned long long cur = __hip_atomic_load(table + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == kPalEmpty) cur = atomicCAS(table + h, kPalEmpty, w);
        if (cur == kPalEmpty || cur == w) return;
    }
    atomicOr(overflow, 1);
}

// One workgroup: the table's words by rank (strictly ascending; zero past the count) and their count.
__global__ __launch_bounds__(1024) void palette_sort_kernel(const unsigned long long *table, uint64_t *palette,
                                                            uint32_t *palette32, int *count) {
    __shared__ unsigned long long key[kPaletteSlots];
    __shared__ int total;
    if (threadIdx.x == 0) total = 0;
    for (int k = threadIdx.x; k < kPaletteSlots; k += blockDim.x) {
        key[k] = table[k];
        palette[k] = 0;
    }
    for (int k = threadIdx.x; k < kPaletteMax; k += blockDim.x) palette32[k] = 0;
    __syncthreads();
    for (int k = threadIdx.x; k < kPaletteSlots; k += blockDim.x) {
        const unsigned long long w = key[k];
        if (w == kPalEmpty) continue;
        int rank = 0;
        for (int j = 0; j < kPaletteSlots; ++j) rank += key[j] < w;   // (the empty marker is the largest value)
        palette[rank] = w;
        if (rank < kPaletteMax) palette32[rank] = (uint32_t)w;
        atomicAdd(&total, 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) *count = total;
}

// Each cell's palette index: a binary search of the (at most kPaletteMax) palette words held in LDS.
__global__ __launch_bounds__(256) void cells8_kernel(const uint64_t *cells, int64_t n, const uint64_t *palette, int count,
                                                     uint8_t *cells8) {
    __shared__ uint64_t pal[kPaletteMax];
    pal[threadIdx.x] = threadIdx.x < count ? palette[threadIdx.x] : ~0ull;
    __syncthreads();
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const uint64_t w = cells[c];
    int lo = 0;
    for (int step = kPaletteMax / 2; step > 0; step >>= 1) lo += pal[lo + step - 1] < w ? step : 0;
    cells8[c] = (uint8_t)lo;
}

// wgrt_debug_set_palette_cap: the most distinct cell words a scene created from now on may have and still get a
// byte grid (tests force the fallback with it; at most kPaletteMax, the default).
std::atomic<int> g_palette_cap{kPaletteMax};

// Blocks of the Jones tiles flagged non-scaled-unitary (the sign bit of their float Wsum, wgrt_pack.h):
// counted once per scene, to pick the trace kernel instantiation (AMP) for its launches.
__global__ __launch_bounds__(256) void nonunitary_kernel(const double *jtiles, int64_t ntiles, int jd, int nblk,
                                                         unsigned long long *count) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ntiles * nblk) return;
    const int64_t g = i / nblk, b = i % nblk;
    const float w = *(const float *)(jtiles + g * jd + kJHeader + kJBlock * b + kJBlockF32);
    if (__float_as_uint(w) >> 31) atomicAdd(count, 1ull);
}

// One thread per (lambda, m, n) tile: the exact lane's tile and its Jones-vector tile
// (wgrt_pack.h pack_tile, the host build's code); flags any non-finite value.
__global__ __launch_bounds__(64) void pack_tiles_kernel(PackView v, int64_t ntiles, double *tiles, double *jtiles,
                                                        int td, int jd, int *nonfinite) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ntiles) return;
    double *T = tiles + g * td;
    pack_tile(v, g, T, jtiles + g * jd);
    bool bad = false;
    for (int k = 0; k < td; ++k) bad |= !isfinite(T[k]);
    if (bad) atomicOr(nonfinite, 1);
}

// hipMalloc of n elements (n may be 0) ...
template <class T>
wgrt_status alloc_n(size_t n, T **dst) {
    return malloc_status(hipMalloc((void **)dst, std::max<size_t>(n, 1) * sizeof(T)));
}

// ... and their copy from the host
template <class T>
wgrt_status upload_n(const T *src, size_t n, T **dst) {
    const wgrt_status st = alloc_n(n, dst);
    if (st != WGRT_OK) return st;
    if (n) HIP_TRY(hipMemcpy(*dst, src, n * sizeof(T), hipMemcpyHostToDevice));
    return WGRT_OK;
}

template <class T>
wgrt_status upload(const std::vector<T> &v, T **dst) {
    return upload_n(v.data(), v.size(), dst);
}

// The scene's palette and byte grid from its cell words: on the host from the host build's words (host_cells), else
// on the device from d_cells.  More distinct words than the cap: the scene keeps only the count.
wgrt_status build_byte_grid(wgrt_scene *s, size_t ncells, const std::vector<uint64_t> *host_cells) {
    const int cap = std::min(g_palette_cap.load(std::memory_order_relaxed), kPaletteMax);
    wgrt_status st;
    if (host_cells) {
        std::vector<uint64_t> pal;
        std::vector<uint8_t> c8;
        s->palette_count = build_palette_host(*host_cells, cap, pal, c8);
        if (s->palette_count > cap) return WGRT_OK;
        pal.resize(kPaletteSlots, 0ull);
        std::vector<uint32_t> pal32(pal.begin(), pal.begin() + kPaletteMax);
        if ((st = upload(pal, &s->d_palette)) != WGRT_OK || (st = upload(c8, &s->d_cells8)) != WGRT_OK ||
            (s->npoly <= 16 && (st = upload(pal32, &s->d_palette32)) != WGRT_OK))
            return st;
        return WGRT_OK;
    }
    unsigned long long *table = nullptr;
    int *flags = nullptr;   // [0] the table overflowed, [1] the count
    uint32_t *pal32 = nullptr;
    auto done = [&](wgrt_status e) {
        (void)hipFree(table);
        (void)hipFree(flags);
        (void)hipFree(pal32);
        return e;
    };
    if ((st = alloc_n((size_t)kPaletteSlots, &table)) != WGRT_OK || (st = alloc_n(2, &flags)) != WGRT_OK ||
        (st = alloc_n((size_t)kPaletteMax, &pal32)) != WGRT_OK || (st = alloc_n((size_t)kPaletteSlots, &s->d_palette)) != WGRT_OK)
        return done(st);
    auto hip = [&](hipError_t e) { return e == hipSuccess ? WGRT_OK : fail(WGRT_ERR_HIP, std::string("byte grid: ") + hipGetErrorString(e)); };
    if ((st = hip(hipMemset(table, 0xff, kPaletteSlots * sizeof(unsigned long long)))) != WGRT_OK ||
        (st = hip(hipMemset(flags, 0, 2 * sizeof(int)))) != WGRT_OK)
        return done(st);
    hipLaunchKernelGGL(palette_collect_kernel, dim3((unsigned)((ncells + 255) / 256)), dim3(256), 0, 0, s->d_cells,
                       (int64_t)ncells, table, flags);
    hipLaunchKernelGGL(palette_sort_kernel, dim3(1), dim3(1024), 0, 0, table, s->d_palette, pal32, flags + 1);
    int h[2] = {0, 0};
    if ((st = hip(hipGetLastError())) != WGRT_OK || (st = hip(hipMemcpy(h, flags, sizeof(h), hipMemcpyDeviceToHost))) != WGRT_OK)
        return done(st);
    s->palette_count = h[0] ? kPaletteSlots : h[1];
    if (s->palette_count > cap) {
        (void)hipFree(s->d_palette);
        s->d_palette = nullptr;
        return done(WGRT_OK);
    }
    if ((st = alloc_n(ncells, &s->d_cells8)) != WGRT_OK) return done(st);
    hipLaunchKernelGGL(cells8_kernel, dim3((unsigned)((ncells + 255) / 256)), dim3(256), 0, 0, s->d_cells, (int64_t)ncells,
                       s->d_palette, s->palette_count, s->d_cells8);
    if ((st = hip(hipGetLastError())) != WGRT_OK || (st = hip(hipDeviceSynchronize())) != WGRT_OK) return done(st);
    if (s->npoly <= 16) {
        s->d_palette32 = pal32;
        pal32 = nullptr;
    }
    return done(WGRT_OK);
}

}  // namespace

extern "C" {

wgrt_status wgrt_scene_create(const wgrt_scene_desc *desc, int device, wgrt_scene **out) {
    return wgrt_scene_create_ex(desc, device, nullptr, out);
}

wgrt_status wgrt_scene_create_ex(const wgrt_scene_desc *desc, int device, const wgrt_scene_opts *opts,
                                 wgrt_scene **out) {
    if (!desc || !out) return fail(WGRT_ERR_INVALID_ARGUMENT, "NULL desc / out");
    *out = nullptr;
    const wgrt_scene_desc &d = *desc;
    const double cell_mm = (opts && opts->cell_mm > 0.0) ? opts->cell_mm : kDefaultCellMm;
    if (opts && !(opts->cell_mm >= 0.0)) return fail(WGRT_ERR_INVALID_ARGUMENT, "cell_mm must be >= 0");
    const bool host_build = opts && opts->host_build != 0;
    const int f32_angles = opts ? opts->lut_f32_angles : 0;
    if (f32_angles & ~0x7f) return fail(WGRT_ERR_INVALID_ARGUMENT, "lut_f32_angles has bits beyond the 7 LUTs");
    // A mixed set: compiled numba unifies the ray's theta (assigned from every table, GRTF:850, 872, 1021,
    // ...) to complex128 as soon as one table is complex128, so the carried cos(theta.real) would be a
    // double cosine of a single-precision table's angle while that table's numerator stays cosf --
    // two cosines per branch the scene does not hold.  Only uniform sets are supported.
    if (f32_angles != 0 && f32_angles != 0x7f)
        return fail(WGRT_ERR_UNSUPPORTED, "lut_f32_angles must be 0 (complex128 LUTs) or 0x7f (all seven complex64): "
                                          "a mixed-precision LUT set is not supported");
    // host: validation, the locator's geometry (extent, vertices, row bands) and the trig table
    // (every cos / sin on the host libm); the cell words and the tiles are built on the device
    // (host_build: both on the host, the reference build the device one is checked against)
    SceneHost host;
    try {
        build_scene_host(d, cell_mm, host, host_build, host_build, f32_angles);
    } catch (const std::exception &e) {
        return fail(WGRT_ERR_INVALID_ARGUMENT, e.what());
    }
    DEVICE_SCOPE(dev_scope, device);   // the caller's current device is restored on return
    auto *s = new wgrt_scene();
    s->device = device;
    s->nx = d.nx;
    s->ny = d.ny;
    s->nl = d.num_lmd;
    s->nfc = (int)d.n_fc_slices;
    s->noc = (int)d.n_oc_slices;
    s->tile_d = host.tile_doubles;
    s->jtile_d = host.jtile_doubles;
    s->npoly = 3 + s->nfc + s->noc;
    s->n_g = d.n_g;
    s->tiles = (int64_t)s->nl * s->nx * s->ny;
    wgrt_status st;
    auto bail = [&](wgrt_status e) {
        wgrt_scene_destroy(s);
        return e;
    };
    if ((st = upload(host.loc.verts, &s->d_verts)) != WGRT_OK ||
        (st = upload(host.loc.poly_off, &s->d_poly_off)) != WGRT_OK ||
        (st = upload(host.loc.row_off, &s->d_row_off)) != WGRT_OK ||
        (st = upload(host.loc.row_edges, &s->d_row_edges)) != WGRT_OK ||
        (st = upload(host.loc.bands, &s->d_bands)) != WGRT_OK)
        return bail(st);
    const size_t ncells = (size_t)host.loc.ncx * host.loc.ncy;
    if (host_build) {
        if ((st = upload(host.tiles, &s->d_tiles)) != WGRT_OK || (st = upload(host.jtiles, &s->d_jtiles)) != WGRT_OK ||
            (st = upload(host.loc.cells, &s->d_cells)) != WGRT_OK)
            return bail(st);
        if (s->npoly <= 16) {
            const std::vector<uint32_t> c32(host.loc.cells.begin(), host.loc.cells.end());
            if ((st = upload(c32, &s->d_cells32)) != WGRT_OK) return bail(st);
        }
        s->edge_cells = host.loc.edge_cells;
    } else {
        // the raw arrays the tiles are packed from, on the device for the packing only
        const int64_t g = (int64_t)d.num_lmd * d.nx * d.ny, nfc = d.n_fc_slices, noc = d.n_oc_slices;
        const size_t n5 = (size_t)g * d.ch5 * 2, n3 = (size_t)g * d.ch3 * 2;
        double *raw[12] = {};
        auto free_raw = [&]() {
            for (double *p : raw) (void)hipFree(p);
        };
        const double *src[12] = {d.lut_ic1, d.lut_ic2, d.lut_ic3, d.lut_fc1, d.lut_fc2, d.lut_oc1, d.lut_oc2,
                                 d.lut_TIR, d.lut_gap, d.eff_reg_FOV, d.eff_reg_FOV_range, host.trig.data()};
        const size_t cnt[12] = {n5, n5, n5, nfc * n3, nfc * n3, noc * n5, noc * n5, (size_t)g * 4, (size_t)g * 8,
                                (size_t)d.nx * d.ny * 8, (size_t)d.nx * d.ny * 4, host.trig.size()};
        for (int k = 0; k < 12; ++k)
            if ((st = upload_n(cnt[k] ? src[k] : nullptr, cnt[k], &raw[k])) != WGRT_OK) {
                free_raw();
                return bail(st);
            }
        PackView v = pack_view(d, raw[11]);
        v.ic1 = raw[0], v.ic2 = raw[1], v.ic3 = raw[2], v.fc1 = raw[3], v.fc2 = raw[4], v.oc1 = raw[5], v.oc2 = raw[6];
        v.tir = raw[7], v.gap = raw[8], v.fov = raw[9], v.fovr = raw[10];
        int *flag = nullptr;
        unsigned long long *ecount = nullptr;
        uint32_t *mask = nullptr;
        auto free_tmp = [&]() {
            free_raw();
            (void)hipFree(flag);
            (void)hipFree(ecount);
            (void)hipFree(mask);
        };
        if ((st = alloc_n((size_t)g * s->tile_d, &s->d_tiles)) != WGRT_OK ||
            (st = alloc_n((size_t)g * s->jtile_d, &s->d_jtiles)) != WGRT_OK || (st = alloc_n(1, &flag)) != WGRT_OK ||
            (st = alloc_n(1, &ecount)) != WGRT_OK || (st = alloc_n(ncells, &mask)) != WGRT_OK ||
            (st = alloc_n(ncells, &s->d_cells)) != WGRT_OK ||
            (s->npoly <= 16 && (st = alloc_n(ncells, &s->d_cells32)) != WGRT_OK)) {
            free_tmp();
            return bail(st);
        }
        HIP_TRY(hipMemset(s->d_tiles, 0, (size_t)g * s->tile_d * sizeof(double)));
        HIP_TRY(hipMemset(s->d_jtiles, 0, (size_t)g * s->jtile_d * sizeof(double)));
        HIP_TRY(hipMemset(flag, 0, sizeof(int)));
        HIP_TRY(hipMemset(ecount, 0, sizeof(unsigned long long)));
        HIP_TRY(hipMemset(mask, 0, ncells * sizeof(uint32_t)));
        hipLaunchKernelGGL(pack_tiles_kernel, dim3((unsigned)((g + 63) / 64)), dim3(64), 0, 0, v, g, s->d_tiles,
                           s->d_jtiles, s->tile_d, s->jtile_d, flag);
        HIP_TRY(hipGetLastError());
        const LocatorHost &L = host.loc;
        const int npoly = (int)L.poly_off.size() - 1, n_edges = L.poly_off.back();
        if (n_edges > 0) {
            hipLaunchKernelGGL(edge_mark_kernel, dim3((unsigned)((L.ncy + 255) / 256), (unsigned)n_edges), dim3(256),
                               0, 0, s->d_verts, s->d_poly_off, npoly, L.x0, L.y0, L.h, L.ncx, L.ncy, mask);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(classify_cells_kernel, dim3((unsigned)((ncells + 255) / 256)), dim3(256), 0, 0, s->d_verts,
                           s->d_poly_off, npoly, s->d_row_off, s->d_row_edges, L.x0, L.y0, L.h, L.ncx, L.ncy, mask,
                           s->d_cells, s->d_cells32, ecount);
        HIP_TRY(hipGetLastError());
        int bad = 0;
        unsigned long long ec = 0;
        HIP_TRY(hipMemcpy(&bad, flag, sizeof(int), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&ec, ecount, sizeof(ec), hipMemcpyDeviceToHost));
        free_tmp();
        if (bad) {
            // The kernels' cheap branch estimates assume finite tables (an inf / NaN coefficient
            // would make the reference's efficiencies NaN); such LUTs are rejected instead.
            return bail(fail(WGRT_ERR_INVALID_ARGUMENT,
                             "non-finite value in the LUTs / lut_TIR / lut_gap / eyebox tables"));
        }
        s->edge_cells = (int64_t)ec;
    }
    if ((st = build_byte_grid(s, ncells, host_build ? &host.loc.cells : nullptr)) != WGRT_OK) return bail(st);
    {   // the scene's non-scaled-unitary blocks (the trace kernel instantiation its launches run)
        const int nblk = 3 + 2 * s->nfc + 2 * s->noc;
        const int64_t nt = (int64_t)s->nl * s->nx * s->ny;
        unsigned long long *cnt = nullptr;
        HIP_TRY(hipMalloc((void **)&cnt, sizeof(unsigned long long)));
        hipError_t e = hipMemset(cnt, 0, sizeof(unsigned long long));
        if (e == hipSuccess && nt * nblk > 0) {
            hipLaunchKernelGGL(nonunitary_kernel, dim3((unsigned)((nt * nblk + 255) / 256)), dim3(256), 0, 0, s->d_jtiles,
                               nt, s->jtile_d, nblk, cnt);
            e = hipGetLastError();
        }
        unsigned long long nu = 0;
        if (e == hipSuccess) e = hipMemcpy(&nu, cnt, sizeof(nu), hipMemcpyDeviceToHost);
        (void)hipFree(cnt);
        if (e != hipSuccess) return bail(fail(WGRT_ERR_HIP, std::string("nonunitary_kernel: ") + hipGetErrorString(e)));
        s->nonunitary_blocks = (int64_t)nu;
    }
    {   // the automatic issue order's tile table starts empty (wgrt_scene.h)
        const size_t nt = (size_t)s->nl * s->nx * s->ny;
        if ((st = alloc_n(nt, &s->d_tile_tail)) != WGRT_OK) return bail(st);
        const hipError_t e = hipMemset(s->d_tile_tail, 0, std::max<size_t>(nt, 1) * sizeof(uint32_t));
        if (e != hipSuccess) return bail(fail(WGRT_ERR_HIP, std::string("hipMemset(tile_tail): ") + hipGetErrorString(e)));
    }
    if ((st = query_trace_grids(s)) != WGRT_OK) return bail(st);
    s->loc_host = host.loc;
    s->loc_host.cells.clear();
    s->loc_host.cells.shrink_to_fit();
    s->loc_host.row_edges.clear();
    s->loc_host.row_edges.shrink_to_fit();
    s->loc_host.bands.clear();
    s->loc_host.bands.shrink_to_fit();
    *out = s;
    return WGRT_OK;
}

wgrt_status wgrt_scene_destroy(wgrt_scene *s) {
    if (!s) return WGRT_OK;
    DeviceScope dev_scope(s->device);
    for (void *p : {(void *)s->d_tiles, (void *)s->d_jtiles, (void *)s->d_cells, (void *)s->d_cells32, (void *)s->d_palette, (void *)s->d_palette32,
                    (void *)s->d_cells8, (void *)s->d_verts,
                    (void *)s->d_poly_off, (void *)s->d_row_off, (void *)s->d_row_edges, (void *)s->d_bands,
                    (void *)s->d_tile_tail})
        (void)hipFree(p);
    for (auto &kv : s->scratch) free_scratch(kv.second);
    delete s;
    return WGRT_OK;
}

wgrt_status wgrt_scene_get_info(const wgrt_scene *s, wgrt_scene_info *info) {
    if (!s || !info) return fail(WGRT_ERR_INVALID_ARGUMENT, "NULL scene / info");
    info->tile_bytes = (int64_t)s->tile_d * 8;
    info->tiles = s->tiles;
    info->grid_cells_x = s->loc_host.ncx;
    info->grid_cells_y = s->loc_host.ncy;
    info->grid_cell_mm = s->loc_host.h;
    info->grid_edge_cells = s->edge_cells;
    info->n_polygons = s->npoly;
    info->device = s->device;
    info->jtile_bytes = (int64_t)s->jtile_d * 8;
    info->nonunitary_blocks = s->nonunitary_blocks;
    return WGRT_OK;
}

wgrt_status wgrt_scene_classify(const wgrt_scene *s, const double *xy, int64_t n, uint64_t *out_mask,
                                void *stream) {
    if (!s || (n > 0 && (!xy || !out_mask))) return fail(WGRT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n <= 0) return WGRT_OK;
    DEVICE_SCOPE(dev_scope, s->device);
    const int64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(classify_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       make_locator(s), s->npoly, xy, n, out_mask);
    HIP_TRY(hipGetLastError());
    return WGRT_OK;
}

wgrt_status wgrt_locator_classify_host(const wgrt_scene_desc *desc, double cell_mm, const double *xy, int64_t n,
                                       uint64_t *out_mask) {
    if (!desc || (n > 0 && (!xy || !out_mask))) return fail(WGRT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!(cell_mm > 0.0)) return fail(WGRT_ERR_INVALID_ARGUMENT, "cell_mm must be > 0");
    SceneHost host;
    try {
        build_scene_host(*desc, cell_mm, host);
    } catch (const std::exception &e) {
        return fail(WGRT_ERR_INVALID_ARGUMENT, e.what());
    }
    const int npoly = (int)host.loc.poly_off.size() - 1;
    // host replica of the device locator (same arithmetic as locate / in_poly)
    LocatorT<uint64_t> g{};
    g.cells = host.loc.cells.data();
    g.verts = host.loc.verts.data();
    g.poly_off = host.loc.poly_off.data();
    g.row_off = host.loc.row_off.data();
    g.row_edges = host.loc.row_edges.data();
    g.x0 = host.loc.x0, g.y0 = host.loc.y0, g.inv_h = host.loc.inv_h, g.ncx = host.loc.ncx, g.ncy = host.loc.ncy;
    for (int64_t i = 0; i < n; ++i) {
        const double x = xy[2 * i], y = xy[2 * i + 1];
        const double fx = std::floor((x - g.x0) * g.inv_h), fy = std::floor((y - g.y0) * g.inv_h);
        uint64_t w = 0;
        int cy = 0;
        if (fx >= 0.0 && fy >= 0.0 && fx < (double)g.ncx && fy < (double)g.ncy) {
            cy = (int)fy;
            w = g.cells[(size_t)cy * g.ncx + (int)fx];
        }
        uint64_t mask = 0;
        for (int k = 0; k < npoly; ++k) {
            const unsigned cls = (unsigned)(w >> (2 * k)) & 3u;
            bool in = cls == 1u;
            if (cls == 2u) {
                const int a = g.poly_off[k], nv = g.poly_off[k + 1] - a;
                const int r = k * g.ncy + cy;
                in = inside_or_on_edge_subset(x, y, g.verts + 2 * a, nv, g.row_edges + g.row_off[r],
                                              g.row_off[r + 1] - g.row_off[r]);
            }
            if (in) mask |= 1ull << k;
        }
        out_mask[i] = mask;
    }
    return WGRT_OK;
}

wgrt_status wgrt_locator_palette_host(const wgrt_scene_desc *desc, double cell_mm, int64_t *ncx, int64_t *ncy,
                                      double *grid, int *distinct_words, int *byte_grid, uint64_t *palette, uint8_t *cells8,
                                      uint64_t *cells, int64_t n_cells) {
    if (!desc) return fail(WGRT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!(cell_mm > 0.0)) return fail(WGRT_ERR_INVALID_ARGUMENT, "cell_mm must be > 0");
    SceneHost host;
    try {
        build_scene_host(*desc, cell_mm, host, true, false);
    } catch (const std::exception &e) {
        return fail(WGRT_ERR_INVALID_ARGUMENT, e.what());
    }
    const int64_t n = (int64_t)host.loc.ncx * host.loc.ncy;
    if (ncx) *ncx = host.loc.ncx;
    if (ncy) *ncy = host.loc.ncy;
    if (grid) grid[0] = host.loc.x0, grid[1] = host.loc.y0, grid[2] = host.loc.h;
    if ((cells8 || cells) && n_cells != n)
        return fail(WGRT_ERR_INVALID_ARGUMENT, "n_cells must be the grid's " + std::to_string(n) + " cells");
    const int cap = std::min(g_palette_cap.load(std::memory_order_relaxed), kPaletteMax);
    std::vector<uint64_t> pal;
    std::vector<uint8_t> c8;
    const int count = build_palette_host(host.loc.cells, cap, pal, c8);
    if (distinct_words) *distinct_words = count;
    if (byte_grid) *byte_grid = count <= cap;
    if (cells) std::copy(host.loc.cells.begin(), host.loc.cells.end(), cells);
    if (count > cap) return WGRT_OK;   // no byte grid: palette / cells8 are left as they were
    if (palette) {
        std::fill(palette, palette + kPaletteMax, 0ull);
        std::copy(pal.begin(), pal.end(), palette);
    }
    if (cells8) std::copy(c8.begin(), c8.end(), cells8);
    return WGRT_OK;
}

wgrt_status wgrt_debug_set_palette_cap(int cap) {
    if (cap < 0) return fail(WGRT_ERR_INVALID_ARGUMENT, "cap must be >= 0");
    g_palette_cap.store(std::min(cap, kPaletteMax), std::memory_order_relaxed);
    return WGRT_OK;
}

wgrt_status wgrt_debug_scene_copy(const wgrt_scene *s, int which, void *dst, int64_t bytes) {
    if (!s || !dst) return fail(WGRT_ERR_INVALID_ARGUMENT, "NULL scene / dst");
    const size_t ncells = (size_t)s->loc_host.ncx * s->loc_host.ncy;
    const void *src = nullptr;
    size_t n = 0;
    switch (which) {
        case 0: src = s->d_cells, n = ncells * sizeof(uint64_t); break;
        case 1: src = s->d_tiles, n = (size_t)s->tiles * s->tile_d * sizeof(double); break;
        case 2: src = s->d_jtiles, n = (size_t)s->tiles * s->jtile_d * sizeof(double); break;
        case 3: src = s->d_cells8, n = ncells; break;
        case 4: src = s->d_palette, n = (size_t)kPaletteMax * sizeof(uint64_t); break;
        default: return fail(WGRT_ERR_INVALID_ARGUMENT, "which: 0 cells, 1 tiles, 2 jtiles, 3 byte grid, 4 palette");
    }
    if (!src) return fail(WGRT_ERR_UNSUPPORTED, "the scene has no byte grid (wgrt_debug_scene_palette)");
    if (bytes != (int64_t)n) return fail(WGRT_ERR_INVALID_ARGUMENT, "bytes must be " + std::to_string(n));
    DEVICE_SCOPE(dev_scope, s->device);
    HIP_TRY(hipMemcpy(dst, src, n, hipMemcpyDeviceToHost));
    return WGRT_OK;
}

}  // extern "C"
