// wgrt_locator.h -- the exact polygon locator on the device (wgrt_scene_build.cpp builds its grid): a
// point's cell word, and is_inside_or_on_edge (GRTF:63-71) from the cell's class or, for an EDGE class,
// from the reference predicate over the polygon's edges that meet the cell's row.
#pragma once

#include "wgrt_args.h"

namespace wgrt {

constexpr int kPolyEff1 = 0;
constexpr int kPolyEff2 = 1;
constexpr int kPolyIC = 2;
constexpr int kPolyFC0 = 3;


// A point's cell of the locator grid: the per-polygon class word and the cell row.
struct Cell {
    uint64_t w;
    int cy;
};

template <class Loc>
__device__ __forceinline__ Cell locate(const Loc &L, double x, double y) {
    const double fx = floor((x - L.x0) * L.inv_h);
    const double fy = floor((y - L.y0) * L.inv_h);
    // NaN / out-of-grid points are outside every polygon (cell word 0 = all OUT)
    if (!(fx >= 0.0 && fy >= 0.0 && fx < (double)L.ncx && fy < (double)L.ncy)) return Cell{0ull, 0};
    const int cx = (int)fx, cy = (int)fy;
    return Cell{(uint64_t)L.cells[cy * L.ncx + cx], cy};
}

// is_inside_or_on_edge(x, y, polygon k) (GRTF:63-71): the cell class when the cell is IN or
// OUT, else the reference predicate over the polygon's edges that meet the cell's row.
template <class Loc>
__device__ __forceinline__ bool in_poly(const Loc &L, const Cell &c, int k, double x, double y) {
    const unsigned cls = (unsigned)(c.w >> (2 * k)) & 3u;
    if (__builtin_expect(cls != 2u, 1)) return cls == 1u;   // IN / OUT; EDGE cells are rare (0.34 % of C3 lane-passes)
    const int a = L.poly_off[k], nv = L.poly_off[k + 1] - a;
    const int r = k * L.ncy + c.cy;
    const int e0 = L.row_off[r], e1 = L.row_off[r + 1];
    return inside_or_on_edge_subset(x, y, L.verts + 2 * a, nv, L.row_edges + e0, e1 - e0);
}

// First slice s in [0, count) of polygons first .. first + count - 1 containing (x, y),
// -1 if none (the slice scans of GRTF:1002-1005 and GRTF:1112-1115, which stop at the
// first hit).  Candidates come straight from the cell word: a slice is tested exactly only
// when its class is EDGE; an IN slice is a hit; OUT slices are skipped.
template <class Loc>
__device__ __forceinline__ int first_slice(const Loc &L, const Cell &c, int first, int count,
                                           double x, double y) {
    uint64_t f = c.w >> (2 * first);
    if (count < 32) f &= (1ull << (2 * count)) - 1ull;
    const uint64_t in = f & 0x5555555555555555ull;           // class 01
    uint64_t cand = in | ((f >> 1) & 0x5555555555555555ull);  // class 01 or 10
    while (cand != 0ull) {
        const int p = __builtin_ctzll(cand);
        const int s = p >> 1;
        if ((in >> p) & 1ull) return s;
        if (in_poly(L, c, first + s, x, y)) return s;
        cand &= cand - 1ull;
    }
    return -1;
}

// Word-only forms for the Jones-vector lane: a cell is just its class word (the row of an
// EDGE cell is recomputed from y on the rare exact test), which keeps prefetched cells in one
// register each.
template <class Loc>
__device__ __forceinline__ typename Loc::Word locate_w(const Loc &L, double x, double y) {
    const double fx = floor((x - L.x0) * L.inv_h);
    const double fy = floor((y - L.y0) * L.inv_h);
    if (!(fx >= 0.0 && fy >= 0.0 && fx < (double)L.ncx && fy < (double)L.ncy)) return 0;
    return L.cells[(int)fy * L.ncx + (int)fx];
}

// The exact test of an EDGE class.  Kp: the launch's kernarg handle -- the locator's array pointers
// are then read from the kernarg segment (not held in SGPRs across the Jones loop); NULL: from L.
// Every reader takes the handle as an argument, so the test is also correct as a real call (a noinline
// build ran the parity tests green); inlined, it keeps the wave loop free of a call's
// register cost.
template <class Loc>
__device__ __forceinline__ bool in_poly_w(const Loc &L, typename Loc::Word w, int k, double x, double y,
                                          const KArgs *Kp = nullptr) {
    const unsigned cls = (unsigned)(w >> (2 * k)) & 3u;
    if (__builtin_expect(cls != 2u, 1)) return cls == 1u;   // IN / OUT; EDGE cells are rare (0.34 % of C3 lane-passes)
    const int cy = (int)floor((y - L.y0) * L.inv_h);   // an EDGE cell is inside the grid
    const int r = k * L.ncy + cy;
    const bool KARG = Kp != nullptr;
    // one 128-B record: the (at most kBandSegs) edges of polygon k meeting this cell row,
    // evaluated with the reference predicate's operations (GRTF:36-71); NaN slots are inert
    const double *const bands = KARG ? KLOCP(Kp, bands) : L.bands;
    const double4 *rec = (const double4 *)(bands + (size_t)r * 4 * kBandSegs);
    const double4 s0 = rec[0], s1 = rec[1], s2 = rec[2], s3 = rec[3];
    if (__builtin_expect(s0.x != INFINITY, 1)) {   // else: a row with more edges than a band record holds
        bool inside = false;
        const double4 sg[kBandSegs] = {s0, s1, s2, s3};
#pragma unroll
        for (int e = 0; e < kBandSegs; ++e) {
            const double xj = sg[e].x, yj = sg[e].y, xi = sg[e].z, yi = sg[e].w;
            if (on_segment(x, y, xj, yj, xi, yi)) return true;
            if (((yi > y) != (yj > y)) && (x < (xj - xi) * (y - yi) / (yj - yi + 1e-20) + xi)) inside = !inside;
        }
        return inside;
    }
    const int32_t *const po = KARG ? KLOCP(Kp, poly_off) : L.poly_off;
    const int32_t *const ro = KARG ? KLOCP(Kp, row_off) : L.row_off;
    const int a = po[k], nv = po[k + 1] - a;
    const int e0 = ro[r], e1 = ro[r + 1];
    return inside_or_on_edge_subset(x, y, (KARG ? KLOCP(Kp, verts) : L.verts) + 2 * a, nv,
                                    (KARG ? KLOCP(Kp, row_edges) : L.row_edges) + e0, e1 - e0);
}

// Cell word of (x, y): the grid has a border of all-OUT cells, so clamping is exact for points
// outside it (and for NaN, which converts to 0).  The byte form (ByteLocatorT) loads the cell's palette index
// with the same clamp and the same index.
template <class Loc>
__device__ __forceinline__ typename Loc::Cell locate_c(const Loc &L, double x, double y) {
    int ix = (int)((x - L.x0) * L.inv_h), iy = (int)((y - L.y0) * L.inv_h);
    ix = min(max(ix, 0), L.ncx - 1);
    iy = min(max(iy, 0), L.ncy - 1);
    return L.cells[iy * L.ncx + ix];
}

}  // namespace wgrt
