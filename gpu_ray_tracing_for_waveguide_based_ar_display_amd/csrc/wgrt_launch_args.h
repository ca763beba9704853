// wgrt_launch_args.h -- the one place that turns (scene, rays) into kernel arguments, for the two units that
// launch lanes over a ray batch: wgrt_trace.hip (fill_args adds what only a trace launch has: order, scratch,
// timeline, fused) and wgrt_shadow.hip (wgrt_debug_shadow).
#pragma once

#include "wgrt_jones_lane.h"
#include "wgrt_scene.h"

namespace wgrt {

// The "NULL ray column" check: every column the kernels read (lmd_num only in full colour) is there.
inline bool ray_columns_present(const wgrt_rays *rays, bool single) {
    return rays->x && rays->y && rays->m && rays->n && (single || rays->lmd_num) && rays->te && rays->tm &&
           rays->delta_phase;
}

// The arguments that come from the scene and the ray columns; everything else is zero.  single: the
// single-wavelength kernel process_rays_kernel_pro (GRTF:419-831) -- no lmd_num column, wavelength 0 of a
// one-wavelength scene, threshold 1e-15; otherwise process_rays_kernel_pro_fullColor (GRTF:833-1246), threshold
// 0.  The two kernels differ in nothing else.  The certification bounds are the product lane's defaults.
inline TraceArgs scene_ray_args(const wgrt_scene *s, const wgrt_rays *rays, bool single) {
    TraceArgs A{};
    A.x = rays->x;
    A.y = rays->y;
    A.m = rays->m;
    A.n = rays->n;
    A.l = single ? nullptr : rays->lmd_num;
    A.threshold = single ? 1e-15 : 0.0;
    A.te = rays->te;
    A.tm = rays->tm;
    A.dph = rays->delta_phase;
    A.tiles = s->d_tiles;
    A.loc = make_locator(s);
    A.tile_d = s->tile_d;
    A.jtiles = s->d_jtiles;
    A.jtile_d = s->jtile_d;
    A.nfc = s->nfc;
    A.noc = s->noc;
    A.nx = s->nx;
    A.ny = s->ny;
    A.nl = s->nl;
    A.n_g = s->n_g;
    A.inv_n_g = 1.0 / s->n_g;
    A.cert_tol = kCertTol;
    A.cert_tol32 = kCertTol32;
    return A;
}

}  // namespace wgrt
