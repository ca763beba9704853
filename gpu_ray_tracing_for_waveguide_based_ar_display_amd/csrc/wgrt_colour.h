// wgrt_colour.h -- the colour math of AR_system_evaluation_functions.evaluation_from_perceive for ONE
// (FoV, eye position) pixel, compiled for the host AND the device (wgrt_eyebox_evaluate's kernels in
// wgrt_eyebox.hip, wgrt_eyebox_evaluate_host in wgrt_eyebox_host.cpp), and the shapes both sides share.
//
// Every step restates the numpy code operation by operation, in its order (EVAL:112-163 and the
// restated colour / OpenCV pieces beside it); the build's -ffp-contract=off -fno-fast-math keeps
// every product and sum separately rounded.  The float64 part differs between host and device only by
// the last places of the libm calls (pow, cbrt, hypot, atan2, sin, cos, exp); the float32 HSV part is
// IEEE + - * / fmodf floorf only, so it equals numpy's wherever its float64 inputs round to the same
// float32.
#pragma once

#include "wgrt_common.h"

namespace wgrt {

#if !defined(__HIPCC__)
using std::atan2;
using std::cbrt;
using std::cos;
using std::exp;
using std::fmod;
using std::hypot;
using std::pow;
using std::sin;
#endif

// The reduction's shape, shared by the kernels and the host replica so that both add in the same order:
// a tile is kEvTileFov consecutive FoVs, a position chunk kEvPosChunk consecutive eye positions, and the
// tiles' partial records are folded in kEvFoldGroups contiguous groups of ceil(n_tiles / kEvFoldGroups)
// tiles (tile order inside a group, then group order).
constexpr int kEvTileFov = 16;
constexpr int kEvPosChunk = 64;
constexpr int kEvFoldGroups = 16;
constexpr int64_t kEvMaxPos = 1 << 20;   // n_pos limit (the y extent of the launch grid)

constexpr double kEvDeg = 180.0 / 3.14159265358979323846;   // np.degrees
constexpr double kEvRad = 3.14159265358979323846 / 180.0;   // np.radians
constexpr float kEvFltEps = 1.1920928955078125e-07f;        // np.finfo(np.float32).eps

WGRT_HD int64_t ev_tiles(int64_t n_fov) { return (n_fov + kEvTileFov - 1) / kEvTileFov; }

// NULL when (n_fov, n_pos) is a shape wgrt_eyebox_evaluate accepts, else what is wrong with it
inline const char *ev_shape_error(int64_t n_fov, int64_t n_pos) {
    if (n_fov < 1 || n_pos < 1) return "need n_fov >= 1 and n_pos >= 1";
    if (n_pos > kEvMaxPos) return "at most 2^20 eye positions";
    if (n_fov > INT32_MAX / 3 / (1 + n_pos)) return "need 3 * n_fov * (1 + n_pos) <= 2^31 - 1";
    return nullptr;
}

// The same for the whole argument list of wgrt_eyebox_evaluate / _host (include/wgrt.h)
inline const char *ev_args_error(const double *sums, int64_t n_fov, int64_t n_pos, double divisor, const double *wl,
                                 const double *lab_d65, const double *out, const float *image, int64_t image_pos,
                                 const void *workspace) {
    if (const char *why = ev_shape_error(n_fov, n_pos)) return why;
    if (!(divisor > 0.0) || !(divisor <= 1.7976931348623157e308)) return "need a finite divisor > 0";
    if (image_pos < -1 || image_pos >= n_pos) return "need -1 <= image_pos < n_pos";
    if (!sums || !wl || !lab_d65 || !out || !workspace) return "NULL argument";
    if (((uintptr_t)sums | (uintptr_t)out | (uintptr_t)workspace) & 7) return "sums / out / workspace must be 8-B aligned";
    if ((uintptr_t)image & 3) return "image must be 4-B aligned";
    return nullptr;
}

// The caller's workspace: four float64 fields of the (tile, position) partial records, two float64 and one
// float32 value per position, and the records' two 4-byte fields (offsets in ev_workspace below).
inline int64_t ev_workspace_bytes(int64_t n_fov, int64_t n_pos) {
    const int64_t rec = ev_tiles(n_fov) * n_pos;
    return 8 * (4 * rec + 2 * n_pos) + 4 * (2 * rec + n_pos + (n_pos & 1));
}

struct EvWorkspace {
    double *de_sum, *y_min, *y_max, *y_sum;   // [n_tiles * n_pos], record (tile, p) at tile * n_pos + p
    double *pos_de, *pos_ufov;                // [n_pos]
    int32_t *dark;                            // [n_tiles * n_pos]
    float *v_max;                             // [n_tiles * n_pos]
    float *max_v;                             // [n_pos]
};

inline EvWorkspace ev_workspace(void *base, int64_t n_fov, int64_t n_pos) {
    const int64_t rec = ev_tiles(n_fov) * n_pos;
    EvWorkspace w;
    w.de_sum = (double *)base;
    w.y_min = w.de_sum + rec;
    w.y_max = w.y_min + rec;
    w.y_sum = w.y_max + rec;
    w.pos_de = w.y_sum + rec;
    w.pos_ufov = w.pos_de + n_pos;
    w.dark = (int32_t *)(w.pos_ufov + n_pos);
    w.v_max = (float *)(w.dark + rec);
    w.max_v = w.v_max + rec;
    return w;
}

// wl = inv(M_SENSOR) . (1, 1, 1) and LAB_D65, computed once on the host in double (EVAL:47-52, 112-118)
struct EvConsts {
    double wl[3], lab_d65[3];
};

// px[c] = wl[c] * perceive[L - 1 - c], perceive = sum / divisor (EVAL:121: the flip of the wavelength axis)
WGRT_HD void ev_px(double s0, double s1, double s2, double divisor, const EvConsts &k, double px[3]) {
    px[0] = k.wl[0] * (s2 / divisor);
    px[1] = k.wl[1] * (s1 / divisor);
    px[2] = k.wl[2] * (s0 / divisor);
}

WGRT_HD double ev_lab_f(double t) {
    return t > 0.008856451679035631 /* (24 / 116) ** 3 */ ? cbrt(t) : (841.0 / 108.0) * t + 16.0 / 116.0;
}

// np.mod(x, 360) of a finite x in (-360, 360)
WGRT_HD double ev_mod360(double x) {
    double m = fmod(x, 360.0);
    if (m != 0.0) {
        if (m < 0.0) m += 360.0;
    } else {
        m = 0.0;
    }
    return m;
}

WGRT_HD double ev_hue(double b, double ap) {
    return (ap == 0.0 && b == 0.0) ? 0.0 : ev_mod360(atan2(b, ap) * kEvDeg);
}

// delta_e_ciede2000(lab1, lab2), every where branch as written
WGRT_HD double ev_ciede2000(const double lab1[3], const double lab2[3]) {
    const double L1 = lab1[0], a1 = lab1[1], b1 = lab1[2];
    const double L2 = lab2[0], a2 = lab2[1], b2 = lab2[2];
    const double C1 = hypot(a1, b1), C2 = hypot(a2, b2);
    const double Cb7 = pow((C1 + C2) / 2, 7.0);
    const double G = 0.5 * (1 - sqrt(Cb7 / (Cb7 + 6103515625.0)));
    const double a1p = (1 + G) * a1, a2p = (1 + G) * a2;
    const double C1p = hypot(a1p, b1), C2p = hypot(a2p, b2);
    const double h1p = ev_hue(b1, a1p), h2p = ev_hue(b2, a2p);
    const double dLp = L2 - L1;
    const double dCp = C2p - C1p;
    const double dh = h2p - h1p;
    const double prod = C1p * C2p;
    const double dhp = prod == 0.0 ? 0.0 : (dh > 180 ? dh - 360 : (dh < -180 ? dh + 360 : dh));
    const double dHp = 2 * sqrt(prod) * sin((dhp / 2) * kEvRad);
    const double Lbp = (L1 + L2) / 2;
    const double Cbp = (C1p + C2p) / 2;
    const double hsum = h1p + h2p;
    const double hbp = prod == 0.0 ? hsum
                                   : (fabs(h1p - h2p) <= 180 ? hsum / 2 : (hsum < 360 ? (hsum + 360) / 2 : (hsum - 360) / 2));
    const double T = 1 - 0.17 * cos((hbp - 30) * kEvRad) + 0.24 * cos((2 * hbp) * kEvRad) +
                     0.32 * cos((3 * hbp + 6) * kEvRad) - 0.20 * cos((4 * hbp - 63) * kEvRad);
    const double u = (hbp - 275) / 25;
    const double dtheta = 30 * exp(-(u * u));
    const double Cbp7 = pow(Cbp, 7.0);
    const double RC = 2 * sqrt(Cbp7 / (Cbp7 + 6103515625.0));
    const double l50 = Lbp - 50;
    const double SL = 1 + 0.015 * (l50 * l50) / sqrt(20 + l50 * l50);
    const double SC = 1 + 0.045 * Cbp;
    const double SH = 1 + 0.015 * Cbp * T;
    const double RT = -sin((2 * dtheta) * kEvRad) * RC;
    const double tl = dLp / SL, tc = dCp / SC, th = dHp / SH;
    return sqrt(tl * tl + tc * tc + th * th + RT * tc * th);
}

// The colour side of one pixel (EVAL:128-133): Y of M_XYZ . px and the CIEDE2000 difference to D65
WGRT_HD void ev_colour(const double px[3], const EvConsts &k, double &Y, double &de) {
    const double X = 6.424000e-01 * px[0] + 1.891400e-01 * px[1] + 2.511000e-01 * px[2];
    Y = 2.650000e-01 * px[0] + 8.849624e-01 * px[1] + 7.390000e-02 * px[2];
    const double Z = 4.999999e-05 * px[0] + 3.693564e-02 * px[1] + 1.528100e+00 * px[2];
    const double d = Y > 1e-10 ? Y : 1e-10;
    const double xn = X / d * 100, yn = Y / d * 100, zn = Z / d * 100;
    constexpr double Xn = 0.3127 / 0.3290, Zn = (1 - 0.3127 - 0.3290) / 0.3290;
    const double fx = ev_lab_f(xn / Xn), fy = ev_lab_f(yn / 1.0), fz = ev_lab_f(zn / Zn);
    double lab[3] = {116 * fy - 16, 500 * (fx - fy), 200 * (fy - fz)};
    if (Y == 0.0) lab[0] = lab[1] = lab[2] = 0.0;
    de = ev_ciede2000(lab, k.lab_d65);
}

WGRT_HD double ev_gamma(double x) {
    x = x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x);   // np.clip(., 0, 1): a NaN passes
    return x <= 0.0031308 ? x * 12.92 : 1.055 * pow(x, 1 / 2.4) - 0.055;
}

// The image side before the normalisation (EVAL:126-127): clip(M_SENSOR . px), sRGB gamma, the float32 cast
// and rgb_to_hsv_f32
WGRT_HD void ev_hsv(const double px[3], float &h, float &s, float &v) {
    const float r = (float)ev_gamma(1.67430115 * px[0] + -0.76582385 * px[1] + -0.06172232 * px[2]);
    const float g = (float)ev_gamma(-0.12551154 * px[0] + 1.47840695 * px[1] + -0.04124377 * px[2]);
    const float b = (float)ev_gamma(-0.01826868 * px[0] + -0.13098157 * px[1] + 1.61444037 * px[2]);
    const float rg = r > g ? r : g, rgm = r < g ? r : g;
    v = rg > b ? rg : b;
    const float vmin = rgm < b ? rgm : b;
    const float diff = v - vmin;
    s = diff / (fabsf(v) + kEvFltEps);
    const float k = 60.0f / (diff + kEvFltEps);
    h = v == r ? (g - b) * k : (v == g ? (b - r) * k + 120.0f : (r - g) * k + 240.0f);
    if (h < 0) h = h + 360.0f;
}

// v / max_v (when max_v > 0) and hsv_to_rgb_f32.  `bad` keeps every input, NaN included, inside the six
// sectors: the sector only selects among four values, it indexes nothing.
WGRT_HD void ev_image_rgb(float h, float s, float v, float max_v, float rgb[3]) {
    if (max_v > 0) v = v / max_v;
    h = h * (float)(6.0 / 360.0);
    float m = fmodf(h, 6.0f);   // np.mod(h, 6)
    if (m != 0.0f) {
        if (m < 0.0f) m += 6.0f;
    } else {
        m = 0.0f;
    }
    const float fl = floorf(m);
    const bool bad = !(fl >= 0.0f && fl < 6.0f);
    const int sector = bad ? 0 : (int)fl;
    const float f = bad ? 0.0f : m - fl;
    const float t0 = v, t1 = v * (1.0f - s), t2 = v * (1.0f - s * f), t3 = v * (1.0f - s * (1.0f - f));
    // OpenCV's sector table, (b, g, r) as indices into (t0, t1, t2, t3):
    // {1, 3, 0}, {1, 0, 2}, {3, 0, 1}, {0, 2, 1}, {0, 1, 3}, {2, 1, 0}
    float bb, gg, rr;
    switch (sector) {
    case 0: bb = t1, gg = t3, rr = t0; break;
    case 1: bb = t1, gg = t0, rr = t2; break;
    case 2: bb = t3, gg = t0, rr = t1; break;
    case 3: bb = t0, gg = t2, rr = t1; break;
    case 4: bb = t0, gg = t1, rr = t3; break;
    default: bb = t2, gg = t1, rr = t0; break;
    }
    const bool grey = s == 0.0f;
    rgb[0] = grey ? v : rr;
    rgb[1] = grey ? v : gg;
    rgb[2] = grey ? v : bb;
}

// One (tile, position) partial record while it is being accumulated, and the rules of EVAL:150-163
struct EvRecord {
    double de_sum, y_min, y_max, y_sum;
    int32_t dark;
    float v_max;
};

WGRT_HD EvRecord ev_record_empty() {
    EvRecord r;
    r.de_sum = 0.0;
    r.y_min = INFINITY;
    r.y_max = -INFINITY;
    r.y_sum = 0.0;
    r.dark = 0;
    r.v_max = -INFINITY;
    return r;
}

WGRT_HD void ev_record_add(EvRecord &r, const EvRecord &o) {
    r.de_sum += o.de_sum;
    r.y_min = o.y_min < r.y_min ? o.y_min : r.y_min;
    r.y_max = o.y_max > r.y_max ? o.y_max : r.y_max;
    r.y_sum += o.y_sum;
    r.dark |= o.dark;
    r.v_max = o.v_max > r.v_max ? o.v_max : r.v_max;
}

WGRT_HD void ev_record_pixel(EvRecord &r, double de, double Y, float v) {
    r.de_sum += de;
    r.y_min = Y < r.y_min ? Y : r.y_min;
    r.y_max = Y > r.y_max ? Y : r.y_max;
    r.y_sum += Y;
    r.dark |= Y == 0.0;
    r.v_max = v > r.v_max ? v : r.v_max;
}

// One eye position from its folded record: the mean of delta E, its U_fov term and U_EB[i, j]
WGRT_HD void ev_position(const EvRecord &r, int64_t n_fov, double &de_mean, double &ufov, double &ueb) {
    de_mean = r.de_sum / (double)n_fov;
    if (r.dark) {
        ufov = 0.0;
        ueb = 0.0;
    } else {
        ufov = r.y_min / r.y_max;
        ueb = r.y_sum / (double)n_fov;
    }
}

// The three figures from the per-position values, in position order
WGRT_HD void ev_totals(const double *pos_de, const double *pos_ufov, const double *pos_ueb, int64_t n_pos,
                       double out3[3]) {
    double de = 0.0, uf = 0.0, mn = pos_ueb[0], mx = pos_ueb[0];
    for (int64_t p = 0; p < n_pos; ++p) {
        de += pos_de[p];
        uf += pos_ufov[p];
        mn = pos_ueb[p] < mn ? pos_ueb[p] : mn;
        mx = pos_ueb[p] > mx ? pos_ueb[p] : mx;
    }
    out3[0] = de / (double)n_pos;
    out3[1] = uf / (double)n_pos;
    out3[2] = mx == 0.0 ? 0.0 : mn / mx;
}

}  // namespace wgrt
