// Forward-backward consistency gate (lfd_cycle_gate): the per-cell arithmetic, compiled for the device (lfd_cycle.hip) and for
// the host (lfd_host.hip's twin).  A cell of the reference grid is followed to the neighbour with warp_AB and back with warp_BA; it keeps
// its (floored) certainty iff it lands within cycle_thresh_px of where it started, else its certainty becomes exactly 0.
//
// Every rounding is written out (the build uses -ffp-contract=off): the twin and the kernels execute the same f32 operations in the same
// order, so cert_out and the counters agree bit for bit.
#pragma once

#include <stdint.h>

#include "../../include/lfd_densify.h"
#include "lfd_geometry.hpp"

#define LFD_CYCLE_MAX_GRID 32768

// The four texels of warp_BA round one sample (texel indices y * Wb + x, CLAMPED to the grid: padding_mode="border") and their weights.
struct LfdCycleTaps {
    int32_t i00, i01, i10, i11;
    float w00, w01, w10, w11;
};

// false: (xb, yb) lies outside [-1, 1]^2 or is NaN - the cell is rejected and `t` names texel 0 four times with weight 0, so that a caller
// without branches still reads inside the grid.  No address is ever formed from such a coordinate.  A coordinate that passes has
// -0.5 <= ix <= Wb - 0.5 with Wb <= 2^15: floorf(ix) converts exactly.  ix is the expression of lfd_grid_nearest / lfd_corr_taps
// (F.grid_sample, align_corners=False).
LFD_HD bool lfd_cycle_taps(float xb, float yb, int32_t Wb, int32_t Hb, LfdCycleTaps& t) {
    const bool inside = xb >= -1.0f && xb <= 1.0f && yb >= -1.0f && yb <= 1.0f;
    const float sxb = inside ? xb : 0.0f, syb = inside ? yb : 0.0f;
    const float ix = ((sxb + 1.0f) * (float)Wb - 1.0f) / 2.0f;
    const float iy = ((syb + 1.0f) * (float)Hb - 1.0f) / 2.0f;
    const float fx = floorf(ix), fy = floorf(iy);
    const int32_t x0 = (int32_t)fx, y0 = (int32_t)fy;                  // in [-1, Wb - 1], [-1, Hb - 1]
    const float wx1 = ix - fx, wy1 = iy - fy;
    const float wx0 = (fx + 1.0f) - ix, wy0 = (fy + 1.0f) - iy;
    const int32_t cx0 = x0 < 0 ? 0 : x0, cx1 = x0 + 1 > Wb - 1 ? Wb - 1 : x0 + 1;
    const int32_t cy0 = y0 < 0 ? 0 : y0, cy1 = y0 + 1 > Hb - 1 ? Hb - 1 : y0 + 1;
    t.i00 = inside ? cy0 * Wb + cx0 : 0; t.i01 = inside ? cy0 * Wb + cx1 : 0;
    t.i10 = inside ? cy1 * Wb + cx0 : 0; t.i11 = inside ? cy1 * Wb + cx1 : 0;
    t.w00 = inside ? wy0 * wx0 : 0.0f; t.w01 = inside ? wy0 * wx1 : 0.0f;
    t.w10 = inside ? wy1 * wx0 : 0.0f; t.w11 = inside ? wy1 * wx1 : 0.0f;
    return inside;
}

// one channel of warp_BA blended: upper row, lower row, their sum
LFD_HD float lfd_cycle_blend(const LfdCycleTaps& t, float v00, float v01, float v10, float v11) {
    const float top = t.w00 * v00 + t.w01 * v01;
    const float bot = t.w10 * v10 + t.w11 * v11;
    return top + bot;
}

// squared cycle error in pixels of the match image: upstream's pixel conversion (n + 1) / 2 * (size - 1) applied to a difference
LFD_HD float lfd_cycle_d2(float xa2, float ya2, float xa, float ya, float wm1, float hm1) {
    const float dx = ((xa2 - xa) * 0.5f) * wm1;
    const float dy = ((ya2 - ya) * 0.5f) * hm1;
    return dx * dx + dy * dy;
}

// The decision from the eight texel values: `inside` from lfd_cycle_taps.  keep iff d2 <= tau2 (false for NaN); *d2_out = +inf outside.
LFD_HD bool lfd_cycle_decide(const LfdCycleTaps& t, bool inside, float x00, float y00, float x01, float y01, float x10, float y10, float x11,
                             float y11, float xa, float ya, float wm1, float hm1, float tau2, float& d2_out) {
    const float xa2 = lfd_cycle_blend(t, x00, x01, x10, x11), ya2 = lfd_cycle_blend(t, y00, y01, y10, y11);
    const float d2 = inside ? lfd_cycle_d2(xa2, ya2, xa, ya, wm1, hm1) : INFINITY;
    d2_out = d2;
    return inside && d2 <= tau2;
}

// One cell with plain loads (the twin, and the kernel for layouts the vector kernel does not take).  wba: f32 [Hb * Wb * 2].
LFD_HD bool lfd_cycle_cell(const float* wba, int32_t Wb, int32_t Hb, float xa, float ya, float xb, float yb, float wm1, float hm1, float tau2,
                           float& d2_out) {
    LfdCycleTaps t;
    const bool inside = lfd_cycle_taps(xb, yb, Wb, Hb, t);
    const float* p00 = wba + 2 * (size_t)t.i00;
    const float* p01 = wba + 2 * (size_t)t.i01;
    const float* p10 = wba + 2 * (size_t)t.i10;
    const float* p11 = wba + 2 * (size_t)t.i11;
    return lfd_cycle_decide(t, inside, p00[0], p00[1], p01[0], p01[1], p10[0], p10[1], p11[0], p11[1], xa, ya, wm1, hm1, tau2, d2_out);
}

// What a launch (or the twin) works on; the pointers of the pairs travel by value in the kernel arguments.
struct LfdCycleArgs {
    const float* cert[LFD_MAX_SLOTS];
    const float* warp_ab[LFD_MAX_SLOTS];
    const float* warp_ba[LFD_MAX_SLOTS];
    float* cert_out[LFD_MAX_SLOTS];
    float* err_out[LFD_MAX_SLOTS];       // all null when no error plane is wanted
    int32_t* rejected;                   // [n_pairs], added to; or null
    const float* axis_x;                 // both null: the identity axes below
    const float* axis_y;
    LfdAxis ax, ay;
    int32_t n_pairs, H, W, C, Hb, Wb;
    float wm1, hm1, certainty_thresh, tau2;
};

// Arguments of lfd_cycle_gate / lfd_cycle_gate_host -> LfdCycleArgs; what is wrong with them, or null.
inline const char* lfd_cycle_fill(int32_t n_pairs, const float* const* cert, const float* const* warp_ab, const float* const* warp_ba, int32_t H,
                                  int32_t W, int32_t warp_channels, int32_t Hb, int32_t Wb, const float* axis_x, const float* axis_y,
                                  int32_t w_match, int32_t h_match, float certainty_thresh, float cycle_thresh_px, float* const* cert_out,
                                  float* const* err_out, int32_t* rejected, LfdCycleArgs& p) {
    if (n_pairs < 1 || n_pairs > LFD_MAX_SLOTS) return "n_pairs must be in [1, LFD_MAX_SLOTS]";
    if (H < 1 || W < 1 || Hb < 1 || Wb < 1 || H > LFD_CYCLE_MAX_GRID || W > LFD_CYCLE_MAX_GRID || Hb > LFD_CYCLE_MAX_GRID || Wb > LFD_CYCLE_MAX_GRID)
        return "H, W, Hb, Wb must be in [1, 32768]";
    if (w_match < 1 || h_match < 1 || w_match >= (1 << 24) || h_match >= (1 << 24)) return "w_match and h_match must be in [1, 2^24)";
    if (warp_channels != 2 && warp_channels != 4) return "warp_channels must be 2 or 4";
    if (!(cycle_thresh_px > 0.0f) || !(cycle_thresh_px <= 3.4028234e38f)) return "cycle_thresh_px must be finite and > 0";
    if (!cert || !warp_ab || !warp_ba || !cert_out) return "null pointer table";
    if ((axis_x == nullptr) != (axis_y == nullptr)) return "axis_x and axis_y must both be given or both be null";
    for (int i = 0; i < LFD_MAX_SLOTS; ++i) {
        const bool live = i < n_pairs;
        if (live && (!cert[i] || !warp_ab[i] || !warp_ba[i] || !cert_out[i] || (err_out && !err_out[i]))) return "null pointer in a pair";
        p.cert[i] = live ? cert[i] : nullptr; p.warp_ab[i] = live ? warp_ab[i] : nullptr; p.warp_ba[i] = live ? warp_ba[i] : nullptr;
        p.cert_out[i] = live ? cert_out[i] : nullptr; p.err_out[i] = (live && err_out) ? err_out[i] : nullptr;
    }
    p.rejected = rejected; p.axis_x = axis_x; p.axis_y = axis_y;
    p.ax = lfd_make_axis(W); p.ay = lfd_make_axis(H);
    p.n_pairs = n_pairs; p.H = H; p.W = W; p.C = warp_channels; p.Hb = Hb; p.Wb = Wb;
    p.wm1 = (float)(w_match - 1); p.hm1 = (float)(h_match - 1);
    p.certainty_thresh = certainty_thresh;
    p.tau2 = cycle_thresh_px * cycle_thresh_px;      // the f32 square, once: no division or square root decides anything
    return nullptr;
}
