// Multi-view point colour (lfd_colour_multiview): the per-point routine, compiled for the device (lfd_colour.hip) and for the host
// (lfd_host.hip's twin).  A point's colour becomes the mean or the median, per channel, of what the views that see it say: its reference (the
// colour it carries), the neighbour that won it, and every other neighbour of the reference that lfd_support_candidate accepts for it - the
// support filter's and the re-triangulation's set, by the same routine.  A neighbour's colour is lfd_bilinear_rgb_f32 of its match-size image
// at the match pixel of its observation: the blend the triangulation kernels use for the reference, not a second one.
//
// Every rounding is written out (the build uses -ffp-contract=off), nothing is divided: the twin and the kernel execute the same f32 operations
// in the same order and agree bit for bit.  A column rewrite, not a filter: no point, count or order changes.
#pragma once

#include <stdint.h>

#include "../../include/lfd_densify.h"
#include "lfd_geometry.hpp"
#include "lfd_support.hpp"

#if defined(__HIP_DEVICE_COMPILE__)
#define LFD_COLOUR_UNROLL _Pragma("unroll")
#else
#define LFD_COLOUR_UNROLL
#endif

// RN_f32(1 / n), n = 1 .. LFD_MAX_SLOTS + 1: 1 / n in f64 rounded once to f32 (the convention of lfd_blend4_weights_f32's 1 / 255)
LFD_HD float lfd_colour_recip(int n) {
    static_assert(LFD_MAX_SLOTS == 16, "the table below has LFD_MAX_SLOTS + 1 entries");
    switch (n) {
        case 2: return 0x1.000000p-1f;
        case 3: return 0x1.555556p-2f;
        case 4: return 0x1.000000p-2f;
        case 5: return 0x1.99999ap-3f;
        case 6: return 0x1.555556p-3f;
        case 7: return 0x1.24924ap-3f;
        case 8: return 0x1.000000p-3f;
        case 9: return 0x1.c71c72p-4f;
        case 10: return 0x1.99999ap-4f;
        case 11: return 0x1.745d18p-4f;
        case 12: return 0x1.555556p-4f;
        case 13: return 0x1.3b13b2p-4f;
        case 14: return 0x1.24924ap-4f;
        case 15: return 0x1.111112p-4f;
        case 16: return 0x1.000000p-4f;
        case 17: return 0x1.e1e1e2p-5f;
        default: return 1.0f;
    }
}

// The guard: such a point keeps its colour bit for bit with status 0, and no address is formed from its cell or its slot.
LFD_HD bool lfd_colour_guarded(float X0, float X1, float X2, float r, float g, float b, int cell, long long HW, int s, int ns) {
    const bool finite = lfd_finite(X0) && lfd_finite(X1) && lfd_finite(X2) && lfd_finite(r) && lfd_finite(g) && lfd_finite(b);
    return !finite || cell < 0 || (long long)cell >= HW || s >= ns;
}

// The colour neighbour image `img` has at the observation (xb, yb) (normalised, as the warp stores it)
LFD_HD void lfd_colour_sample(const uint8_t* img, const LfdSupportGeom& g, float xb, float yb, float* rgb) {
    lfd_bilinear_rgb_f32(img, g.w_match, g.h_match, lfd_match_px(xb, g.wm1), lfd_match_px(yb, g.hm1), rgb);
}

// The value at position m0 (and m1) of the ascending order of v[0 .. N)[ch], by counting: rank(a) = #{b < a: v[b] <= v[a]} + #{b > a: v[b] <
// v[a]} is a permutation of 0 .. N - 1 (equal values rank by index).  Entries that take no part hold +inf and rank behind every one that does.
template <int N>
LFD_HD float lfd_colour_median(const float (&v)[N][3], int ch, int n) {
    const int m0 = (n - 1) >> 1, m1 = n >> 1;
    float lo = 0.0f, hi = 0.0f;
    LFD_COLOUR_UNROLL
    for (int a = 0; a < N; ++a) {
        int rank = 0;
        LFD_COLOUR_UNROLL
        for (int b = 0; b < N; ++b) {
            if (b < a) rank += (v[b][ch] <= v[a][ch]) ? 1 : 0;
            if (b > a) rank += (v[b][ch] < v[a][ch]) ? 1 : 0;
        }
        lo = (rank == m0) ? v[a][ch] : lo;
        hi = (rank == m1) ? v[a][ch] : hi;
    }
    return (m0 == m1) ? lo : (lo + hi) * 0.5f;
}

// One point that passed the guard.  sl, img: the slots of its reference and their images, [ns]; s < ns: the winning slot, (wsx, wsy) its
// observation at the point's cell; c, wx, wy: [KMAX] certainty and observation of every OTHER slot j < ns at the cell (index s is not read).
// rgb: in, the reference's colour; out, the blend.  Returns n, the number of views blended (>= 1).
template <int KMAX, int MODE>
LFD_HD unsigned lfd_colour_point(const LfdSlot* sl, const uint8_t* const* img, int ns, int s, const LfdSupportGeom& g, const float* c,
                                 const float* wx, const float* wy, float wsx, float wsy, float X0, float X1, float X2, float* rgb) {
    const bool winner = lfd_finite(wsx) && lfd_finite(wsy);
    int n = 1;
    if (MODE == LFD_COLOUR_MEAN) {
        float sum[3] = {rgb[0], rgb[1], rgb[2]};
        if (winner) {
            float v[3];
            lfd_colour_sample(img[s], g, wsx, wsy, v);
            sum[0] = sum[0] + v[0]; sum[1] = sum[1] + v[1]; sum[2] = sum[2] + v[2];
            ++n;
        }
        LFD_COLOUR_UNROLL
        for (int j = 0; j < KMAX; ++j) {
            if (j < ns && j != s && lfd_support_candidate(sl[j], g, c[j], wx[j], wy[j], X0, X1, X2)) {
                float v[3];
                lfd_colour_sample(img[j], g, wx[j], wy[j], v);
                sum[0] = sum[0] + v[0]; sum[1] = sum[1] + v[1]; sum[2] = sum[2] + v[2];
                ++n;
            }
        }
        const float rn = lfd_colour_recip(n);
        rgb[0] = sum[0] * rn; rgb[1] = sum[1] * rn; rgb[2] = sum[2] * rn;
    } else {
        const float inf = __builtin_huge_valf();
        float v[KMAX + 1][3];
        v[0][0] = rgb[0]; v[0][1] = rgb[1]; v[0][2] = rgb[2];
        float w[3] = {inf, inf, inf};
        if (winner) {
            lfd_colour_sample(img[s], g, wsx, wsy, w);
            ++n;
        }
        LFD_COLOUR_UNROLL
        for (int j = 0; j < KMAX; ++j) {
            float u[3] = {inf, inf, inf};
            if (j < ns && j != s && lfd_support_candidate(sl[j], g, c[j], wx[j], wy[j], X0, X1, X2)) {
                lfd_colour_sample(img[j], g, wx[j], wy[j], u);
                ++n;
            }
            const bool is_s = j == s;
            v[j + 1][0] = is_s ? w[0] : u[0]; v[j + 1][1] = is_s ? w[1] : u[1]; v[j + 1][2] = is_s ? w[2] : u[2];
        }
        rgb[0] = lfd_colour_median<KMAX + 1>(v, 0, n);
        rgb[1] = lfd_colour_median<KMAX + 1>(v, 1, n);
        rgb[2] = lfd_colour_median<KMAX + 1>(v, 2, n);
    }
    return (unsigned)n;
}

// What a launch works on (device), by value in the kernel arguments.
struct LfdColourArgs {
    LfdPointStage st;                  // (g.reproj_thresh unused)
    const uint8_t* const* img;         // [n_refs * k] the neighbours' match-size images (device table)
    float* o_rgb;                      // [3 * capacity]; may be st.rgb itself
    uint8_t* status;                   // [capacity] or null
    unsigned long long* counters;      // [2] or null: points blended, the sum of their n; added to
    int32_t mode;
};

// Arguments of lfd_colour_multiview / lfd_colour_multiview_host that do not depend on the batch; what is wrong with them, or null.
inline const char* lfd_colour_check(const lfd_points* in, const int64_t* ref_offsets, const uint8_t* const* nbr_image, float support_thresh_px,
                                    int32_t mode, const float* rgb_out, const uint8_t* status) {
    if (!in || !ref_offsets || !nbr_image) return "null in / ref_offsets / nbr_image";
    if (!in->xyz || !rgb_out) return "null point arrays";
    if (!in->cell || !in->slot || !in->rgb) return "in->cell, in->slot and in->rgb are required";
    if (in->capacity < 0 || in->capacity > 0x7fffffffLL) return "capacity must be in [0, 2^31 - 1]";
    if (mode != LFD_COLOUR_MEAN && mode != LFD_COLOUR_MEDIAN) return "mode must be 1 (mean) or 2 (median)";
    if (!(support_thresh_px > 0.0f) || !(support_thresh_px <= 3.4028234e38f)) return "support_thresh_px must be finite and > 0";
    const long long cap = in->capacity;
    const struct { const void* p; long long elem; } a[5] = {{in->xyz, 12}, {in->rgb, 12}, {in->err, 4}, {in->cell, 4}, {in->slot, 1}},
                                                    b[2] = {{rgb_out, 12}, {status, 1}};
    for (int j = 0; j < 2; ++j) {
        if (!b[j].p) continue;
        const uintptr_t b0 = reinterpret_cast<uintptr_t>(b[j].p), b1 = b0 + (uintptr_t)(b[j].elem * cap);
        for (int i = 0; i < 5; ++i) {
            if (!a[i].p || (j == 0 && i == 1 && rgb_out == in->rgb)) continue;       // (in place: every point is independent)
            const uintptr_t a0 = reinterpret_cast<uintptr_t>(a[i].p), a1 = a0 + (uintptr_t)(a[i].elem * cap);
            if (a0 < b1 && b0 < a1) return "rgb_out must be in->rgb itself or overlap nothing of in; status must overlap nothing of in";
        }
    }
    if (status) {
        const uintptr_t a0 = reinterpret_cast<uintptr_t>(rgb_out), a1 = a0 + (uintptr_t)(12 * cap);
        const uintptr_t b0 = reinterpret_cast<uintptr_t>(status), b1 = b0 + (uintptr_t)cap;
        if (a0 < b1 && b0 < a1) return "rgb_out and status overlap each other";
    }
    return nullptr;
}

// ... and the one that does: every valid slot needs its image.
inline const char* lfd_colour_check_images(const lfd_batch* b, const uint8_t* const* nbr_image) {
    for (int r = 0; r < b->n_refs; ++r)
        for (int j = 0; j < b->n_slots[r]; ++j)
            if (!nbr_image[(size_t)r * b->k + j]) return "null image in a valid slot";
    return nullptr;
}
