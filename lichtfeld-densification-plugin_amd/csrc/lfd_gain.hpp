// Per-image exposure gains (lfd_gain_accumulate / lfd_gain_apply): the per-sample and per-value routines, compiled for the device
// (lfd_gain.hip) and for the host (lfd_host.hip's twins).  While a reference is resident every point carries the reference's colour and, for
// each view that confirms it, that view's colour at the same surface point: a sample of the brightness ratio of two images.  The views, the
// guard and the sampling are lfd_colour.hpp's (the multi-view colour) - no second candidate test, no second blend.
//
// A sample is six f32 values in [0.05, 0.95] (clipped pixels are not linear), each quantised exactly - a multiplication by 2^24, then
// truncation - and added as integers: the sums do not depend on the order, so the device, the twin and a NumPy loop agree on every element.
#pragma once

#include <stdint.h>

#include "../../include/lfd_densify.h"
#include "lfd_colour.hpp"

#define LFD_GAIN_QUANTITIES 7      // per row of the table: N, Sref[3], Snbr[3]

LFD_HD bool lfd_gain_in_range(float c) { return c >= 0.05f && c <= 0.95f; }

// c in [0.05, 0.95]: c * 2^24 is exact (a power of two), below 2^24, and the conversion truncates
LFD_HD uint32_t lfd_gain_quantise(float c) { return (uint32_t)(c * 16777216.0f); }

// Slot j < ns of a point that passed lfd_colour_guarded.  is_winner: j is the point's winning slot (it takes part unless its observation is
// not finite); otherwise lfd_support_candidate decides.  cert, (wx, wy): the slot's certainty and observation at the point's cell; ref_ok:
// the reference's three values lie in range.  Returns whether the sample counts; q[3] then holds the neighbour's quantised colour.
LFD_HD bool lfd_gain_sample(const LfdSlot& sl, const uint8_t* img, const LfdSupportGeom& g, bool is_winner, bool ref_ok, float cert, float wx,
                            float wy, float X0, float X1, float X2, uint32_t* q) {
    const bool part = is_winner ? (lfd_finite(wx) && lfd_finite(wy)) : lfd_support_candidate(sl, g, cert, wx, wy, X0, X1, X2);
    if (!part || !ref_ok) return false;
    float v[3];
    lfd_colour_sample(img, g, wx, wy, v);
    if (!(lfd_gain_in_range(v[0]) && lfd_gain_in_range(v[1]) && lfd_gain_in_range(v[2]))) return false;
    q[0] = lfd_gain_quantise(v[0]); q[1] = lfd_gain_quantise(v[1]); q[2] = lfd_gain_quantise(v[2]);
    return true;
}

// lfd_gain_apply: one colour value under factor f; one f32 rounding, a value that is not finite keeps its bits
LFD_HD float lfd_gain_value(float c, float f) {
    if (!lfd_finite(c)) return c;
    const float v = c * f;
    return v < 1.0f ? v : 1.0f;
}

// What an accumulate launch works on (device), by value in the kernel arguments.
struct LfdGainArgs {
    LfdPointStage st;                  // (g.reproj_thresh unused)
    const uint8_t* const* img;         // [n_refs * k] the neighbours' match-size images (device table)
    unsigned long long* table;         // [n_refs * k][7], added to
};

struct LfdGainApplyArgs {
    const long long* offs;             // [n_refs + 1]
    const float* factors;              // [n_refs][3]
    const float* rgb;                  // [3 * n]
    float* o_rgb;                      // [3 * n]; may be `rgb` itself
    long long n;
    int32_t n_refs;
};

static inline bool lfd_gain_overlap(const void* a, long long a_bytes, const void* b, long long b_bytes) {
    if (!a || !b) return false;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), a1 = a0 + (uintptr_t)a_bytes;
    const uintptr_t b0 = reinterpret_cast<uintptr_t>(b), b1 = b0 + (uintptr_t)b_bytes;
    return a0 < b1 && b0 < a1;
}

// Arguments of lfd_gain_accumulate[_host] that do not depend on the batch: lfd_colour_check's rules for the points, plus the table's; what is
// wrong with them, or null.  (The table's size depends on the batch: n_rows = n_refs * k of a batch that has been validated, or 0 before.)
inline const char* lfd_gain_check(const lfd_points* in, const int64_t* ref_offsets, const uint8_t* const* nbr_image, float support_thresh_px,
                                  const uint64_t* table, long long n_rows) {
    if (const char* why = lfd_colour_check(in, ref_offsets, nbr_image, support_thresh_px, LFD_COLOUR_MEAN, in ? in->rgb : nullptr, nullptr)) return why;
    if (!table) return "null table";
    const long long cap = in->capacity, bytes = n_rows * LFD_GAIN_QUANTITIES * 8;
    const struct { const void* p; long long elem; } a[5] = {{in->xyz, 12}, {in->rgb, 12}, {in->err, 4}, {in->cell, 4}, {in->slot, 1}};
    for (int i = 0; i < 5; ++i)
        if (lfd_gain_overlap(table, bytes > 0 ? bytes : 1, a[i].p, a[i].elem * cap)) return "table must overlap nothing of in";
    return nullptr;
}

inline const char* lfd_gain_apply_check(const float* rgb, int64_t n, const int64_t* ref_offsets, int32_t n_refs, const float* factors,
                                        const float* rgb_out) {
    if (!rgb || !rgb_out || !ref_offsets || !factors) return "null rgb / rgb_out / ref_offsets / factors";
    if (n < 0 || n > 0x7fffffffLL) return "n must be in [0, 2^31 - 1]";
    if (n_refs <= 0) return "n_refs must be > 0";
    if (rgb_out != rgb && lfd_gain_overlap(rgb, 12 * n, rgb_out, 12 * n)) return "rgb_out must be rgb itself or overlap nothing of it";
    if (lfd_gain_overlap(factors, 12LL * n_refs, rgb_out, 12 * n) || lfd_gain_overlap(ref_offsets, 8LL * (n_refs + 1), rgb_out, 12 * n))
        return "rgb_out must overlap neither factors nor ref_offsets";
    return nullptr;
}
