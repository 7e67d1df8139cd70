// Multi-view support filter (lfd_support_filter): the per-(point, slot) routine, compiled for the device (lfd_support.hip) and for
// the host (lfd_host.hip's twin).  A triangulated point is projected into every OTHER neighbour of its reference and compared with what that
// neighbour's warp says the cell maps to; it is kept iff at least min_support of them agree within support_thresh_px.
//
// Every rounding is written out (the build uses -ffp-contract=off) and nothing is divided, inverted or rooted: the twin and the kernels execute
// the same f32 multiplies, adds, subtracts and fmaf in the same order, so the support counts and the decisions agree bit for bit.
//
// LfdSlot, LfdSupportGeom and lfd_support_candidate - the candidate test - are also what the multi-view re-triangulation (lfd_refine.hpp,
// DESIGN 4.9) works with: the test exists once, so its candidates are this filter's set by construction.
#pragma once

#include <stdint.h>

#include "../../include/lfd_densify.h"
#include "lfd_geometry.hpp"

// live(j), first half: the raw certainty of the other neighbour at the point's cell (a NaN, and the exact 0 the cycle gate leaves, are not live)
LFD_HD bool lfd_support_live(float cert) { return cert > 0.0f; }

// live(j), second half: the pixel of mask_b the other neighbour's warp points at, looked up as cell_cert does (lfd_kernels.hip); -1: outside
LFD_HD long long lfd_support_mask_index(float xb, float yb, int W, int H, float mask_sx, float mask_sy, int w_match, int h_match) {
    const int ix = lfd_grid_nearest(xb, W), iy = lfd_grid_nearest(yb, H);
    if (ix < 0 || iy < 0) return -1;
    return (long long)lfd_nearest_src(iy, mask_sy, h_match) * w_match + lfd_nearest_src(ix, mask_sx, w_match);
}

// agree(j): Pi, sx, sy of LfdPairConst (interleaved projection rows, camera px per match px); (xb, yb) the neighbour's normalised observation.
// The observation is lfd_eval_correspondence's, the projection lfd_reproj_sq's chain; the comparison is cross-multiplied by the depth.
LFD_HD bool lfd_support_agree(const float* Pi, float sx, float sy, float X0, float X1, float X2, float xb, float yb, float wm1, float hm1, float tau) {
    const float ub = lfd_match_px(xb, wm1) * sx;
    const float vb = lfd_match_px(yb, hm1) * sy;
    const float px = lfd_proj_row(Pi, 0, X0, X1, X2, 1.0f);
    const float py = lfd_proj_row(Pi, 1, X0, X1, X2, 1.0f);
    const float pz = lfd_proj_row(Pi, 2, X0, X1, X2, 1.0f);
    const float mu = ub * pz, mv = vb * pz;
    const float du = px - mu, dv = py - mv;
    const float su = du * du, sv = dv * dv;
    const float d2 = su + sv;
    const float t = tau * pz;
    const float t2 = t * t;
    return pz > 0.0f && d2 <= t2;          // a NaN anywhere rejects
}

// reference of input point i: the last r in [0, n_refs) whose (clamped) offset is <= i.  offs: [n_refs + 1], offsets beyond `cap` count as `cap`
// (a producer that ran out of capacity reports the counts it would have needed).  Always a valid reference, whatever offs holds.
LFD_HD int lfd_support_ref_of(const long long* offs, int n_refs, long long cap, long long i) {
    int lo = 0, hi = n_refs;                // invariant: offs[lo] <= i (offs[0] is 0), answer in [lo, hi)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        long long o = offs[mid];
        o = o > cap ? cap : o;
        if (o <= i) lo = mid; else hi = mid;
    }
    return lo;
}

LFD_HD long long lfd_support_clamp(long long v, long long cap) { return v < 0 ? 0 : (v > cap ? cap : v); }

struct LfdSlot {                 // one neighbour of the reference at work (LDS on the device, a table on the host)
    const float* cert;
    const float* warp;
    const uint8_t* mask_b;
    float P[12];                 // interleaved (LfdPairConst)
    float sx, sy;
};

struct LfdSupportGeom {          // the grid and the thresholds of a launch (reproj_thresh: the re-triangulation's acceptance test only)
    int32_t H, W, C, w_match, h_match;
    float wm1, hm1, mask_sx, mask_sy, tau, reproj_thresh;
};

LFD_HD void lfd_slot_fill(LfdSlot& o, const float* cert, const float* warp, const uint8_t* mask_b, const LfdPairConst& c) {
    o.cert = cert; o.warp = warp; o.mask_b = mask_b;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int e = 0; e < 12; ++e) o.P[e] = c.P[e];
    o.sx = c.sx; o.sy = c.sy;
}

// The candidate test, the one copy the support filter and the re-triangulation share on both builds: neighbour `sl`, whose certainty and warp
// at the point's cell are cert and (wx, wy), is live (the mask is looked at only behind a live certainty) and agrees with X.
LFD_HD bool lfd_support_candidate(const LfdSlot& sl, const LfdSupportGeom& g, float cert, float wx, float wy, float X0, float X1, float X2) {
    bool live = lfd_support_live(cert);
    const uint8_t* mb = sl.mask_b;
    if (live && mb) {
        const long long m = lfd_support_mask_index(wx, wy, g.W, g.H, g.mask_sx, g.mask_sy, g.w_match, g.h_match);
        live = m >= 0 && mb[m] != 0;
    }
    const bool agree = lfd_support_agree(sl.P, sl.sx, sl.sy, X0, X1, X2, wx, wy, g.wm1, g.hm1, g.tau);
    return live && agree;
}

inline LfdSupportGeom lfd_support_geom(const lfd_batch* b, float wm1, float hm1, float mask_sx, float mask_sy, float tau, float reproj_thresh) {
    LfdSupportGeom g;
    g.H = b->H; g.W = b->W; g.C = b->warp_channels; g.w_match = b->w_match; g.h_match = b->h_match;
    g.wm1 = wm1; g.hm1 = hm1; g.mask_sx = mask_sx; g.mask_sy = mask_sy; g.tau = tau; g.reproj_thresh = reproj_thresh;
    return g;
}

// What every per-point stage behind triangulation hands its kernel (device): the first member of each stage's Lfd*Args, by value in the kernel
// arguments.  A stage reads what it needs of it; lfd_api.hip's fill_stage fills all of it.
struct LfdPointStage {
    const void* refs;                  // LfdRefDesc [n_refs]            (lfd_device.hpp; the twins read the lfd_batch itself)
    const void* slots;                 // LfdSlotDesc [n_refs * k]
    const LfdPairConst* pair_const;    // [n_refs * k]
    const long long* offs;             // [n_refs + 1]
    const float* xyz; const float* rgb; const float* err; const int32_t* cell; const uint8_t* slot;
    long long capacity;                // in->capacity
    int32_t n_refs, k, n_wg;           // n_wg: workgroups of 256 points that cover the capacity
    LfdSupportGeom g;
    const LfdRefConst* ref_const;      // [n_refs]          (what only some stages read comes last: with these three between the fields every
    const float* axis_x;               // [W], [H]: the A-grid axes (two-channel warps)    kernel reads, the support and photo kernels spill more)
    const float* axis_y;
};

// The compaction behind a per-point verdict (lfd_compact_launch, lfd_support.hip): the points whose keep byte is set move to the output in order.
struct LfdCompactArgs {
    const long long* offs_in;          // [n_refs + 1]
    long long* offs_out;               // [n_refs + 1]
    const float* xyz; const float* rgb; const float* err; const int32_t* cell; const uint8_t* slot;
    float* o_xyz; float* o_rgb; float* o_err; int32_t* o_cell; uint8_t* o_slot;
    const uint8_t* keep;               // workspace [n_wg * 256]: 1 where the point is kept, else 0
    unsigned* wg_kept;                 // workspace [n_wg + 1]: kept points per workgroup, then their exclusive prefix and the total
    const float* extra_in;             // [n_wg * 256] or null: one more f32 per point ...
    float* extra_out;                  // ... which moves with the points when this is set
    long long capacity;                // in->capacity
    int32_t n_refs, n_wg;
};

// What a launch of the support filter's own kernel works on (device), by value in the kernel arguments.
struct LfdSupportArgs {
    LfdPointStage st;
    int32_t* seg_counts;               // [n_refs * k] or null (zeroed before the launch)
    uint8_t* support;                  // [capacity] or null
    uint8_t* keep;                     // workspace [n_wg * 256]: 1 where support >= min_support
    unsigned* wg_kept;                 // workspace [n_wg + 1]: kept points per workgroup
    int32_t min_support;
};

// Arguments of lfd_support_filter / lfd_support_filter_host that do not depend on the batch; what is wrong with them (and the status), or null.
inline const char* lfd_support_check(const lfd_points* in, const int64_t* ref_offsets_in, int32_t min_support, float support_thresh_px,
                                     const lfd_points* out, const int64_t* ref_offsets_out, int* code) {
    *code = LFD_ERR_INVALID;
    if (!in || !out || !ref_offsets_in || !ref_offsets_out) return "null in / out / ref_offsets";
    if (!in->xyz || !in->rgb || !in->err || !out->xyz || !out->rgb || !out->err) return "null point arrays";
    if (!in->cell || !in->slot) return "in->cell and in->slot are required";
    if (in->capacity < 0 || out->capacity < 0 || in->capacity > 0x7fffffffLL) return "capacity must be in [0, 2^31 - 1]";
    if (min_support < 1 || min_support > LFD_MAX_SLOTS - 1) return "min_support must be in [1, LFD_MAX_SLOTS - 1]";
    if (!(support_thresh_px > 0.0f) || !(support_thresh_px <= 3.4028234e38f)) return "support_thresh_px must be finite and > 0";
    const struct { const void* p; long long elem; } a[5] = {{in->xyz, 12}, {in->rgb, 12}, {in->err, 4}, {in->cell, 4}, {in->slot, 1}},
                                                    b[5] = {{out->xyz, 12}, {out->rgb, 12}, {out->err, 4}, {out->cell, 4}, {out->slot, 1}};
    for (int i = 0; i < 5; ++i)
        for (int j = 0; j < 5; ++j) {
            if (!a[i].p || !b[j].p) continue;
            const uintptr_t a0 = reinterpret_cast<uintptr_t>(a[i].p), a1 = a0 + (uintptr_t)(a[i].elem * in->capacity);
            const uintptr_t b0 = reinterpret_cast<uintptr_t>(b[j].p), b1 = b0 + (uintptr_t)(b[j].elem * out->capacity);
            if (a0 < b1 && b0 < a1) return "in and out overlap";
        }
    if (out->capacity < in->capacity) { *code = LFD_ERR_CAPACITY; return "out->capacity must be >= in->capacity"; }
    return nullptr;
}
