// Far-field shell (lfd_far_accumulate / lfd_far_emit): the per-cell and per-direction-cell routines, compiled for the device
// (lfd_far.hip) and for the host (lfd_host.hip's twins).  A grid cell of a reference is FAR when every neighbour that matched it confidently
// sees it where the rotation-only transfer predicts - the point at infinity (d, 0) of the cell's ray projected into the neighbour.  Far cells
// are summed, as exact integers, into a cube-map table of direction cells; lfd_far_emit turns the occupied cells into shell points.
//
// The decision is f32 with every rounding written out (the build uses -ffp-contract=off) and nothing divided; the direction cell, the unit
// direction and the emitted records are f64 with IEEE division and square root on both builds.  All sums are integers: device, twin and a
// NumPy loop agree on every element of the table whatever the order.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/lfd_densify.h"
#include "lfd_support.hpp"

#define LFD_FAR_QUANTITIES 7       // per direction cell: sum of rint(d_hat 2^30) [3] (i64, two's complement), sum of the u8 colour [3], count
#define LFD_FAR_MIN_CELLS 8
#define LFD_FAR_MAX_CELLS 512
#define LFD_FAR_MAX_VIEWS 8

// The reference camera's back-projection, f32: M = R^T K^-1 (3 x 3, row-major), so that d = M (u, v, 1) is the world direction of camera
// pixel (u, v).  K^-1 is lfd_inv3_intrinsics' (what the fundamental matrix uses); each entry is a forward fused chain.
LFD_HD void lfd_far_dir_matrix(const LfdCam& c, float* M) {
    float Ki[9];
    lfd_inv3_intrinsics(c.K, Ki);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) M[3 * i + j] = lfd_dot3_chain(c.R[i], Ki[j], c.R[3 + i], Ki[3 + j], c.R[6 + i], Ki[6 + j]);
}

// d = M (xa_px sx, ya_px sy, 1): (xan, yan) the cell's normalised A-coordinate, sx / sy the reference's camera px per match px
LFD_HD void lfd_far_direction(const float* M, float sx, float sy, float xan, float yan, float wm1, float hm1, float* d) {
    const float ua = lfd_match_px(xan, wm1) * sx;
    const float va = lfd_match_px(yan, hm1) * sy;
    for (int i = 0; i < 3; ++i) d[i] = fmaf(M[3 * i + 1], va, fmaf(M[3 * i], ua, M[3 * i + 2]));
}

// lfd_support_agree's chain with the homogeneous coordinate 0 instead of 1: the point at infinity of the ray against the neighbour's observation
LFD_HD bool lfd_far_agree(const float* Pi, float sx, float sy, float d0, float d1, float d2, float xb, float yb, float wm1, float hm1, float tau) {
    const float ub = lfd_match_px(xb, wm1) * sx;
    const float vb = lfd_match_px(yb, hm1) * sy;
    const float px = lfd_proj_row(Pi, 0, d0, d1, d2, 0.0f);
    const float py = lfd_proj_row(Pi, 1, d0, d1, d2, 0.0f);
    const float pz = lfd_proj_row(Pi, 2, d0, d1, d2, 0.0f);
    const float mu = ub * pz, mv = vb * pz;
    const float du = px - mu, dv = py - mv;
    const float su = du * du, sv = dv * dv;
    const float d2s = su + sv;
    const float t = tau * pz;
    const float t2 = t * t;
    return pz > 0.0f && d2s <= t2;         // a NaN anywhere rejects
}

// Slot `sl` at a cell whose raw certainty and observation are cert and (wx, wy) is CONFIDENT: bit 0 of lfd_far_slot, and what the epipolar
// audit (lfd_audit.hpp) counts
LFD_HD bool lfd_far_confident(const LfdSlot& sl, const LfdSupportGeom& g, float far_certainty, float cert, float wx, float wy) {
    bool conf = cert >= far_certainty;     // a NaN is not confident
    if (conf) {
        const long long m = lfd_support_mask_index(wx, wy, g.W, g.H, g.mask_sx, g.mask_sy, g.w_match, g.h_match);   // -1: outside the neighbour
        conf = m >= 0 && (!sl.mask_b || sl.mask_b[m] != 0);
    }
    return conf;
}

// ... confident (bit 0), confident and agreeing with infinity (bit 1)
LFD_HD int lfd_far_slot(const LfdSlot& sl, const LfdSupportGeom& g, float far_certainty, float cert, float wx, float wy, float d0, float d1,
                        float d2) {
    if (!lfd_far_confident(sl, g, far_certainty, cert, wx, wy)) return 0;
    return lfd_far_agree(sl.P, sl.sx, sl.sy, d0, d1, d2, wx, wy, g.wm1, g.hm1, g.tau) ? 3 : 1;
}

LFD_HD bool lfd_far_verdict(int n_conf, int n_agree, int min_views, int ns) {
    return n_conf >= (min_views < ns ? min_views : ns) && n_agree == n_conf;      // one confident neighbour that sees parallax vetoes the cell
}

// The direction cell of d and rint(d_hat 2^30), f64 only; false for a zero or non-finite d (nothing is converted to an integer then).
// Cube map: face = 2 m + (d_m < 0), m the index of the largest |d_i| (lowest on ties); the other two components, ascending, over |d_m|.
LFD_HD bool lfd_far_key(float d0, float d1, float d2, int S, long long* key, long long* q) {
    if (!(lfd_finite(d0) && lfd_finite(d1) && lfd_finite(d2))) return false;
    const double d[3] = {(double)d0, (double)d1, (double)d2};
    const double a[3] = {fabs(d[0]), fabs(d[1]), fabs(d[2])};
    int m = 0;
    if (a[1] > a[m]) m = 1;
    if (a[2] > a[m]) m = 2;
    if (!(a[m] > 0.0)) return false;
    const int ia = m == 0 ? 1 : 0, ib = m == 2 ? 1 : 2;
    const double u = d[ia] / a[m], v = d[ib] / a[m];
    const double fu = floor(((u + 1.0) * 0.5) * (double)S), fv = floor(((v + 1.0) * 0.5) * (double)S);
    int iu = (int)fu, iv = (int)fv;                                    // in [0, S]: |u|, |v| <= 1
    iu = iu < 0 ? 0 : (iu > S - 1 ? S - 1 : iu);
    iv = iv < 0 ? 0 : (iv > S - 1 ? S - 1 : iv);
    const int face = 2 * m + (d[m] < 0.0 ? 1 : 0);
    *key = ((long long)face * S + iv) * S + iu;
    const double n2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];       // the products are exact (f32 factors)
    const double n = sqrt(n2);
    for (int i = 0; i < 3; ++i) q[i] = (long long)rint((d[i] / n) * 1073741824.0);
    return true;
}

// One direction cell of the table -> one shell record; false: not emitted.  row: the cell's seven sums.
LFD_HD bool lfd_far_kept(const uint64_t* row, long long min_samples) {
    return (long long)row[6] >= min_samples && ((row[0] | row[1] | row[2]) != 0);
}

LFD_HD void lfd_far_record(const uint64_t* row, const double* centre, double radius, float* xyz, float* rgb, float* normal, int32_t* samples) {
    const double s[3] = {(double)(long long)row[0], (double)(long long)row[1], (double)(long long)row[2]};
    const double n = sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
    const double cnt = (double)row[6];
    for (int i = 0; i < 3; ++i) {
        const double h = s[i] / n;
        xyz[i] = (float)(centre[i] + radius * h);
        if (normal) normal[i] = (float)(-h);
        rgb[i] = (float)((double)row[3 + i] / (255.0 * cnt));
    }
    if (samples) *samples = row[6] > 0x7fffffffull ? 0x7fffffff : (int32_t)row[6];
}

// What an accumulate launch works on (device), by value in the kernel arguments.
struct LfdFarArgs {
    const LfdCam* cams;
    const void* refs;                  // LfdRefDesc [n_refs]
    const void* slots;                 // LfdSlotDesc [n_refs * k]
    const LfdRefConst* ref_const;      // [n_refs]
    const LfdPairConst* pair_const;    // [n_refs * k]
    const float* axis_x; const float* axis_y;
    unsigned long long* table;         // [6 S S][7], added to
    unsigned long long* counters;      // [n_refs] or null, added to
    uint8_t* flags;                    // [n_refs * H * W] or null: 1 for a far cell, 0 otherwise (written, not added to)
    int32_t n_refs, k, S, min_views;
    float far_certainty;
    LfdSupportGeom g;                  // (tau: far_thresh_px; reproj_thresh unused)
};

struct LfdFarEmitArgs {
    const unsigned long long* table;
    const uint8_t* keep;
    const unsigned* wg_kept;
    double centre[3], radius;
    float* xyz; float* rgb; float* normal; int32_t* samples;
    long long n_cells, capacity, min_samples;
};

static inline bool lfd_far_overlap(const void* a, long long a_bytes, const void* b, long long b_bytes) {
    if (!a || !b) return false;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), a1 = a0 + (uintptr_t)a_bytes;
    const uintptr_t b0 = reinterpret_cast<uintptr_t>(b), b1 = b0 + (uintptr_t)b_bytes;
    return a0 < b1 && b0 < a1;
}

static inline long long lfd_far_table_bytes(int32_t S) { return 6LL * S * S * LFD_FAR_QUANTITIES * 8; }

// Arguments of lfd_far_accumulate[_host] that do not depend on the batch; what is wrong with them, or null.
inline const char* lfd_far_check(float far_thresh_px, float far_certainty, int32_t far_min_views, int32_t shell_cells, const uint64_t* table) {
    if (!table) return "null table";
    if (!(far_thresh_px > 0.0f) || !(far_thresh_px <= 3.4028234e38f)) return "far_thresh_px must be finite and > 0";
    if (!(far_certainty > 0.0f) || !(far_certainty <= 3.4028234e38f)) return "far_certainty must be finite and > 0";
    if (far_min_views < 1 || far_min_views > LFD_FAR_MAX_VIEWS) return "far_min_views must be in [1, 8]";
    if (shell_cells < LFD_FAR_MIN_CELLS || shell_cells > LFD_FAR_MAX_CELLS) return "shell_cells must be in [8, 512]";
    return nullptr;
}

// ... and those that do: the table (and the counters) must overlap none of the planes of a batch that has been validated
inline const char* lfd_far_check_batch(const lfd_batch* b, int32_t shell_cells, const uint64_t* table, const int64_t* counters,
                                       const uint8_t* flags) {
    const long long tb = lfd_far_table_bytes(shell_cells), cb = counters ? 8LL * b->n_refs : 0, HW = (long long)b->H * b->W;
    const long long img = 3LL * b->w_match * b->h_match, msk = (long long)b->w_match * b->h_match, fb = flags ? HW * b->n_refs : 0;
    if (lfd_far_overlap(table, tb, counters, cb)) return "table and counters overlap";
    if (lfd_far_overlap(table, tb, flags, fb) || lfd_far_overlap(counters, cb, flags, fb)) return "flags overlap the table or the counters";
    for (int r = 0; r < b->n_refs; ++r) {
        const void* own[2] = {b->image[r], b->mask_a ? b->mask_a[r] : nullptr};
        const long long own_b[2] = {img, msk};
        for (int e = 0; e < 2; ++e)
            if (lfd_far_overlap(table, tb, own[e], own_b[e]) || lfd_far_overlap(counters, cb, own[e], own_b[e]) ||
                lfd_far_overlap(flags, fb, own[e], own_b[e]))
                return "table / counters / flags must overlap nothing of the batch";
        for (int j = 0; j < b->n_slots[r]; ++j) {
            const size_t s = (size_t)r * b->k + j;
            const void* pl[3] = {b->cert[s], b->warp[s], b->mask_b ? b->mask_b[s] : nullptr};
            const long long pl_b[3] = {4 * HW, 4 * HW * b->warp_channels, msk};
            for (int e = 0; e < 3; ++e)
                if (lfd_far_overlap(table, tb, pl[e], pl_b[e]) || lfd_far_overlap(counters, cb, pl[e], pl_b[e]) ||
                    lfd_far_overlap(flags, fb, pl[e], pl_b[e]))
                    return "table / counters / flags must overlap nothing of the batch";
        }
    }
    return nullptr;
}

inline const char* lfd_far_emit_check(const uint64_t* table, int32_t shell_cells, int64_t min_samples, const double* centre, double radius,
                                      const float* xyz, const float* rgb, const float* normal, const int32_t* samples, int64_t capacity,
                                      const int64_t* n_out) {
    if (!table || !centre || !xyz || !rgb || !n_out) return "null table / centre / xyz / rgb / n_out";
    if (shell_cells < LFD_FAR_MIN_CELLS || shell_cells > LFD_FAR_MAX_CELLS) return "shell_cells must be in [8, 512]";
    if (min_samples < 1) return "min_samples must be >= 1";
    if (!(fabs(centre[0]) <= 1.7976931348623157e308 && fabs(centre[1]) <= 1.7976931348623157e308 && fabs(centre[2]) <= 1.7976931348623157e308))
        return "centre must be finite";
    if (!(radius > 0.0) || !(radius <= 1.7976931348623157e308)) return "radius must be finite and > 0";
    if (capacity < 0 || capacity > 0x7fffffffLL) return "capacity must be in [0, 2^31 - 1]";
    const long long tb = lfd_far_table_bytes(shell_cells);
    const struct { const void* p; long long bytes; } o[4] = {{xyz, 12 * capacity}, {rgb, 12 * capacity}, {normal, 12 * capacity}, {samples, 4 * capacity}};
    for (int i = 0; i < 4; ++i) {
        if (lfd_far_overlap(table, tb, o[i].p, o[i].bytes)) return "the outputs must not overlap the table";
        for (int j = i + 1; j < 4; ++j)
            if (lfd_far_overlap(o[i].p, o[i].bytes, o[j].p, o[j].bytes)) return "the outputs overlap each other";
    }
    return nullptr;
}
