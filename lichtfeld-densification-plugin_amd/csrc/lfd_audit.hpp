// Epipolar audit (lfd_epipolar_audit): the per-(cell, slot) routine, compiled for the device (lfd_audit.hip) and for the host
// (lfd_host.hip's twin).  Every confident match of a (reference, neighbour) pair is measured against the pair's epipolar geometry as the poses
// give it: the distance of the neighbour's observation from the line F (ua, va, 1), in px of the neighbour's camera image, sorted into one of
// 64 bins of an eighth of a pixel.  The histograms are summed per pair as exact integers; core/audit.py turns them into a report on the poses.
//
// The coordinates are f32 as the dense kernel forms them; the line and the distance are f64 with every product and sum rounded separately (the
// build uses -ffp-contract=off); the bin is decided without division or root: device, twin and a NumPy evaluation agree on every integer.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/lfd_densify.h"
#include "lfd_far.hpp"

#define LFD_AUDIT_BINS 64
#define LFD_AUDIT_QUANTITIES 66    // per (reference, slot): usable samples, degenerate samples, the 64 bins
#define LFD_AUDIT_NONE 255         // cell map: no usable confident slot, or mask_a unset

LFD_HD bool lfd_audit_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }   // false for NaN / Inf

// The bin of one confident match, or -1 for a degenerate sample.  F: LfdPairConst::F (f32 values, so F_i * ua is exact); (rsx, rsy) and
// (ssx, ssy) the camera px per match px of the reference and of the neighbour; (xan, yan) / (xb, yb) the normalised coordinates in A and B.
LFD_HD int lfd_audit_bin(const double* F, float rsx, float rsy, float ssx, float ssy, float xan, float yan, float xb, float yb, float wm1,
                         float hm1) {
    const double ua = (double)(lfd_match_px(xan, wm1) * rsx), va = (double)(lfd_match_px(yan, hm1) * rsy);
    const double ub = (double)(lfd_match_px(xb, wm1) * ssx), vb = (double)(lfd_match_px(yb, hm1) * ssy);
    const double l0 = (F[0] * ua + F[1] * va) + F[2];
    const double l1 = (F[3] * ua + F[4] * va) + F[5];
    const double l2 = (F[6] * ua + F[7] * va) + F[8];
    const double num = (ub * l0 + vb * l1) + l2;
    const double n2 = l0 * l0 + l1 * l1;
    const double num2 = num * num;
    if (!(lfd_audit_finite(num2) && lfd_audit_finite(n2) && n2 > 0.0)) return -1;
    // the number of b in 0 .. 62 with num2 >= RN(e2[b] n2), e2[b] = (b + 1)^2 / 64 (exact): rounding is monotone, so the predicate is monotone
    // in b and six steps of a binary search give the count
    int bin = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int step = 32; step >= 1; step >>= 1) {
        const int t = bin + step;                                      // <= 63
        const double e2 = (double)(t * t) * 0.015625;
        const double bound = e2 * n2;
        if (num2 >= bound) bin = t;
    }
    return bin;
}

// What a launch works on (device), by value in the kernel arguments.
struct LfdAuditArgs {
    const void* refs;                  // LfdRefDesc [n_refs]
    const void* slots;                 // LfdSlotDesc [n_refs * k]
    const LfdRefConst* ref_const;      // [n_refs]
    const LfdPairConst* pair_const;    // [n_refs * k]
    const float* axis_x; const float* axis_y;
    unsigned long long* table;         // [n_refs * k][66], added to
    uint8_t* best;                     // [n_refs * H * W] or null, written
    int32_t n_refs, k;
    float audit_certainty;
    LfdSupportGeom g;                  // (tau and reproj_thresh unused)
};

static inline long long lfd_audit_table_bytes(const lfd_batch* b) { return (long long)b->n_refs * b->k * LFD_AUDIT_QUANTITIES * 8; }

// Arguments of lfd_epipolar_audit[_host] that do not depend on the batch; what is wrong with them, or null.
inline const char* lfd_audit_check(float audit_certainty, const uint64_t* table) {
    if (!table) return "null table";
    if (!(audit_certainty > 0.0f) || !(audit_certainty <= 3.4028234e38f)) return "audit_certainty must be finite and > 0";
    return nullptr;
}

// ... and those that do: the table and the cell map must overlap none of the planes of a batch that has been validated, nor each other
inline const char* lfd_audit_check_batch(const lfd_batch* b, const uint64_t* table, const uint8_t* best) {
    if (b->n_refs > 65535) return "at most 65535 references per batch";
    const long long tb = lfd_audit_table_bytes(b), HW = (long long)b->H * b->W, bb = best ? HW * b->n_refs : 0;
    const long long img = 3LL * b->w_match * b->h_match, msk = (long long)b->w_match * b->h_match;
    if (lfd_far_overlap(table, tb, best, bb)) return "table and best overlap";
    for (int r = 0; r < b->n_refs; ++r) {
        const void* own[2] = {b->image[r], b->mask_a ? b->mask_a[r] : nullptr};
        const long long own_b[2] = {img, msk};
        for (int e = 0; e < 2; ++e)
            if (lfd_far_overlap(table, tb, own[e], own_b[e]) || lfd_far_overlap(best, bb, own[e], own_b[e]))
                return "table / best must overlap nothing of the batch";
        for (int j = 0; j < b->n_slots[r]; ++j) {
            const size_t s = (size_t)r * b->k + j;
            const void* pl[3] = {b->cert[s], b->warp[s], b->mask_b ? b->mask_b[s] : nullptr};
            const long long pl_b[3] = {4 * HW, 4 * HW * b->warp_channels, msk};
            for (int e = 0; e < 3; ++e)
                if (lfd_far_overlap(table, tb, pl[e], pl_b[e]) || lfd_far_overlap(best, bb, pl[e], pl_b[e]))
                    return "table / best must overlap nothing of the batch";
        }
    }
    return nullptr;
}
