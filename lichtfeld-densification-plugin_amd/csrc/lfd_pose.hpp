// Pose corrections from the matches (lfd_pose_accumulate): the per-pair constants and the per-(cell, slot) routine, compiled for the
// device (lfd_pose.hip) and for the host (lfd_host.hip's twin).  Every confident match of a (reference A, neighbour B) pair contributes one row
// of the Gauss-Newton normal equations of the epipolar error with respect to the pair's RELATIVE pose: the signed distance r of B's observation
// from its epipolar line, in px of B's camera image, and its derivative J with respect to a left twist (omega, tau) of the relative pose
// T = T_B T_A^-1 -> exp(omega, tau) T, taken at the FOOT of the observation on the line (at the noisy observation itself the step is biased:
// errors in variables).  The sums are quantised integers, so device, twin and a NumPy evaluation agree on every element whatever the order;
// core/poses.py expands them to the two cameras' twists, projects the gauge out and solves.
//
// The pair's geometry comes from the uploaded camera table (f32 values, every operation in f64 and written out, lfd_pose_make_const);
// batch->fundamental is NOT used: a caller's F says nothing about R and t.  The build uses -ffp-contract=off; division and root are IEEE.
//
// Overflow: a sample is summed only with |J_i| < 2^16, so |Jq_i| = |rint(8 J_i)| <= 2^19, and with num^2 < c^2 d2, c = pose_inlier_px <= 64,
// so |rq| = |rint(1024 r)| <= 2^16; a product is at most 2^38, and a launch adds at most H W <= 2^24 samples to a row (the call refuses
// more): a column grows by at most 2^62 per launch.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/lfd_densify.h"
#include "lfd_far.hpp"

#define LFD_POSE_QUANTITIES 32     // per (reference, slot): inliers, outliers, degenerate, rq rq, Jq_i rq [6], Jq_i Jq_j (i <= j, row-major) [21], unused
#define LFD_POSE_SUMS 28           // columns 3 .. 30: the signed sums
#define LFD_POSE_MAX_CELLS (1LL << 24)
#define LFD_POSE_INLIER 0
#define LFD_POSE_OUTLIER 1
#define LFD_POSE_DEGENERATE 2

// What a pair needs, 32 doubles (LDS on the device): K_A^-1, R = R_B R_A^T, th = t / |t| of t = t_B - R t_A, K_B^-1, tn = |t|, ok (1 / 0).
struct LfdPoseConst {
    double KAi[9], R[9], th[3], KBi[9], tn, ok;
};

LFD_HD bool lfd_pose_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }   // false for NaN / Inf

// Host only (lfd_api.hip per launch, lfd_host.hip).  The inverses are lfd_inv3_intrinsics' f32 values, what the library's own F uses.
inline void lfd_pose_make_const(const LfdCam& a, const LfdCam& b, LfdPoseConst& o) {
    float KAi[9], KBi[9];
    lfd_inv3_intrinsics(a.K, KAi);
    lfd_inv3_intrinsics(b.K, KBi);
    for (int i = 0; i < 9; ++i) { o.KAi[i] = (double)KAi[i]; o.KBi[i] = (double)KBi[i]; }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            o.R[3 * i + j] = ((double)b.R[3 * i] * (double)a.R[3 * j] + (double)b.R[3 * i + 1] * (double)a.R[3 * j + 1]) +
                             (double)b.R[3 * i + 2] * (double)a.R[3 * j + 2];
    double t[3];
    for (int i = 0; i < 3; ++i) {
        const double rt = (o.R[3 * i] * (double)a.t[0] + o.R[3 * i + 1] * (double)a.t[1]) + o.R[3 * i + 2] * (double)a.t[2];
        t[i] = (double)b.t[i] - rt;
    }
    const double tn = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
    const bool ok = lfd_pose_finite(tn) && tn > 0.0;                   // coincident centres (or a non-finite pose): every sample is degenerate
    o.tn = ok ? tn : 0.0;
    o.ok = ok ? 1.0 : 0.0;
    for (int i = 0; i < 3; ++i) o.th[i] = ok ? t[i] / tn : 0.0;
}

// One confident match.  pc: the pair's LfdPoseConst; (rsx, rsy) / (ssx, ssy) the camera px per match px of A and of B; (xan, yan) / (xb, yb)
// the normalised coordinates in A and B (formed into camera px as lfd_audit_bin forms them); c2 = (double)pose_inlier_px squared.  Returns
// the sample's class; for an inlier q[0 .. 5] = Jq, q[6] = rq, else q is all zero.
LFD_HD int lfd_pose_sample(const LfdPoseConst& pc, float rsx, float rsy, float ssx, float ssy, float xan, float yan, float xb, float yb, float wm1,
                           float hm1, double c2, int32_t* q) {
    for (int i = 0; i < 7; ++i) q[i] = 0;
    const double ua = (double)(lfd_match_px(xan, wm1) * rsx), va = (double)(lfd_match_px(yan, hm1) * rsy);
    const double ub = (double)(lfd_match_px(xb, wm1) * ssx), vb = (double)(lfd_match_px(yb, hm1) * ssy);
    double yA[3], p[3], l[3];
    for (int i = 0; i < 3; ++i) yA[i] = (pc.KAi[3 * i] * ua + pc.KAi[3 * i + 1] * va) + pc.KAi[3 * i + 2];
    for (int i = 0; i < 3; ++i) p[i] = (pc.R[3 * i] * yA[0] + pc.R[3 * i + 1] * yA[1]) + pc.R[3 * i + 2] * yA[2];
    const double n[3] = {pc.th[1] * p[2] - pc.th[2] * p[1], pc.th[2] * p[0] - pc.th[0] * p[2], pc.th[0] * p[1] - pc.th[1] * p[0]};
    for (int i = 0; i < 3; ++i) l[i] = (pc.KBi[i] * n[0] + pc.KBi[3 + i] * n[1]) + pc.KBi[6 + i] * n[2];      // K_B^-T n
    const double num = (ub * l[0] + vb * l[1]) + l[2];
    const double d2 = l[0] * l[0] + l[1] * l[1];
    const double num2 = num * num;
    if (!(pc.ok != 0.0 && lfd_pose_finite(num) && lfd_pose_finite(d2) && lfd_pose_finite(num2) && d2 > 0.0)) return LFD_POSE_DEGENERATE;
    const double d = sqrt(d2);
    const double r = num / d;
    const double s0 = (r * l[0]) / d, s1 = (r * l[1]) / d;
    const double uf = ub - s0, vf = vb - s1;                           // the foot of the observation on the line
    double yB[3];
    for (int i = 0; i < 3; ++i) yB[i] = (pc.KBi[3 * i] * uf + pc.KBi[3 * i + 1] * vf) + pc.KBi[3 * i + 2];
    const double J[6] = {(n[1] * yB[2] - n[2] * yB[1]) / d, (n[2] * yB[0] - n[0] * yB[2]) / d, (n[0] * yB[1] - n[1] * yB[0]) / d,
                         (p[1] * yB[2] - p[2] * yB[1]) / d, (p[2] * yB[0] - p[0] * yB[2]) / d, (p[0] * yB[1] - p[1] * yB[0]) / d};
    bool fine = lfd_pose_finite(r) && lfd_pose_finite(uf) && lfd_pose_finite(vf);
    for (int i = 0; i < 6; ++i) fine = fine && fabs(J[i]) < 65536.0;   // (false for a NaN or an infinity)
    if (!fine) return LFD_POSE_DEGENERATE;
    const double bound = c2 * d2;
    if (num2 >= bound) return LFD_POSE_OUTLIER;                        // |r| >= pose_inlier_px, decided without the division
    for (int i = 0; i < 6; ++i) q[i] = (int32_t)rint(8.0 * J[i]);
    q[6] = (int32_t)rint(1024.0 * r);
    return LFD_POSE_INLIER;
}

// The 28 signed sums of one inlier, in the table's column order from column 3: rq rq, Jq_i rq, Jq_i Jq_j (i <= j)
LFD_HD long long lfd_pose_term(const int32_t* q, int e) {
    if (e == 0) return (long long)q[6] * q[6];
    if (e < 7) return (long long)q[e - 1] * q[6];
    int i = 0, f = e - 7;                                              // row-major upper triangle of 6 x 6
    while (f >= 6 - i) { f -= 6 - i; ++i; }
    return (long long)q[i] * q[i + f];
}

// What a launch works on (device), by value in the kernel arguments.
struct LfdPoseArgs {
    const void* refs;                  // LfdRefDesc [n_refs]
    const void* slots;                 // LfdSlotDesc [n_refs * k]
    const LfdRefConst* ref_const;      // [n_refs]
    const LfdPairConst* pair_const;    // [n_refs * k]
    const LfdPoseConst* pose_const;    // [n_refs * k]
    const float* axis_x; const float* axis_y;
    unsigned long long* table;         // [n_refs * k][32], added to (two's complement)
    int32_t n_refs, k;
    float pose_certainty;
    double c2;                         // pose_inlier_px squared
    LfdSupportGeom g;                  // (tau and reproj_thresh unused)
};

static inline long long lfd_pose_table_bytes(const lfd_batch* b) { return (long long)b->n_refs * b->k * LFD_POSE_QUANTITIES * 8; }

// Arguments of lfd_pose_accumulate[_host] that do not depend on the batch; what is wrong with them, or null.
inline const char* lfd_pose_check(float pose_certainty, float pose_inlier_px, const int64_t* table) {
    if (!table) return "null table";
    if (!(pose_certainty > 0.0f) || !(pose_certainty <= 3.4028234e38f)) return "pose_certainty must be finite and > 0";
    if (!(pose_inlier_px > 0.0f) || !(pose_inlier_px <= 64.0f)) return "pose_inlier_px must be in (0, 64]";
    return nullptr;
}

// ... and those that do: the table must overlap none of the planes of a batch that has been validated
inline const char* lfd_pose_check_batch(const lfd_batch* b, const int64_t* table) {
    if (b->n_refs > 65535) return "at most 65535 references per batch";
    const long long tb = lfd_pose_table_bytes(b), HW = (long long)b->H * b->W;
    if (HW > LFD_POSE_MAX_CELLS) return "at most 2^24 grid cells per reference (the sums' overflow bound)";
    const long long img = 3LL * b->w_match * b->h_match, msk = (long long)b->w_match * b->h_match;
    for (int r = 0; r < b->n_refs; ++r) {
        const void* own[2] = {b->image[r], b->mask_a ? b->mask_a[r] : nullptr};
        const long long own_b[2] = {img, msk};
        for (int e = 0; e < 2; ++e)
            if (lfd_far_overlap(table, tb, own[e], own_b[e])) return "the table must overlap nothing of the batch";
        for (int j = 0; j < b->n_slots[r]; ++j) {
            const size_t s = (size_t)r * b->k + j;
            const void* pl[3] = {b->cert[s], b->warp[s], b->mask_b ? b->mask_b[s] : nullptr};
            const long long pl_b[3] = {4 * HW, 4 * HW * b->warp_channels, msk};
            for (int e = 0; e < 3; ++e)
                if (lfd_far_overlap(table, tb, pl[e], pl_b[e])) return "the table must overlap nothing of the batch";
        }
    }
    return nullptr;
}
