// Depth-uncertainty gate on triangulated points (lfd_depth_sigma_filter): the per-point routine, compiled for the device
// (lfd_sigma.hip) and for the host (lfd_host.hip's twin).  The point X of a reference with centre C is moved along the reference's ray,
// X(l) = C + l D, D = X - C; every view that took part in placing it sees its projection move by g = d proj / d l (camera px per unit l) and
// contributes the Fisher information I = g^T P g of l, P the view's 2x2 match precision in camera px^-2.  sigma_rel = 1 / sqrt(sum I) is the
// Cramer-Rao bound on the relative depth error.
//
// Every rounding is written out (the build uses -ffp-contract=off).  Everything runs in f64 from the f32 inputs - g is a difference of nearly
// equal terms -, one fma chain per quantity, the views in a fixed order (winning slot, then candidates by ascending slot); the result is rounded
// to f32 once.  The two builds differ only where lfd_geometry.hpp's do: lfd_recip_refined (IEEE division / Newton-refined v_rcp_f64) and
// lfd_sqrt_rare.  The candidate set is lfd_support_candidate's (lfd_support.hpp), the precision scales and the validity test are
// lfd_refine.hpp's: called, not copied.
#pragma once

#include <stdint.h>

#include "../../include/lfd_densify.h"
#include "lfd_geometry.hpp"
#include "lfd_support.hpp"
#include "lfd_refine.hpp"

#define LFD_SIGMA_INF (__builtin_huge_valf())

struct LfdSigmaRef {             // the reference itself: its centre (LfdRefConst::C)
    float C[3];
};

// Information of one view about l.  Pi: the view's interleaved projection rows; (x0, x1, x2): the point; (d0, d1, d2): D; (p00, p01, p11): the
// view's precision, camera px^-2.  A view the point lies behind (pz <= 0, or a NaN) or whose contribution is not finite adds nothing.
LFD_HD void lfd_sigma_add_view(double& sum, const float* Pi, double x0, double x1, double x2, double d0, double d1, double d2, double p00,
                               double p01, double p11) {
    const double px = fma(x2, (double)Pi[4], fma(x1, (double)Pi[2], fma(x0, (double)Pi[0], (double)Pi[6])));
    const double py = fma(x2, (double)Pi[5], fma(x1, (double)Pi[3], fma(x0, (double)Pi[1], (double)Pi[7])));
    const double pz = fma(x2, (double)Pi[10], fma(x1, (double)Pi[9], fma(x0, (double)Pi[8], (double)Pi[11])));
    const double hx = fma(d2, (double)Pi[4], fma(d1, (double)Pi[2], d0 * (double)Pi[0]));
    const double hy = fma(d2, (double)Pi[5], fma(d1, (double)Pi[3], d0 * (double)Pi[1]));
    const double hz = fma(d2, (double)Pi[10], fma(d1, (double)Pi[9], d0 * (double)Pi[8]));
    const double rz = lfd_recip_refined(pz);
    const double u = px * rz, v = py * rz;                  // the projection
    const double gx = fma(-u, hz, hx) * rz;                 // hx / pz - px hz / pz^2
    const double gy = fma(-v, hz, hy) * rz;
    const double tu = fma(p01, gy, p00 * gx);
    const double tv = fma(p11, gy, p01 * gx);
    const double I = fma(gy, tv, gx * tu);
    const bool ok = pz > 0.0 && fabs(I) <= 1.7976931348623157e308;      // (a NaN fails both)
    sum = ok ? sum + I : sum;
}

// sum of the views' information -> sigma_rel (f32); +inf where the sum is not finite or not positive.
LFD_HD float lfd_sigma_finish(double sum) {
    if (!(sum > 0.0) || !(sum <= 1.7976931348623157e308)) return LFD_SIGMA_INF;
    return (float)lfd_recip_refined(lfd_sqrt_rare(sum));
}

// precision of a neighbour in camera px^-2 from its plane's entry (lfd_refine_add_neighbour_weighted's products)
LFD_HD void lfd_sigma_plane_prec(const LfdSlotPrec& ws, float q00, float q01, float q11, double& p00, double& p01, double& p11) {
    p00 = (double)q00 * ws.rxx; p01 = (double)q01 * ws.rxy; p11 = (double)q11 * ws.ryy;
}

// One point.  sl[0 .. ns): the reference's neighbours; s < ns: the winning slot; ws[0 .. ns) beside them when `planes` (else not read) and then
// o.qs / o.q00.. the gathered plane entries; otherwise every view has the isotropic precision iso = 1 / iso_sigma_px^2.  CAND: the candidates
// of the point (lfd_support_candidate at g.tau, from o.cert / o.wx / o.wy) take part when `accepted` (the refinement replaced the point); with
// CAND false, or accepted false, the winner alone does and nothing of o but qs is read.
template <int KMAX, bool CAND>
LFD_HD float lfd_sigma_point(const LfdSigmaRef& ref, const LfdSlot* sl, const LfdSlotPrec* ws, int ns, int s, const LfdSupportGeom& g,
                             bool planes, double iso, bool accepted, const LfdRefineGather& o, float X0, float X1, float X2) {
    if (!(lfd_finite(X0) && lfd_finite(X1) && lfd_finite(X2))) return LFD_SIGMA_INF;
    const double x0 = (double)X0, x1 = (double)X1, x2 = (double)X2;
    const double d0 = x0 - (double)ref.C[0], d1 = x1 - (double)ref.C[1], d2 = x2 - (double)ref.C[2];
    double sum = 0.0;
    {
        double p00 = iso, p01 = 0.0, p11 = iso;
        bool valid = true;
        if (planes) {
            valid = lfd_refine_prec_valid(o.qs[0], o.qs[1], o.qs[2]);
            lfd_sigma_plane_prec(ws[s], o.qs[0], o.qs[1], o.qs[2], p00, p01, p11);
        }
        if (valid) lfd_sigma_add_view(sum, sl[s].P, x0, x1, x2, d0, d1, d2, p00, p01, p11);
    }
    if constexpr (CAND) {
        if (accepted) {
            LFD_REFINE_UNROLL
            for (int j = 0; j < KMAX; ++j) {
                if (j < ns && j != s && lfd_support_candidate(sl[j], g, o.cert[j], o.wx[j], o.wy[j], X0, X1, X2)) {
                    double p00 = iso, p01 = 0.0, p11 = iso;
                    bool valid = true;
                    if (planes) {
                        valid = lfd_refine_prec_valid(o.q00[j], o.q01[j], o.q11[j]);
                        lfd_sigma_plane_prec(ws[j], o.q00[j], o.q01[j], o.q11[j], p00, p01, p11);
                    }
                    if (valid) lfd_sigma_add_view(sum, sl[j].P, x0, x1, x2, d0, d1, d2, p00, p01, p11);
                }
            }
        }
    }
    return lfd_sigma_finish(sum);
}

// the gate: max_rel_sigma == 0 keeps everything; otherwise a NaN and +inf drop
LFD_HD bool lfd_sigma_keep(float sigma_rel, float max_rel_sigma) { return max_rel_sigma == 0.0f || sigma_rel <= max_rel_sigma; }

// What the gate's own launch works on (device), by value in the kernel arguments.
struct LfdSigmaArgs {
    LfdPointStage st;
    int32_t* seg_counts;               // [n_refs * k] or null (zeroed before the launch)
    float* sigma;                      // [capacity] or null: sigma_rel of every input point
    const uint8_t* status;             // [capacity] or null: the refinement's status (candidates take part where it has LFD_REFINE_ACCEPTED)
    const float* const* prec;          // [n_refs * k] precision planes (device table), or null: the isotropic form
    float* ws_sigma;                   // workspace [n_wg * 256] or null: sigma_rel of every input point, for the compaction to move
    uint8_t* keep;                     // workspace [n_wg * 256]: 1 where the point is kept
    unsigned* wg_kept;                 // workspace [n_wg + 1]: kept points per workgroup
    double iso;                        // 1 / iso_sigma_px^2 (the isotropic form)
    float max_rel_sigma;
};

// Arguments of lfd_depth_sigma_filter / lfd_depth_sigma_filter_host that do not depend on the batch; what is wrong with them (and the status),
// or null.
inline const char* lfd_sigma_check(const lfd_points* in, const int64_t* ref_offsets_in, const float* const* precision, float iso_sigma_px,
                                   const uint8_t* refine_status, float support_thresh_px, float max_rel_sigma, const lfd_points* out,
                                   const int64_t* ref_offsets_out, const float* sigma_rel, const float* sigma_rel_out, int* code) {
    *code = LFD_ERR_INVALID;
    if (!in || !out || !ref_offsets_in || !ref_offsets_out) return "null in / out / ref_offsets";
    if (!in->xyz || !in->rgb || !in->err || !out->xyz || !out->rgb || !out->err) return "null point arrays";
    if (!in->cell || !in->slot) return "in->cell and in->slot are required";
    if (in->capacity < 0 || out->capacity < 0 || in->capacity > 0x7fffffffLL) return "capacity must be in [0, 2^31 - 1]";
    const bool iso = iso_sigma_px > 0.0f && iso_sigma_px <= 3.4028234e38f;
    if (iso_sigma_px != 0.0f && !iso) return "iso_sigma_px must be finite and >= 0";
    if ((precision != nullptr) == iso) return "exactly one of precision and iso_sigma_px > 0 must be given";
    if (!(max_rel_sigma >= 0.0f) || !(max_rel_sigma <= 3.4028234e38f)) return "max_rel_sigma must be finite and >= 0";
    if (refine_status && (!(support_thresh_px > 0.0f) || !(support_thresh_px <= 3.4028234e38f)))
        return "support_thresh_px must be finite and > 0 when refine_status is given";
    const struct { const void* p; long long elem; } a[7] = {{in->xyz, 12}, {in->rgb, 12}, {in->err, 4}, {in->cell, 4}, {in->slot, 1},
                                                            {refine_status, 1}, {sigma_rel, 4}};
    const struct { const void* p; long long elem; long long cap; } b[7] = {{out->xyz, 12, out->capacity}, {out->rgb, 12, out->capacity},
        {out->err, 4, out->capacity}, {out->cell, 4, out->capacity}, {out->slot, 1, out->capacity}, {sigma_rel_out, 4, out->capacity},
        {sigma_rel, 4, in->capacity}};
    for (int i = 0; i < 7; ++i)
        for (int j = 0; j < 7; ++j) {
            if (!a[i].p || !b[j].p || (i == 6 && j == 6)) continue;
            const uintptr_t a0 = reinterpret_cast<uintptr_t>(a[i].p), a1 = a0 + (uintptr_t)(a[i].elem * in->capacity);
            const uintptr_t b0 = reinterpret_cast<uintptr_t>(b[j].p), b1 = b0 + (uintptr_t)(b[j].elem * b[j].cap);
            if (a0 < b1 && b0 < a1) return "in and out overlap";
        }
    if (out->capacity < in->capacity) { *code = LFD_ERR_CAPACITY; return "out->capacity must be >= in->capacity"; }
    return nullptr;
}
