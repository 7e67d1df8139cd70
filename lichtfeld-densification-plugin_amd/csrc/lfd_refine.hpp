// Multi-view re-triangulation of supported points (lfd_refine_multiview): the per-point routine, compiled for the device
// (lfd_refine.hip) and for the host (lfd_host.hip's twin).  The support filter (lfd_support.hpp) finds, per two-view point, the OTHER neighbours of
// its reference whose own warp agrees with it; here their observations join the two that made the point in one N-view DLT, and the result
// replaces the point when it still passes the two-view tests and every view that agreed before agrees with it.
//
// Every rounding is written out (the build uses -ffp-contract=off).  The candidate set is lfd_support_candidate's (lfd_support.hpp), the one
// function the support filter counts with, so it is the filter's set bit for bit on both builds; the rows are lfd_eval_correspondence's f32
// rows; M = sum row row^T is one f64 fma chain in the fixed view order (reference, winning slot, candidates by ascending slot).  The two builds
// differ only where lfd_geometry.hpp's do: lfd_recip_refined (IEEE division / Newton-refined v_rcp_f64), lfd_sqrt_rare, lfd_rcp_f32,
// lfd_sqrt_f32.
//
// One routine, lfd_refine_point<KMAX, WEIGHTED>, serves lfd_refine_multiview and its precision-weighted variant: WEIGHTED adds the
// validity test of the participating planes and the weighted M; where a plane is invalid it runs lfd_refine_build_unweighted, the very code of
// the other instantiation.
#pragma once

#include <stdint.h>

#include "../../include/lfd_densify.h"
#include "lfd_geometry.hpp"
#include "lfd_support.hpp"

#define LFD_REFINE_ACCEPTED 0x80       /* status: n_extra | (accepted ? 0x80 : 0) */
#define LFD_REFINE_WEIGHTED 0x40       /* status: the weighted rows were used (every participating view's precision was valid) */

struct LfdRefineRef {            // the reference itself
    float P[12];                 // interleaved (LfdRefConst)
    float sx, sy;
};

struct LfdSlotPrec {             // beside LfdSlot (weighted only): the neighbour's precision plane and what turns its entries into camera px^-2
    const float* prec;           // [H*W*3]: (q00, q01, q11) per cell, px^-2 of the neighbour's MATCH image
    double rxx, rxy, ryy;        // 1 / (sx sx), 1 / (sx sy), 1 / (sy sy) through lfd_recip_refined (the products of f32 values are exact)
};

struct LfdRefineGather {         // what the caller gathered at the point's cell, [KMAX] each, entries j < ns, j != s (the rest is not read)
    const float* cert;           // certainty of the other neighbours
    const float* wx;             // their warps' B side
    const float* wy;
    const float* q00;            // weighted only (null otherwise): their precision, and qs[3] the winning slot's
    const float* q01;
    const float* q11;
    const float* qs;
};

// M (upper triangle: m00 m01 m02 m03 m11 m12 m13 m22 m23 m33) += the two DLT rows of one view, u p2 - p0 and v p2 - p1, formed in f32 exactly as
// lfd_eval_correspondence forms them (multiply, then subtract); the products of f32 values are exact in f64.  `first`: M is set, not added to
// (the products themselves, as lfd_null_vector_rows starts).
LFD_HD void lfd_refine_add_view(double* M, const float* Pi, float u, float v, bool first) {
    float ru[4], rv[4];
    for (int c = 0; c < 4; ++c) {
        ru[c] = u * Pi[8 + c] - Pi[2 * c];
        rv[c] = v * Pi[8 + c] - Pi[2 * c + 1];
    }
    {
        const double a0 = (double)ru[0], a1 = (double)ru[1], a2 = (double)ru[2], a3 = (double)ru[3];
        if (first) {
            M[0] = a0 * a0; M[1] = a0 * a1; M[2] = a0 * a2; M[3] = a0 * a3;
            M[4] = a1 * a1; M[5] = a1 * a2; M[6] = a1 * a3; M[7] = a2 * a2; M[8] = a2 * a3; M[9] = a3 * a3;
        } else {
            M[0] = fma(a0, a0, M[0]); M[1] = fma(a0, a1, M[1]); M[2] = fma(a0, a2, M[2]); M[3] = fma(a0, a3, M[3]);
            M[4] = fma(a1, a1, M[4]); M[5] = fma(a1, a2, M[5]); M[6] = fma(a1, a3, M[6]);
            M[7] = fma(a2, a2, M[7]); M[8] = fma(a2, a3, M[8]); M[9] = fma(a3, a3, M[9]);
        }
    }
    {
        const double a0 = (double)rv[0], a1 = (double)rv[1], a2 = (double)rv[2], a3 = (double)rv[3];
        M[0] = fma(a0, a0, M[0]); M[1] = fma(a0, a1, M[1]); M[2] = fma(a0, a2, M[2]); M[3] = fma(a0, a3, M[3]);
        M[4] = fma(a1, a1, M[4]); M[5] = fma(a1, a2, M[5]); M[6] = fma(a1, a3, M[6]);
        M[7] = fma(a2, a2, M[7]); M[8] = fma(a2, a3, M[8]); M[9] = fma(a3, a3, M[9]);
    }
}

// Smallest eigenvector of the symmetric positive semi-definite 4x4 matrix M (upper triangle as above) by the scheme of lfd_null_vector_rows
// (DESIGN 4.1): LDL^T without pivoting, Newton-refined pivot reciprocals, inverse iteration from e4 (its first solve is the last column of
// L^-T), lfd_nullvec_settled from the second solve on, at most LFD_NULLVEC_MAXIT solves per pass and LFD_NULLVEC_PASSES passes.  Pass 0 is a
// plain loop here (this routine runs once per supported point behind the dense kernel, not inside its geometry loop); like lfd_null_vector_rows'
// it brings an iterate above 2^64 back before its fifth solve.  The shifted passes ARE lfd_null_vector_rows' (LFD_NULLVEC_SHIFTED_PASSES,
// lfd_geometry.hpp: the Rayleigh shift backed off by the residual, the negative-pivot test, the step-down and the bisections of a shift above
// mu4, the restart from e4, the rescaling), with nothing to rebuild: M stays where it is (ten values).  c[4]: an un-normalised multiple; returns
// the number of solves, the free first one included as lfd_null_vector_rows counts it (3 .. 1 + LFD_NULLVEC_MAXIT LFD_NULLVEC_PASSES).
LFD_HD int lfd_null_vector_sym(const double* M, double* c) {
    const double m00 = M[0], m01 = M[1], m02 = M[2], m03 = M[3], m11 = M[4], m12 = M[5], m13 = M[6], m22 = M[7], m23 = M[8], m33 = M[9];
    double x0, x1, x2, x3;
    int it = 1;
    bool settled = false;
    double rho = 0.0;
    {
        LFD_NULLVEC_FACTORISE(m00, m11, m22, m33);
        // first solve from e4: the last column of L^-T
        x3 = 1.0;
        x2 = -l32;
        x1 = fma(-l21, x2, -l31);
        x0 = fma(-l10, x1, fma(-l20, x2, -l30));
        for (int k = 1; k <= LFD_NULLVEC_MAXIT; ++k) {
            if (k == 5) LFD_NULLVEC_KEEP_IN_RANGE();
            const double o0 = x0, o1 = x1, o2 = x2, o3 = x3;
            LFD_NULLVEC_SOLVE(x0, x1, x2, x3, x0, x1, x2, x3);
            ++it;
            if (k >= 2 && lfd_nullvec_settled(x0, x1, x2, x3, o0, o1, o2, o3)) {
                settled = true;
                // M x = d3 o, so the Rayleigh quotient of x is d3 (x . o) / (x . x)
                const double xo = fma(x3, o3, fma(x2, o2, fma(x1, o1, x0 * o0)));
                const double xx = fma(x3, x3, fma(x2, x2, fma(x1, x1, x0 * x0)));
                rho = (d3 * xo) * lfd_recip_refined(xx);
                break;
            }
        }
    }
    // lfd_nullvec_settled reads a small change of direction as convergence, and pass 0 changes little next to v3 as well: started nearly
    // orthogonal to v4 (a far point) with sigma4/sigma3 close to 1 it drifts away from v3 by less than LFD_NULLVEC_TOL per solve.  The inertia
    // tells the two apart: M - sh I = L D L^T just below the eigenvalue the pass settled on, sh = rho (1 - 2^-10), has a negative pivot iff M
    // has an eigenvalue below sh - x is not v4, and the shifted passes (which search their shift from such a state) take over.  2^-10 is below
    // the gap 1 - r^2 of every r <= 0.999 the rules ask a direction for.  No negative pivot: x is returned as it is, same bits.  (NaN compares
    // false: a NaN leaves as before.)
    if (settled) {
        const double sh = fma(-0x1p-10, rho, rho);
        LFD_NULLVEC_FACTORISE(m00 - sh, m11 - sh, m22 - sh, m33 - sh);
        (void)s0; (void)s1; (void)s2; (void)l32;
        settled = !LFD_NULLVEC_NEGATIVE_PIVOT();
    }
#define LFD_SYM_KEEPS_M()
    LFD_NULLVEC_SHIFTED_PASSES(LFD_SYM_KEEPS_M)
#undef LFD_SYM_KEEPS_M
    c[0] = x0; c[1] = x1; c[2] = x2; c[3] = x3;
    return it;
}

// X' = c[0..2] / c[3] rounded to f32 as the two-view path rounds it.  False where that path's w guard would act (|c3| / |c| < 1e-12: a point
// at infinity has no place in the candidates' test, which takes the homogeneous coordinate as 1) or a coordinate is not finite.
LFD_HD bool lfd_refine_dehomogenise(const double* c, float& X0, float& X1, float& X2) {
    const double c33 = c[3] * c[3];
    const double n2 = fma(c[0], c[0], fma(c[1], c[1], fma(c[2], c[2], c33)));
    const double r = lfd_recip_refined(c[3]);
    X0 = (float)(c[0] * r);
    X1 = (float)(c[1] * r);
    X2 = (float)(c[2] * r);
    const bool guard = c33 < 1e-24 * n2;
    // (the squares rely on lfd_null_vector_sym's rescaling, which keeps |c| below 1e154: a larger c would give Inf < Inf and skip the guard)
    return !guard && (n2 == n2) && lfd_finite(X0) && lfd_finite(X1) && lfd_finite(X2);
}

// The two-view test of lfd_eval_correspondence at X (reference, winning slot): pz > 0 in both and err = sqrt(max of the squared reprojection
// distances) <= reproj_thresh, the same operations and the same comparison.  A NaN rejects.
LFD_HD bool lfd_refine_two_view(const float* Pa, const float* Pb, float X0, float X1, float X2, float ua, float va, float ub, float vb,
                                float reproj_thresh, float& err) {
    float z1, z2;
    const float q1 = lfd_reproj_sq(Pa, X0, X1, X2, 1.0f, ua, va, z1);
    const float q2 = lfd_reproj_sq(Pb, X0, X1, X2, 1.0f, ub, vb, z2);
    const float qm = (q1 > q2 || q1 != q1) ? q1 : q2;
    err = lfd_sqrt_f32(qm);
    return (err <= reproj_thresh) && (z1 > 0.0f) && (z2 > 0.0f);
}

// ---- precision-weighted rows (lfd_refine_multiview_weighted) ------------------------------------------------------------------------
LFD_HD void lfd_slot_prec_scale(float sx, float sy, LfdSlotPrec& o) {
    const double x = (double)sx, y = (double)sy;
    o.rxx = lfd_recip_refined(x * x);
    o.rxy = lfd_recip_refined(x * y);
    o.ryy = lfd_recip_refined(y * y);
}

// valid(j): the three values finite and the matrix positive definite; the determinant in f64 (two exact products, one rounding)
LFD_HD bool lfd_refine_prec_valid(float q00, float q01, float q11) {
    const double a = (double)q00 * (double)q11, b = (double)q01 * (double)q01;
    const double det = a - b;
    return lfd_finite(q00) && lfd_finite(q01) && lfd_finite(q11) && q00 > 0.0f && q11 > 0.0f && det > 0.0;
}

// M (ten entries, as above) += ru^T (a ru + b rv) + rv^T (b ru + c rv): the view's two f32 rows weighted by the symmetric 2x2 (a b; b c).
// Per column c: tu_c = fma(b, rv_c, a ru_c), tv_c = fma(c, rv_c, b ru_c); per entry (i <= j): M_ij = fma(rv_i, tv_j, fma(ru_i, tu_j, M_ij)).
LFD_HD void lfd_refine_add_view_weighted(double* M, const float* Pi, float u, float v, double a, double b, double c) {
    double ru[4], rv[4], tu[4], tv[4];
    for (int e = 0; e < 4; ++e) {
        const float fu = u * Pi[8 + e] - Pi[2 * e];
        const float fv = v * Pi[8 + e] - Pi[2 * e + 1];
        ru[e] = (double)fu; rv[e] = (double)fv;
        tu[e] = fma(b, rv[e], a * ru[e]);
        tv[e] = fma(c, rv[e], b * ru[e]);
    }
    M[0] = fma(rv[0], tv[0], fma(ru[0], tu[0], M[0])); M[1] = fma(rv[0], tv[1], fma(ru[0], tu[1], M[1]));
    M[2] = fma(rv[0], tv[2], fma(ru[0], tu[2], M[2])); M[3] = fma(rv[0], tv[3], fma(ru[0], tu[3], M[3]));
    M[4] = fma(rv[1], tv[1], fma(ru[1], tu[1], M[4])); M[5] = fma(rv[1], tv[2], fma(ru[1], tu[2], M[5]));
    M[6] = fma(rv[1], tv[3], fma(ru[1], tu[3], M[6])); M[7] = fma(rv[2], tv[2], fma(ru[2], tu[2], M[7]));
    M[8] = fma(rv[2], tv[3], fma(ru[2], tu[3], M[8])); M[9] = fma(rv[3], tv[3], fma(ru[3], tu[3], M[9]));
}

// One neighbour view into M: its precision in camera px^-2 (q / (s s)) times w2 = 1 / (pz pz), pz the f32 depth of the two-view X in that view
// (what turns the algebraic rows into first-order pixel residuals).  lam += (p00 + p11) / 2.
LFD_HD void lfd_refine_add_neighbour_weighted(double* M, double& lam, const LfdSlot& sl, const LfdSlotPrec& ws, float q00, float q01,
                                              float q11, float X0, float X1, float X2, float u, float v) {
    const double p00 = (double)q00 * ws.rxx, p01 = (double)q01 * ws.rxy, p11 = (double)q11 * ws.ryy;
    const double z = (double)lfd_proj_row(sl.P, 2, X0, X1, X2, 1.0f);
    const double w2 = lfd_recip_refined(z * z);
    lam = lam + (p00 + p11) * 0.5;
    lfd_refine_add_view_weighted(M, sl.P, u, v, w2 * p00, w2 * p01, w2 * p11);
}

// ---- one point ---------------------------------------------------------------------------------------------------------------------------------
#if defined(__HIP_DEVICE_COMPILE__)
#define LFD_REFINE_UNROLL _Pragma("unroll")
#else
#define LFD_REFINE_UNROLL
#endif

// Today's M: reference, winning slot, candidates by ascending slot, every view with weight one.
template <int KMAX>
LFD_HD void lfd_refine_build_unweighted(double* M, const LfdRefineRef& ref, const LfdSlot* sl, int s, unsigned cand, const LfdSupportGeom& g,
                                        const LfdRefineGather& o, float ua, float va, float ub, float vb) {
    lfd_refine_add_view(M, ref.P, ua, va, true);
    lfd_refine_add_view(M, sl[s].P, ub, vb, false);
    LFD_REFINE_UNROLL
    for (int j = 0; j < KMAX; ++j) {
        if ((cand >> j) & 1u) {
            const float uj = lfd_match_px(o.wx[j], g.wm1) * sl[j].sx, vj = lfd_match_px(o.wy[j], g.hm1) * sl[j].sy;
            lfd_refine_add_view(M, sl[j].P, uj, vj, false);
        }
    }
}

// The weighted M: winning slot, candidates by ascending slot, reference LAST - it has no matching noise (a cell centre), so it enters
// isotropically with lamA = the sum of the neighbours' mean precisions: as precise as everything that looked at it, which also makes the
// solution invariant to a common scale of the planes.  (X0, X1, X2): the two-view point, whose depths scale the rows.
template <int KMAX>
LFD_HD void lfd_refine_build_weighted(double* M, const LfdRefineRef& ref, const LfdSlot* sl, const LfdSlotPrec* ws, int s, unsigned cand,
                                      const LfdSupportGeom& g, const LfdRefineGather& o, float ua, float va, float ub, float vb, float X0, float X1,
                                      float X2) {
    for (int e = 0; e < 10; ++e) M[e] = 0.0;
    double lam = 0.0;
    lfd_refine_add_neighbour_weighted(M, lam, sl[s], ws[s], o.qs[0], o.qs[1], o.qs[2], X0, X1, X2, ub, vb);
    LFD_REFINE_UNROLL
    for (int j = 0; j < KMAX; ++j) {
        if ((cand >> j) & 1u) {
            const float uj = lfd_match_px(o.wx[j], g.wm1) * sl[j].sx, vj = lfd_match_px(o.wy[j], g.hm1) * sl[j].sy;
            lfd_refine_add_neighbour_weighted(M, lam, sl[j], ws[j], o.q00[j], o.q01[j], o.q11[j], X0, X1, X2, uj, vj);
        }
    }
    const double z = (double)lfd_proj_row(ref.P, 2, X0, X1, X2, 1.0f);
    const double wa = lam * lfd_recip_refined(z * z);
    lfd_refine_add_view_weighted(M, ref.P, ua, va, wa, 0.0, wa);
}

// One point.  sl[0 .. ns): the reference's neighbours (ws[0 .. ns) beside them when WEIGHTED, else not read); s: the winning slot (s < ns);
// (xan, yan) / (xbn, ybn): the reference's and the winner's normalised observations of the cell; o: what the other neighbours hold at the cell
// (KMAX >= ns).  The candidates are lfd_support_candidate's.  WEIGHTED and every participating view (slot s, the candidates) has a valid
// precision: the weighted M; otherwise the unweighted one - with WEIGHTED false nothing else is compiled.  Solve and acceptance are the same.
// Returns the status byte n_extra | LFD_REFINE_WEIGHTED | LFD_REFINE_ACCEPTED; X0, X1, X2, err are replaced iff it has LFD_REFINE_ACCEPTED.
template <int KMAX, bool WEIGHTED>
LFD_HD unsigned lfd_refine_point(const LfdRefineRef& ref, const LfdSlot* sl, const LfdSlotPrec* ws, int ns, int s, const LfdSupportGeom& g,
                                 float xan, float yan, float xbn, float ybn, const LfdRefineGather& o, float& X0, float& X1, float& X2,
                                 float& err) {
    unsigned cand = 0u;
    LFD_REFINE_UNROLL
    for (int j = 0; j < KMAX; ++j) {
        if (j < ns && j != s) cand |= lfd_support_candidate(sl[j], g, o.cert[j], o.wx[j], o.wy[j], X0, X1, X2) ? (1u << j) : 0u;
    }
    if (cand == 0u) return 0u;
    unsigned n_extra = 0u;
    for (unsigned m = cand; m; m &= m - 1u) ++n_extra;
    bool weighted = false;
    if constexpr (WEIGHTED) {
        weighted = lfd_refine_prec_valid(o.qs[0], o.qs[1], o.qs[2]);
        LFD_REFINE_UNROLL
        for (int j = 0; j < KMAX; ++j) {
            if ((cand >> j) & 1u) weighted = lfd_refine_prec_valid(o.q00[j], o.q01[j], o.q11[j]) && weighted;
        }
    }

    const float ua = lfd_match_px(xan, g.wm1) * ref.sx, va = lfd_match_px(yan, g.hm1) * ref.sy;
    const float ub = lfd_match_px(xbn, g.wm1) * sl[s].sx, vb = lfd_match_px(ybn, g.hm1) * sl[s].sy;
    double M[10];
    if (weighted) {
        if constexpr (WEIGHTED) lfd_refine_build_weighted<KMAX>(M, ref, sl, ws, s, cand, g, o, ua, va, ub, vb, X0, X1, X2);
    } else {
        lfd_refine_build_unweighted<KMAX>(M, ref, sl, s, cand, g, o, ua, va, ub, vb);
    }
    const unsigned base = n_extra | (weighted ? (unsigned)LFD_REFINE_WEIGHTED : 0u);
    double c[4];
    lfd_null_vector_sym(M, c);
    float Y0, Y1, Y2, e;
    bool ok = lfd_refine_dehomogenise(c, Y0, Y1, Y2);
    ok = lfd_refine_two_view(ref.P, sl[s].P, Y0, Y1, Y2, ua, va, ub, vb, g.reproj_thresh, e) && ok;
    LFD_REFINE_UNROLL
    for (int j = 0; j < KMAX; ++j) {
        if ((cand >> j) & 1u)
            ok = lfd_support_agree(sl[j].P, sl[j].sx, sl[j].sy, Y0, Y1, Y2, o.wx[j], o.wy[j], g.wm1, g.hm1, g.tau) && ok;
    }
    if (!ok) return base;
    X0 = Y0; X1 = Y1; X2 = Y2; err = e;
    return base | LFD_REFINE_ACCEPTED;
}

// What a launch works on (device), by value in the kernel arguments.
struct LfdRefineArgs {
    LfdPointStage st;
    float* o_xyz; float* o_err;
    uint8_t* status;                   // [capacity] or null
    unsigned long long* counters;      // [2] or null: points refined, points with a candidate that kept their two-view position; added to
                                       // ([3] when prec is set: + points solved with weighted rows; without prec element 2 is never touched)
    const float* const* prec;          // lfd_refine_multiview_weighted: [n_refs * k] precision planes (device table; entries at j >= n_slots[r]
                                       // are not read); null: lfd_refine_multiview
};

// Arguments of lfd_refine_multiview / lfd_refine_multiview_host that do not depend on the batch; what is wrong with them, or null.
inline const char* lfd_refine_check(const lfd_points* in, const int64_t* ref_offsets, float support_thresh_px, float reproj_thresh,
                                    const float* xyz_out, const float* err_out, const uint8_t* status) {
    if (!in || !ref_offsets) return "null in / ref_offsets";
    if (!in->xyz || !in->err || !xyz_out || !err_out) return "null point arrays";
    if (!in->cell || !in->slot) return "in->cell and in->slot are required";
    if (in->capacity < 0 || in->capacity > 0x7fffffffLL) return "capacity must be in [0, 2^31 - 1]";
    if (!(support_thresh_px > 0.0f) || !(support_thresh_px <= 3.4028234e38f)) return "support_thresh_px must be finite and > 0";
    if (!(reproj_thresh > 0.0f) || !(reproj_thresh <= 3.4028234e38f)) return "reproj_thresh must be finite and > 0";
    const bool in_place = xyz_out == in->xyz && err_out == in->err;
    const long long cap = in->capacity;
    const struct { const void* p; long long elem; } a[5] = {{in->xyz, 12}, {in->rgb, 12}, {in->err, 4}, {in->cell, 4}, {in->slot, 1}},
                                                    b[3] = {{xyz_out, 12}, {err_out, 4}, {status, 1}};
    for (int j = 0; j < 3; ++j) {
        if (!b[j].p) continue;
        const uintptr_t b0 = reinterpret_cast<uintptr_t>(b[j].p), b1 = b0 + (uintptr_t)(b[j].elem * cap);
        for (int i = 0; i < 5; ++i) {
            if (!a[i].p) continue;
            if (in_place && ((j == 0 && i == 0) || (j == 1 && i == 2))) continue;
            const uintptr_t a0 = reinterpret_cast<uintptr_t>(a[i].p), a1 = a0 + (uintptr_t)(a[i].elem * cap);
            if (a0 < b1 && b0 < a1) return "xyz_out / err_out / status must be in->xyz and in->err themselves or overlap nothing of in";
        }
        for (int i = 0; i < j; ++i) {
            if (!b[i].p) continue;
            const uintptr_t a0 = reinterpret_cast<uintptr_t>(b[i].p), a1 = a0 + (uintptr_t)(b[i].elem * cap);
            if (a0 < b1 && b0 < a1) return "xyz_out, err_out and status overlap each other";
        }
    }
    return nullptr;
}

// The one argument lfd_refine_multiview_weighted[_host] adds, checked behind the batch's own validation; what is wrong with it, or null.
inline const char* lfd_refine_check_precision(const lfd_batch* b, const float* const* precision) {
    if (!precision) return "null precision";
    for (int r = 0; r < b->n_refs; ++r)
        for (int j = 0; j < b->n_slots[r]; ++j)
            if (!precision[(size_t)r * b->k + j]) return "null precision plane in a valid slot";
    return nullptr;
}

// The solver's pieces (lfd_geometry.hpp) have no user behind this header.
#undef LFD_NULLVEC_FACTORISE_D
#undef LFD_NULLVEC_FACTORISE
#undef LFD_NULLVEC_SOLVE
#undef LFD_NULLVEC_KEEP_IN_RANGE
#undef LFD_NULLVEC_SHIFTED_SOLVES
#undef LFD_NULLVEC_NEGATIVE_PIVOT
#undef LFD_NULLVEC_PIVOTS_AT_SH
#undef LFD_NULLVEC_SHIFTED_PASSES
