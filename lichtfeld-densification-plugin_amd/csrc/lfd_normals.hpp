// Per-point surface normals from the resident warps (lfd_estimate_normals): the per-point routine, compiled for the device
// (lfd_normals.hip) and for the host (lfd_host.hip's twin).  A point sits on a grid cell of its reference; the winning neighbour's warp around
// that cell gives the neighbouring surface samples Y_q.  The normal is the cross product of the two regression slopes of Y on the cell offsets
// (dx, dy) over the window cells that are live, pass the two-view test and lie on the point's side of any depth step, oriented towards the
// reference's centre.  The common factor 1 / det of the slopes cancels in the direction: nothing is divided or decomposed.
//
// Every rounding is written out (the build uses -ffp-contract=off).  Y_q is lfd_eval_correspondence's f32 point - the routine that made the
// point itself, with the Sampson and parallax gates off -, live(q) is lfd_support_filter's (lfd_support.hpp), the depths are lfd_proj_row's
// chain.  The counts and the moments of (dx, dy) are exact integers; the sums of D_q = Y_q - X are plain f64 adds in raster order (a small
// integer times a double is exact), so both builds hold the same sums bit for bit wherever they hold the same Y_q.  They differ where
// lfd_geometry.hpp's do, and in the final normalisation: IEEE sqrt and divide on the host, lfd_sqrt_rare / lfd_recip_refined on the device
// (components within one f32 ulp).
#pragma once

#include <stdint.h>

#include "../../include/lfd_densify.h"
#include "lfd_geometry.hpp"
#include "lfd_support.hpp"

#define LFD_NORMAL_FITTED 0x80         /* status: cells that took part | (fitted ? 0x80 : 0); 0 where the guard acted */
#define LFD_NORMAL_MAX_RADIUS 4

struct LfdNormalSlot {           // one neighbour of the reference at work (LDS on the device, a table on the host), beside its LfdPairConst
    const float* cert;
    const float* warp;
    const uint8_t* mask_b;
};

struct LfdNormalAcc {            // what lives across the window loop: nine f64 sums (three 3-vectors) and six integers
    double A0[3], Ax[3], Ay[3];  // sum D_q, sum dx D_q, sum dy D_q
    int n, sx, sy, sxx, sxy, syy;
};

struct LfdNormalPoint {          // the point: its position, the view vector Vw = C_A - X (f64), its depth in the reference, the depth band
    float X[3];
    double Vw[3];
    float pz, band;              // band = depth_step_rel * pz (f32)
};

// the window's two-view test: lfd_eval_correspondence with the Sampson and the parallax gate off and no_filter off
LFD_HD LfdKernelParams lfd_normal_params(const LfdSupportGeom& g) {
    LfdKernelParams kp;
    kp.sampson_thresh = 0.0; kp.certainty_thresh = 0.0f; kp.reproj_thresh = g.reproj_thresh; kp.dot_thresh = 0.0f;
    kp.wm1 = g.wm1; kp.hm1 = g.hm1; kp.use_sampson = 0; kp.use_parallax = 0; kp.no_filter = 0;
    return kp;
}

// v / |v| rounded to f32 once per component; false (and zeros) where v.v is not finite or not > 0
LFD_HD bool lfd_normal_unit(const double* v, float* out) {
    const double nn = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    out[0] = 0.0f; out[1] = 0.0f; out[2] = 0.0f;
    if (!(nn > 0.0) || !(nn <= 1.7976931348623157e308)) return false;
#if defined(__HIP_DEVICE_COMPILE__)
    const double r = lfd_recip_refined(lfd_sqrt_rare(nn));
    out[0] = (float)(v[0] * r); out[1] = (float)(v[1] * r); out[2] = (float)(v[2] * r);
#else
    const double l = sqrt(nn);
    out[0] = (float)(v[0] / l); out[1] = (float)(v[1] / l); out[2] = (float)(v[2] / l);
#endif
    return true;
}

// The point's own part.  C: the reference's centre (LfdRefConst::C).  `fallback` receives Vw / |Vw| ((0,0,0) where |Vw| is zero or not
// finite).  Returns the guard's verdict on X alone: X finite and its depth in the reference > 0 (the cell and the slot are the caller's to
// test, before any address is formed from them).
LFD_HD bool lfd_normal_begin(const LfdRefConst& rc, float X0, float X1, float X2, float depth_step_rel, LfdNormalPoint& pt, float* fallback) {
    pt.X[0] = X0; pt.X[1] = X1; pt.X[2] = X2;
    pt.Vw[0] = (double)rc.C[0] - (double)X0;
    pt.Vw[1] = (double)rc.C[1] - (double)X1;
    pt.Vw[2] = (double)rc.C[2] - (double)X2;
    lfd_normal_unit(pt.Vw, fallback);
    pt.pz = lfd_proj_row(rc.P, 2, X0, X1, X2, 1.0f);
    pt.band = depth_step_rel * pt.pz;
    return lfd_finite(X0) && lfd_finite(X1) && lfd_finite(X2) && pt.pz > 0.0f;
}

LFD_HD void lfd_normal_clear(LfdNormalAcc& a) {
    for (int e = 0; e < 3; ++e) { a.A0[e] = 0.0; a.Ax[e] = 0.0; a.Ay[e] = 0.0; }
    a.n = 0; a.sx = 0; a.sy = 0; a.sxx = 0; a.sxy = 0; a.syy = 0;
}

// One window cell q = (qx, qy) = (x + dx, y + dy), inside the grid.  cert and (xan, yan, xbn, ybn): the winning slot's raw certainty and the
// two sides of its observation at q (the caller's loads).  mask_a: the reference's mask or null.
LFD_HD void lfd_normal_cell(LfdNormalAcc& a, const LfdNormalPoint& pt, const LfdRefConst& rc, const LfdPairConst& pc, const uint8_t* mask_a,
                            const uint8_t* mask_b, const LfdSupportGeom& g, const LfdKernelParams& kp, int qx, int qy, int dx, int dy, float cert,
                            float xan, float yan, float xbn, float ybn) {
    bool live = lfd_support_live(cert);
    if (live && mask_b) {
        const long long m = lfd_support_mask_index(xbn, ybn, g.W, g.H, g.mask_sx, g.mask_sy, g.w_match, g.h_match);
        live = m >= 0 && mask_b[m] != 0;
    }
    if (live && mask_a)
        live = mask_a[(size_t)lfd_nearest_src(qy, g.mask_sy, g.h_match) * g.w_match + lfd_nearest_src(qx, g.mask_sx, g.w_match)] != 0;
    if (!live) return;
    LfdCellResult res;
    lfd_eval_correspondence(rc, pc, xan, yan, xbn, ybn, kp, res);
    if (!res.keep) return;
    const float pzq = lfd_proj_row(rc.P, 2, res.x, res.y, res.z, 1.0f);
    const float d = pzq - pt.pz;
    if (!(fabsf(d) <= pt.band)) return;               // a depth step between q and the point (a NaN rejects)
    const double D0 = (double)res.x - (double)pt.X[0], D1 = (double)res.y - (double)pt.X[1], D2 = (double)res.z - (double)pt.X[2];
    const double fx = (double)dx, fy = (double)dy;
    a.A0[0] = a.A0[0] + D0; a.A0[1] = a.A0[1] + D1; a.A0[2] = a.A0[2] + D2;
    a.Ax[0] = a.Ax[0] + fx * D0; a.Ax[1] = a.Ax[1] + fx * D1; a.Ax[2] = a.Ax[2] + fx * D2;
    a.Ay[0] = a.Ay[0] + fy * D0; a.Ay[1] = a.Ay[1] + fy * D1; a.Ay[2] = a.Ay[2] + fy * D2;
    a.n += 1; a.sx += dx; a.sy += dy; a.sxx += dx * dx; a.sxy += dx * dy; a.syy += dy * dy;
}

// The fit.  nrm: the fallback on entry, the normal on return; returns the status byte.
LFD_HD unsigned lfd_normal_finish(const LfdNormalAcc& acc, const LfdNormalPoint& pt, float* nrm) {
    const long long n = acc.n, sx = acc.sx, sy = acc.sy;
    const long long a = n * acc.sxx - sx * sx, b = n * acc.sxy - sx * sy, c = n * acc.syy - sy * sy;
    const unsigned st = (unsigned)acc.n;
    if (a * c - b * b <= 0) return st;                 // fewer than three cells, or all of them collinear
    const double fn = (double)n, fsx = (double)sx, fsy = (double)sy;
    double U[3], V[3], N[3];
    for (int e = 0; e < 3; ++e) {
        U[e] = fn * acc.Ax[e] - fsx * acc.A0[e];
        V[e] = fn * acc.Ay[e] - fsy * acc.A0[e];
    }
    N[0] = U[1] * V[2] - U[2] * V[1];
    N[1] = U[2] * V[0] - U[0] * V[2];
    N[2] = U[0] * V[1] - U[1] * V[0];
    const double dot = (N[0] * pt.Vw[0] + N[1] * pt.Vw[1]) + N[2] * pt.Vw[2];
    if (dot < 0.0) { N[0] = -N[0]; N[1] = -N[1]; N[2] = -N[2]; }
    float u[3];
    if (!lfd_normal_unit(N, u)) return st;
    nrm[0] = u[0]; nrm[1] = u[1]; nrm[2] = u[2];
    return st | (unsigned)LFD_NORMAL_FITTED;
}

// One point over plain pointers, the window walked in raster order with every value read where it is needed: the twin's form of the routine
// (the kernel issues a window row's loads before its arithmetic and calls the same three functions).  sl / pc [ns]: the reference's
// neighbours; ax / ay: the A-grid axes (two-channel warps).  nrm[3] receives the normal; returns the status byte.
inline unsigned lfd_normal_point(const LfdRefConst& rc, const LfdPairConst* pc, const LfdNormalSlot* sl, int ns, const uint8_t* mask_a,
                                 const float* ax, const float* ay, const LfdSupportGeom& g, const LfdKernelParams& kp, int R, float depth_step_rel,
                                 int cell, int s, float X0, float X1, float X2, float* nrm) {
    LfdNormalPoint pt;
    const bool ok = lfd_normal_begin(rc, X0, X1, X2, depth_step_rel, pt, nrm);
    const long long HW = (long long)g.H * g.W;
    if (!ok || cell < 0 || (long long)cell >= HW || s >= ns) return 0u;      // no address is formed from a cell or a slot outside the batch
    const float* cert = sl[s].cert;
    const float* warp = sl[s].warp;
    const int y = cell / g.W, x = cell - y * g.W;
    LfdNormalAcc acc;
    lfd_normal_clear(acc);
    for (int dy = -R; dy <= R; ++dy) {
        const int qy = y + dy;
        if (qy < 0 || qy >= g.H) continue;
        for (int dx = -R; dx <= R; ++dx) {
            const int qx = x + dx;
            if (qx < 0 || qx >= g.W) continue;
            const size_t q = (size_t)qy * g.W + qx;
            const float* wp = warp + q * g.C;
            const float xan = g.C == 4 ? wp[0] : ax[qx], yan = g.C == 4 ? wp[1] : ay[qy];
            lfd_normal_cell(acc, pt, rc, pc[s], mask_a, sl[s].mask_b, g, kp, qx, qy, dx, dy, cert[q], xan, yan, wp[g.C - 2], wp[g.C - 1]);
        }
    }
    return lfd_normal_finish(acc, pt, nrm);
}

// What a launch works on (device), by value in the kernel arguments.
struct LfdNormalArgs {
    LfdPointStage st;                  // (g.tau unused; g.reproj_thresh: the window cells' two-view test)
    float* normals;                    // [3 * capacity]
    uint8_t* status;                   // [capacity] or null
    unsigned long long* counters;      // [2] or null: points fitted, points that fell back; added to
    int32_t radius;
    float depth_step_rel;
};

// Arguments of lfd_estimate_normals / lfd_estimate_normals_host that do not depend on the batch; what is wrong with them, or null.
inline const char* lfd_normals_check(const lfd_points* in, const int64_t* ref_offsets, int32_t radius_cells, float depth_step_rel,
                                     float reproj_thresh, const float* normals_out, const uint8_t* status) {
    if (!in || !ref_offsets) return "null in / ref_offsets";
    if (!in->xyz || !normals_out) return "null point arrays";
    if (!in->cell || !in->slot) return "in->cell and in->slot are required";
    if (in->capacity < 0 || in->capacity > 0x7fffffffLL) return "capacity must be in [0, 2^31 - 1]";
    if (radius_cells < 1 || radius_cells > LFD_NORMAL_MAX_RADIUS) return "radius_cells must be in [1, 4]";
    if (!(depth_step_rel > 0.0f) || !(depth_step_rel <= 3.4028234e38f)) return "depth_step_rel must be finite and > 0";
    if (!(reproj_thresh > 0.0f) || !(reproj_thresh <= 3.4028234e38f)) return "reproj_thresh must be finite and > 0";
    const long long cap = in->capacity;
    const struct { const void* p; long long elem; } a[5] = {{in->xyz, 12}, {in->rgb, 12}, {in->err, 4}, {in->cell, 4}, {in->slot, 1}},
                                                    b[2] = {{normals_out, 12}, {status, 1}};
    for (int j = 0; j < 2; ++j) {
        if (!b[j].p) continue;
        const uintptr_t b0 = reinterpret_cast<uintptr_t>(b[j].p), b1 = b0 + (uintptr_t)(b[j].elem * cap);
        for (int i = 0; i < 5; ++i) {
            if (!a[i].p) continue;
            const uintptr_t a0 = reinterpret_cast<uintptr_t>(a[i].p), a1 = a0 + (uintptr_t)(a[i].elem * cap);
            if (a0 < b1 && b0 < a1) return "normals_out / status must overlap nothing of in";
        }
    }
    if (status) {
        const uintptr_t a0 = reinterpret_cast<uintptr_t>(normals_out), a1 = a0 + (uintptr_t)(12 * cap);
        const uintptr_t b0 = reinterpret_cast<uintptr_t>(status), b1 = b0 + (uintptr_t)cap;
        if (a0 < b1 && b0 < a1) return "normals_out and status overlap each other";
    }
    return nullptr;
}
