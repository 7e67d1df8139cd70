// Free-space filter on the final cloud (lfd_freespace_filter): what the kernels (lfd_freespace.hip) and the twin (lfd_host.hip)
// share - the projection of a point into a reference's camera, the judgement of one reference about one point, the keep decision and the checks
// of a call's arguments.
//
// Every reference's own points are a sparse depth map of what it saw: Z_r[cell] is the smallest depth of r's own points in that cell of a
// pw x ph plane over r's image.  A point of ANOTHER reference that projects into r's image is supported by r when a cell of the 3 x 3 window
// around it holds a depth within tol of the point's, refuted when the point lies in front of everything r saw in that window, and otherwise
// left alone (occluded or unobserved).  The projection is f64 from the f32 inputs with every sum written out; the depth test is f32 with every
// rounding written out; nothing is contracted (the build uses -ffp-contract=off).  Positive finite f32 order like their bit patterns, so a
// z-buffer is a plane of u32 words and its minimum is one integer minimum: the result does not depend on the order of the points.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/lfd_densify.h"

#if defined(__HIPCC__)
#define LFD_HD __host__ __device__ __forceinline__
#else
#define LFD_HD inline
#endif

#define LFD_FREESPACE_EMPTY 0x7f800000u        // the bits of +inf: a cell nobody wrote; every finite positive depth is below it

// One reference's camera as the kernels read it: the 12 f32 entries of P widened (exactly) to f64 and the image size, 14 values.
struct LfdFreespaceCam {
    double P[12];
    double w, h;
};

LFD_HD void lfd_freespace_cam(const float* P, int32_t w, int32_t h, LfdFreespaceCam& c) {
    for (int e = 0; e < 12; ++e) c.P[e] = (double)P[e];
    c.w = (double)w;
    c.h = (double)h;
}

LFD_HD bool lfd_freespace_finite(double v) { return v - v == 0.0; }      // false for NaN and both infinities

// Point (x, y, z) in camera c.  True iff the point is inside: the three sums finite, p_2 > 0, 0 <= u < w, 0 <= v < h and the f32 depth finite
// and > 0; then (cx, cy) is its cell of the pw x ph plane and d its depth.  Nothing is written for a point outside.
LFD_HD bool lfd_freespace_project(const LfdFreespaceCam& c, double pw, double ph, float x, float y, float z, int& cx, int& cy, float& d) {
    const double X = (double)x, Y = (double)y, Z = (double)z;
    const double a0 = c.P[0] * X, a1 = c.P[1] * Y, a2 = c.P[2] * Z;          // (products of two widened f32: exact)
    const double b0 = c.P[4] * X, b1 = c.P[5] * Y, b2 = c.P[6] * Z;
    const double c0 = c.P[8] * X, c1 = c.P[9] * Y, c2 = c.P[10] * Z;
    const double s0 = a0 + a1, s1 = b0 + b1, s2 = c0 + c1;
    const double t0 = s0 + a2, t1 = s1 + b2, t2 = s2 + c2;
    const double p0 = t0 + c.P[3], p1 = t1 + c.P[7], p2 = t2 + c.P[11];
    if (!(lfd_freespace_finite(p0) && lfd_freespace_finite(p1) && lfd_freespace_finite(p2)) || !(p2 > 0.0)) return false;
    const double u = p0 / p2, v = p1 / p2;
    if (!(u >= 0.0 && u < c.w && v >= 0.0 && v < c.h)) return false;
    const float df = (float)p2;
    if (!(df > 0.0f) || !(df <= 3.4028234e38f)) return false;
    const double gu = u * pw, gv = v * ph;
    const double fx = floor(gu / c.w), fy = floor(gv / c.h);
    const double mx = pw - 1.0, my = ph - 1.0;
    cx = (int)(fx < mx ? fx : mx);
    cy = (int)(fy < my ? fy : my);
    d = df;
    return true;
}

#define LFD_FREESPACE_SILENT 0
#define LFD_FREESPACE_SUPPORT 1
#define LFD_FREESPACE_REFUTE 2

// What the reference whose z-buffer is `plane` (pw x ph words) says about a point at cell (cx, cy) with depth d (finite, > 0): support when a
// cell of the 3 x 3 window (the part of it inside the plane) holds a finite D with D - tol D <= d <= D + tol D, else refutation when the window
// holds a finite cell and d < D_min - tol D_min for the smallest one, else nothing.
LFD_HD int lfd_freespace_judge(const uint32_t* plane, int pw, int ph, int cx, int cy, float d, float tol) {
    uint32_t dmin = LFD_FREESPACE_EMPTY;
    bool support = false;
    for (int dy = -1; dy <= 1; ++dy) {
        const int yy = cy + dy;
        if (yy < 0 || yy >= ph) continue;
        const uint32_t* row = plane + (long long)yy * pw;
        for (int dx = -1; dx <= 1; ++dx) {
            const int xx = cx + dx;
            if (xx < 0 || xx >= pw) continue;
            const uint32_t bits = row[xx];
            if (bits >= LFD_FREESPACE_EMPTY) continue;                       // +inf: nobody there (the planes hold nothing else above it)
            float D;
            __builtin_memcpy(&D, &bits, 4);
            const float t = tol * D;
            const float lo = D - t, hi = D + t;
            support = support || (lo <= d && d <= hi);
            dmin = bits < dmin ? bits : dmin;
        }
    }
    if (support) return LFD_FREESPACE_SUPPORT;
    if (dmin >= LFD_FREESPACE_EMPTY) return LFD_FREESPACE_SILENT;
    float D;
    __builtin_memcpy(&D, &dmin, 4);
    const float t = tol * D;
    const float lo = D - t;
    return d < lo ? LFD_FREESPACE_REFUTE : LFD_FREESPACE_SILENT;
}

// The two counts of a point of reference `own`: every other reference in which it is inside judges it.  cams: n_refs cameras, zbuf: n_refs planes.
LFD_HD void lfd_freespace_count_point(const LfdFreespaceCam* cams, const uint32_t* zbuf, int n_refs, int own, int pw, int ph, float x, float y,
                                      float z, float tol, int& violations, int& supports) {
    const double dpw = (double)pw, dph = (double)ph;
    const long long plane = (long long)pw * ph;
    int v = 0, s = 0;
    for (int j = 0; j < n_refs; ++j) {
        if (j == own) continue;
        int cx, cy;
        float d;
        if (!lfd_freespace_project(cams[j], dpw, dph, x, y, z, cx, cy, d)) continue;
        const int say = lfd_freespace_judge(zbuf + (long long)j * plane, pw, ph, cx, cy, d, tol);
        v += say == LFD_FREESPACE_REFUTE ? 1 : 0;
        s += say == LFD_FREESPACE_SUPPORT ? 1 : 0;
    }
    violations = v;
    supports = s;
}

// dropped iff at least min_violations references refute the point and more refute than support it (the unsaturated counts)
LFD_HD bool lfd_freespace_keep(int violations, int supports, int min_violations) { return !(violations >= min_violations && violations > supports); }

LFD_HD uint8_t lfd_freespace_u8(int c) { return (uint8_t)(c > 255 ? 255 : c); }

// What is wrong with the arguments of lfd_freespace_filter / lfd_freespace_filter_host (the context apart), or null.
inline const char* lfd_freespace_check(const float* xyz, const float* rgb, const float* err, int64_t n, const int64_t* offs, int32_t n_refs,
                                       const float* cam_P, const int32_t* cam_wh, int32_t pw, int32_t ph, float tol, int32_t min_violations,
                                       const float* xyz_out, const float* rgb_out, const float* err_out, const int64_t* offs_out,
                                       const uint8_t* violations, const uint8_t* supports, const int64_t* n_out) {
    if (!offs || !offs_out || !n_out) return "null ref_offsets_host / ref_offsets_out_host / n_out_host";
    if (!cam_P || !cam_wh) return "null cam_P_host / cam_wh_host";
    if (n < 0 || n > 0x7fffffffLL) return "n must be in [0, 2^31 - 1]";
    if (n_refs < 1) return "n_refs must be >= 1";
    if (n > 0 && (!xyz || !xyz_out)) return "null xyz / xyz_out";
    if ((rgb == nullptr) != (rgb_out == nullptr) || (err == nullptr) != (err_out == nullptr)) return "rgb / rgb_out and err / err_out must both be given or both be null";
    if (offs[0] != 0 || offs[n_refs] != n) return "ref_offsets_host must start at 0 and end at n";
    for (int32_t r = 0; r < n_refs; ++r)
        if (offs[r + 1] < offs[r]) return "ref_offsets_host must not decrease";
    if (pw < 1 || ph < 1) return "the z-buffer plane pw x ph must be at least 1 x 1";
    if ((long long)n_refs * (long long)pw > 0x7fffffffLL || (long long)n_refs * (long long)pw * (long long)ph > 0x7fffffffLL)
        return "n_refs * pw * ph must be at most 2^31 - 1 z-buffer cells";
    for (int32_t r = 0; r < n_refs; ++r) {
        if (cam_wh[2 * r] < 1 || cam_wh[2 * r + 1] < 1) return "a camera's image size w, h must be at least 1 x 1";
        for (int e = 0; e < 12; ++e)
            if (!(cam_P[12 * r + e] - cam_P[12 * r + e] == 0.0f)) return "a camera's P has an entry that is not finite";
    }
    if (!(tol > 0.0f) || !(tol < 1.0f)) return "tol must be in (0, 1)";
    if (min_violations < 1 || min_violations > 255) return "min_violations must be in [1, 255]";
    const struct { const void* p; long long elem; } a[3] = {{xyz, 12}, {rgb, 12}, {err, 4}},
                                                    b[5] = {{xyz_out, 12}, {rgb_out, 12}, {err_out, 4}, {violations, 1}, {supports, 1}};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 5; ++j) {
            if (!a[i].p || !b[j].p) continue;
            const uintptr_t a0 = reinterpret_cast<uintptr_t>(a[i].p), a1 = a0 + (uintptr_t)(a[i].elem * n);
            const uintptr_t b0 = reinterpret_cast<uintptr_t>(b[j].p), b1 = b0 + (uintptr_t)(b[j].elem * n);
            if (a0 < b1 && b0 < a1) return "in and out arrays overlap";
        }
    return nullptr;
}
