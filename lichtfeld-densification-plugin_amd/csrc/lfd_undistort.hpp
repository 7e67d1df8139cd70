// Image undistortion in front of everything else (lfd_undistort_image): what the kernel (lfd_undistort.hip) and the twin
// (lfd_host.hip) share - the camera model, the validity test and the blend of one output pixel, and the checks of a call's arguments.
//
// COLMAP's SIMPLE_RADIAL, RADIAL, OPENCV and FULL_OPENCV are one formula with eight coefficients d = (k1, k2, p1, p2, k3, k4, k5, k6).  The
// output is the pinhole image of the same (fx, fy, cx, cy): output pixel (i, j), its centre at +0.5 (COLMAP's convention), is sent through
// the model to where the photograph shows it and sampled there.  All in f64, every rounding written out and nothing contracted (the build
// uses -ffp-contract=off), + - * / and floor only: device, twin and a NumPy reference agree byte for byte.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/lfd_densify.h"

#if defined(__HIPCC__)
#define LFD_HD __host__ __device__ __forceinline__
#else
#define LFD_HD inline
#endif

struct LfdUndistortArgs {
    const uint8_t* src;
    uint8_t* dst;
    uint8_t* valid255;           // or null
    int32_t w, h, channels, nearest;
    double fx, fy, cx, cy;
    double k1, k2, p1, p2, k3, k4, k5, k6;
};

// Where output pixel (i, j) lies in the source image, in pixel-index coordinates (su, sv); false when that is outside the half-pixel border
// of the image or not a number (a zero denominator included).
LFD_HD bool lfd_undistort_source(const LfdUndistortArgs& p, int i, int j, double& su, double& sv) {
    const double x = (((double)j + 0.5) - p.cx) / p.fx;
    const double y = (((double)i + 0.5) - p.cy) / p.fy;
    const double xx = x * x, yy = y * y;
    const double r2 = xx + yy;
    const double r4 = r2 * r2;
    const double r6 = r4 * r2;
    const double xy = x * y;
    const double num = ((1.0 + p.k1 * r2) + p.k2 * r4) + p.k3 * r6;
    const double den = ((1.0 + p.k4 * r2) + p.k5 * r4) + p.k6 * r6;
    const double rad = num / den;
    const double xd = (x * rad + (2.0 * p.p1) * xy) + p.p2 * (r2 + 2.0 * xx);
    const double yd = (y * rad + (2.0 * p.p2) * xy) + p.p1 * (r2 + 2.0 * yy);
    su = (p.fx * xd + p.cx) - 0.5;
    sv = (p.fy * yd + p.cy) - 0.5;
    return su >= -0.5 && su <= (double)p.w - 0.5 && sv >= -0.5 && sv <= (double)p.h - 0.5;          // a NaN fails every comparison
}

LFD_HD int lfd_undistort_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// Output pixel (i, j), 0 <= i < h, 0 <= j < w: writes its `channels` bytes and its validity byte; returns whether it is valid.  No
// floating-point value is converted to an integer before the validity test has passed.
LFD_HD bool lfd_undistort_pixel(const LfdUndistortArgs& p, int i, int j) {
    double su, sv;
    const bool valid = lfd_undistort_source(p, i, j, su, sv);
    const size_t o = (size_t)i * (size_t)p.w + (size_t)j;
    if (p.valid255) p.valid255[o] = valid ? 255 : 0;
    uint8_t* d = p.dst + o * (size_t)p.channels;
    if (!valid) {
        for (int c = 0; c < p.channels; ++c) d[c] = 0;
        return false;
    }
    const int ch = p.channels;
    if (p.nearest) {
        const int xs = lfd_undistort_clamp((int)floor(su + 0.5), p.w - 1);
        const int ys = lfd_undistort_clamp((int)floor(sv + 0.5), p.h - 1);
        const uint8_t* s = p.src + ((size_t)ys * (size_t)p.w + (size_t)xs) * (size_t)ch;
        for (int c = 0; c < ch; ++c) d[c] = s[c];
        return true;
    }
    const double fx0 = floor(su), fy0 = floor(sv);
    const double ax = su - fx0, ay = sv - fy0;
    const int x0 = (int)fx0, y0 = (int)fy0;
    const int xa = lfd_undistort_clamp(x0, p.w - 1), xb = lfd_undistort_clamp(x0 + 1, p.w - 1);       // edge replication inside the border
    const int ya = lfd_undistort_clamp(y0, p.h - 1), yb = lfd_undistort_clamp(y0 + 1, p.h - 1);
    const uint8_t* r0 = p.src + (size_t)ya * (size_t)p.w * (size_t)ch;
    const uint8_t* r1 = p.src + (size_t)yb * (size_t)p.w * (size_t)ch;
    for (int c = 0; c < ch; ++c) {
        const double p00 = (double)r0[(size_t)xa * ch + c], p01 = (double)r0[(size_t)xb * ch + c];
        const double p10 = (double)r1[(size_t)xa * ch + c], p11 = (double)r1[(size_t)xb * ch + c];
        const double top = p00 + ax * (p01 - p00);
        const double bot = p10 + ax * (p11 - p10);
        const double val = top + ay * (bot - top);
        d[c] = (uint8_t)(int)floor(val + 0.5);               // within [0, 255]: ax, ay are in [0, 1)
    }
    return true;
}

// What is wrong with the arguments of lfd_undistort_image / lfd_host_undistort_image (the context apart), or null.
inline const char* lfd_undistort_check(const uint8_t* src, int32_t w, int32_t h, int32_t channels, const double* intr, const double* dist,
                                       const uint8_t* dst, const uint8_t* valid255) {
    if (!src || !dst || !intr || !dist) return "null src / dst / intr / dist";
    if (w < 1 || h < 1 || (long long)w * (long long)h > 0x7fffffffLL) return "w and h must be >= 1 and w * h at most 2^31 - 1";
    if (channels != 1 && channels != 3) return "channels must be 1 or 3";
    if (!__builtin_isfinite(intr[0]) || !__builtin_isfinite(intr[1]) || !(intr[0] > 0.0) || !(intr[1] > 0.0)) return "fx and fy must be finite and > 0";
    if (!__builtin_isfinite(intr[2]) || !__builtin_isfinite(intr[3])) return "cx and cy must be finite";
    for (int e = 0; e < 8; ++e)
        if (!__builtin_isfinite(dist[e])) return "the distortion coefficients must be finite";
    const uintptr_t px = (uintptr_t)w * (uintptr_t)h;
    const struct { const void* p; uintptr_t bytes; } a[3] = {{src, px * (uintptr_t)channels}, {dst, px * (uintptr_t)channels}, {valid255, px}};
    for (int i = 0; i < 3; ++i)
        for (int j = i + 1; j < 3; ++j) {
            if (!a[i].p || !a[j].p) continue;
            const uintptr_t a0 = reinterpret_cast<uintptr_t>(a[i].p), b0 = reinterpret_cast<uintptr_t>(a[j].p);
            if (a0 < b0 + a[j].bytes && b0 < a0 + a[i].bytes) return "src, dst and valid255 must not overlap";
        }
    return nullptr;
}

inline LfdUndistortArgs lfd_undistort_args(const uint8_t* src, int32_t w, int32_t h, int32_t channels, int32_t nearest, const double* intr,
                                           const double* dist, uint8_t* dst, uint8_t* valid255) {
    LfdUndistortArgs p;
    p.src = src; p.dst = dst; p.valid255 = valid255;
    p.w = w; p.h = h; p.channels = channels; p.nearest = nearest ? 1 : 0;
    p.fx = intr[0]; p.fy = intr[1]; p.cx = intr[2]; p.cy = intr[3];
    p.k1 = dist[0]; p.k2 = dist[1]; p.p1 = dist[2]; p.p2 = dist[3]; p.k3 = dist[4]; p.k4 = dist[5]; p.k5 = dist[6]; p.k6 = dist[7];
    return p;
}
