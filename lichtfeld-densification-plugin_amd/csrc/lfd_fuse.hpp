// Oriented voxel fusion (lfd_fuse_oriented): what the kernels (lfd_fuse.hip) and the twin (lfd_host.hip) share - the usable-normal
// test, the side of a point, the per-side sums and what a row is made of, the grid of a call and the checks of its arguments.
//
// The points of a voxel are merged per SIDE: side 1 holds the points whose usable normal has a negative dot product with the voxel's pivot - the
// usable normal of its point with the lowest input index -, side 0 everything else.  Every rounding is written out and nothing is contracted (the
// build uses -ffp-contract=off): the products of two f32 values are exact in f64, so only the additions round.  Grid, keys, voxel order and colour
// scale are lfd_voxel_downsample's: lfd_fuse_grid and lfd_fuse_cscale below are the one statement of that arithmetic, used by both device entry
// points (lfd_api.hip) and by the twin (lfd_host.hip).
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/lfd_densify.h"
#if defined(__HIPCC__)
#include "lfd_geometry.hpp"      // lfd_sqrt_rare, lfd_recip_refined
#endif

#if !defined(LFD_HD)
#if defined(__HIPCC__)
#define LFD_HD __host__ __device__ __forceinline__
#else
#define LFD_HD inline
#endif
#endif

#define LFD_FUSE_SIDE 1u         /* flag byte of a sorted point: its side ... */
#define LFD_FUSE_USABLE 2u       /* ... and whether its normal is usable (takes part in N) */

LFD_HD bool lfd_fuse_usable(float n0, float n1, float n2) {
    if (!(__builtin_isfinite(n0) && __builtin_isfinite(n1) && __builtin_isfinite(n2))) return false;
    const double a = (double)n0 * (double)n0, b = (double)n1 * (double)n1, c = (double)n2 * (double)n2;
    const double ab = a + b;
    return ab + c > 0.0;
}

// the flag byte of a point with normal n in a voxel whose pivot is p (has_pivot: the voxel has one so far)
LFD_HD unsigned lfd_fuse_flag(const float* n, bool has_pivot, const float* p) {
    if (!lfd_fuse_usable(n[0], n[1], n[2])) return 0u;
    if (!has_pivot) return LFD_FUSE_USABLE;                     // this point is the pivot: d = n . n > 0
    const double a = (double)n[0] * (double)p[0], b = (double)n[1] * (double)p[1], c = (double)n[2] * (double)p[2];
    const double ab = a + b;
    const double d = ab + c;
    return LFD_FUSE_USABLE | (d < 0.0 ? LFD_FUSE_SIDE : 0u);
}

struct LfdFuseAcc {              // one side of one voxel
    double p[3], c[3], N[3];
    unsigned cnt;
};

LFD_HD void lfd_fuse_clear(LfdFuseAcc& a) {
    for (int e = 0; e < 3; ++e) { a.p[e] = 0.0; a.c[e] = 0.0; a.N[e] = 0.0; }
    a.cnt = 0u;
}

// x, n, rgb: the point's three floats each
LFD_HD void lfd_fuse_add(LfdFuseAcc& a, const float* x, const float* n, const float* rgb, bool usable, double cscale) {
    for (int e = 0; e < 3; ++e) {
        a.p[e] = a.p[e] + (double)x[e];
        a.c[e] = a.c[e] + (double)rgb[e] / cscale;
    }
    if (usable)
        for (int e = 0; e < 3; ++e) a.N[e] = a.N[e] + (double)n[e];
    a.cnt += 1u;
}

// N / |N| rounded to f32 once per component; zeros where N . N is not finite or not > 0.  The device divides through a refined reciprocal
// (components within one f32 ulp of the host's), as lfd_normal_unit does.
LFD_HD void lfd_fuse_unit(double N0, double N1, double N2, float* out) {
    const double q = (N0 * N0 + N1 * N1) + N2 * N2;
    out[0] = 0.0f; out[1] = 0.0f; out[2] = 0.0f;
    if (!(q > 0.0) || !(q <= 1.7976931348623157e308)) return;
#if defined(__HIP_DEVICE_COMPILE__)
    const double r = lfd_recip_refined(lfd_sqrt_rare(q));
    out[0] = (float)(N0 * r); out[1] = (float)(N1 * r); out[2] = (float)(N2 * r);
#else
    const double l = sqrt(q);
    out[0] = (float)(N0 / l); out[1] = (float)(N1 / l); out[2] = (float)(N2 / l);
#endif
}

// one output row from one side's sums (cnt >= 1)
LFD_HD void lfd_fuse_emit(const LfdFuseAcc& a, float* xyz_out, float* nrm_out, float* rgb_out) {
    const double cnt = (double)a.cnt;
    for (int e = 0; e < 3; ++e) {
        xyz_out[e] = (float)(a.p[e] / cnt);
        rgb_out[e] = (float)(a.c[e] / cnt);
    }
    lfd_fuse_unit(a.N[0], a.N[1], a.N[2], nrm_out);
}

// linear voxel key of a point (lfd_voxel_keys_kernel's expression)
LFD_HD unsigned long long lfd_fuse_key(float x, float y, float z, double o0, double o1, double o2, double h, unsigned long long e1,
                                       unsigned long long e2) {
    const double k0 = floor(((double)x - o0) / h);
    const double k1 = floor(((double)y - o1) / h);
    const double k2 = floor(((double)z - o2) / h);
    return ((unsigned long long)k0 * e1 + (unsigned long long)k1) * e2 + (unsigned long long)k2;
}

struct LfdFuseGrid {
    double origin[3];
    unsigned long long e[3];     // extents E_c = max key_c + 1
    int bits;                    // significant bits of the largest linear key: what the radix sort has to look at
};

// The grid of a call from the min / max of its (finite) coordinates, as lfd_voxel_downsample derives it.  False: the linear key leaves 63 bits.
inline bool lfd_fuse_grid(const float* lo, const float* hi, double h, LfdFuseGrid& g) {
    for (int c = 0; c < 3; ++c) {
        g.origin[c] = (double)lo[c] - 0.5 * h;
        const double kmax = floor(((double)hi[c] - g.origin[c]) / h);           // the key is monotone in the coordinate
        if (!(kmax < 9223372036854775808.0)) return false;
        g.e[c] = (unsigned long long)kmax + 1ull;
    }
    unsigned __int128 cells = (unsigned __int128)g.e[0] * g.e[1];               // every E_c <= 2^63: neither product overflows 128 bits
    if (cells <= ((unsigned __int128)1 << 63)) cells *= g.e[2];
    if (cells > ((unsigned __int128)1 << 63)) return false;
    const unsigned long long max_key = (unsigned long long)cells - 1ull;
    g.bits = max_key ? 64 - __builtin_clzll(max_key) : 0;
    return true;
}

// colour scale from the colour maximum over the non-NaN values and whether a NaN was seen (NumPy's `rgb.max() > 1.0`)
inline double lfd_fuse_cscale(float cmax, bool any_nan) { return any_nan ? 1.0 : ((double)cmax > 1.0 ? 255.0 : 1.0); }

#define LFD_FUSE_NONFINITE "non-finite coordinate in the input"
#define LFD_FUSE_KEY_RANGE "key range: the linear voxel key does not fit 63 bits"

// What is wrong with the arguments of lfd_fuse_oriented / lfd_fuse_oriented_host (the context apart), or null.
inline const char* lfd_fuse_check(const float* xyz, const float* normals, const float* rgb, int64_t n, double voxel_size, const float* xyz_out,
                                  const float* normals_out, const float* rgb_out, const uint32_t* count_out, const int64_t* n_rows,
                                  const int64_t* n_voxels) {
    if (!n_rows || !n_voxels) return "null n_rows_host / n_voxels_host";
    if (n < 0 || n > 0x7fffffffLL) return "n must be in [0, 2^31 - 1]";
    if (!(voxel_size > 0.0) || !(voxel_size <= 1.7976931348623157e308)) return "voxel_size must be finite and > 0";
    if (n > 0 && (!xyz || !normals || !rgb)) return "null xyz / normals / rgb";
    if (n > 0 && (!xyz_out || !normals_out || !rgb_out)) return "null xyz_out / normals_out / rgb_out";
    const struct { const void* p; long long elem; } a[7] = {{xyz, 12}, {normals, 12}, {rgb, 12}, {xyz_out, 12}, {normals_out, 12}, {rgb_out, 12},
                                                            {count_out, 4}};
    for (int j = 3; j < 7; ++j)
        for (int i = 0; i < j; ++i) {
            if (!a[i].p || !a[j].p) continue;
            const uintptr_t a0 = reinterpret_cast<uintptr_t>(a[i].p), a1 = a0 + (uintptr_t)(a[i].elem * n);
            const uintptr_t b0 = reinterpret_cast<uintptr_t>(a[j].p), b1 = b0 + (uintptr_t)(a[j].elem * n);
            if (a0 < b1 && b0 < a1) return i < 3 ? "in and out arrays overlap" : "out arrays overlap each other";
        }
    return nullptr;
}
