// Gaussian-ready output (lfd_knn_dist2, lfd_pack_gaussians): what the kernels (lfd_knn.hip) and the twin (lfd_host.hip) share - the
// f32 distance, the best-three update, the grid of a call with its stop bounds, the ring scan of one point, the 68-byte record and the checks of
// the arguments.
//
// dist2[i] = ((a + b) + c) / 3.0f over the three smallest d2(i, j), j != i by INDEX (a duplicate counts with distance 0), where
// d2 = (dx dx + dy dy) + dz dz in f32, every rounding written out and nothing contracted (the build uses -ffp-contract=off): the arithmetic of
// lfd_consensus_agree.  Only values enter, so ties need no rule, and the result does not depend on the grid: it is what a brute-force loop over all
// pairs gives, bit for bit.
//
// Neighbours are found through a grid of cells of side h whose linear keys are sorted.  A point scans the cells of Chebyshev ring 1, 2, ..
// LFD_KNN_RMAX around its own and stops behind ring r once its third-best d2 is at most bound(r), a value no unscanned point can undercut
// (lfd_knn_grid derives it); a point that has not stopped behind the last ring is finished by brute force over the whole cloud.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/lfd_densify.h"

#if !defined(LFD_HD)
#if defined(__HIPCC__)
#define LFD_HD __host__ __device__ __forceinline__
#else
#define LFD_HD inline
#endif
#endif

#define LFD_KNN_RMAX 3                           /* rings a point scans before it is handed to the brute-force pass */
#define LFD_KNN_MAX_AXIS 1073741824.0            /* 2^30 cells per axis: lfd_consensus_grid's limit, for the same reason (f64 roundings of a key) */
#define LFD_KNN_REFINE_DENSITY 16                /* automatic cell size: refined while points / occupied cells exceeds this ... */
#define LFD_KNN_REFINE_MAX 8                     /* ... at most this many times, h / 4 each time */

struct LfdKnnPt {                // one point of the cloud in cell order: a candidate costs the scan one 16-byte load
    float x, y, z;
    uint32_t idx;                // its input index
};

LFD_HD float lfd_knn_d2(float xi, float yi, float zi, float xj, float yj, float zj) {
    const float dx = xi - xj, dy = yi - yj, dz = zi - zj;
    const float sx = dx * dx, sy = dy * dy, sz = dz * dz;
    const float sxy = sx + sy;
    return sxy + sz;
}

// d into the ascending triple (a, b, c) of the smallest values so far (no NaN reaches this: the coordinates are finite)
LFD_HD void lfd_knn_insert(float d, float& a, float& b, float& c) {
    const float nc = d < c ? (d < b ? b : d) : c;
    const float nb = d < b ? (d < a ? a : d) : b;
    const float na = d < a ? d : a;
    a = na; b = nb; c = nc;
}

LFD_HD float lfd_knn_mean(float a, float b, float c) {
    const float ab = a + b;
    const float s = ab + c;
    return s / 3.0f;
}

struct LfdKnnGrid {
    double origin[3], h;
    unsigned long long e[3];     // extents E_c = max cell_c + 1
    int bits;                    // significant bits of the largest linear key: what the radix sort has to look at
    float bound1, bound2, bound3;    // bound(r): no point outside rings 0 .. r has an f32 d2 below it
};

LFD_HD float lfd_knn_bound(const LfdKnnGrid& g, int r) { return r == 1 ? g.bound1 : (r == 2 ? g.bound2 : g.bound3); }

// cell of a coordinate: floor(((f64) x - origin) / h), IEEE subtract and divide; >= 0 and < E_c for every point of the call
LFD_HD long long lfd_knn_cell(float x, double o, double h) { return (long long)floor(((double)x - o) / h); }

LFD_HD unsigned long long lfd_knn_key(float x, float y, float z, const LfdKnnGrid& g) {
    const unsigned long long k0 = (unsigned long long)lfd_knn_cell(x, g.origin[0], g.h), k1 = (unsigned long long)lfd_knn_cell(y, g.origin[1], g.h),
                             k2 = (unsigned long long)lfd_knn_cell(z, g.origin[2], g.h);
    return (k0 * g.e[1] + k1) * g.e[2] + k2;
}

// every point but the one at sorted position j whose key lies in [lo, hi] - one row range of cells - into the triple: one binary search, then a walk
LFD_HD void lfd_knn_walk(const unsigned long long* skey, const LfdKnnPt* spt, long long n, long long j, const LfdKnnPt& me, unsigned long long lo,
                         unsigned long long hi, float& a, float& b, float& c) {
    long long l = 0, h = n;
    while (l < h) {
        const long long mid = (l + h) >> 1;
        if (skey[mid] < lo) l = mid + 1; else h = mid;
    }
    for (long long q = l; q < n; ++q) {
        if (skey[q] > hi) break;
        if (q == j) continue;
        const LfdKnnPt p = spt[q];
        lfd_knn_insert(lfd_knn_d2(me.x, me.y, me.z, p.x, p.y, p.z), a, b, c);
    }
}

// The point at sorted position j: ring after ring until the stop bound holds.  True: *mean is its result.  False: LFD_KNN_RMAX rings did not
// settle it.  Ring 1 is the nine rows (k0 + a, k1 + b) with the cells k2 - 1 .. k2 + 1 as one key range each; ring r > 1 is the shell only: the
// full range k2 - r .. k2 + r in the rows with max(|a|, |b|) = r, the two end cells in the inner rows.  Rows and cells outside the grid are left out.
LFD_HD bool lfd_knn_scan_point(const unsigned long long* skey, const LfdKnnPt* spt, long long n, long long j, const LfdKnnGrid& g, float* mean) {
    const LfdKnnPt me = spt[j];
    const long long k0 = lfd_knn_cell(me.x, g.origin[0], g.h), k1 = lfd_knn_cell(me.y, g.origin[1], g.h), k2 = lfd_knn_cell(me.z, g.origin[2], g.h);
    const long long E0 = (long long)g.e[0], E1 = (long long)g.e[1], E2 = (long long)g.e[2];
    float a = INFINITY, b = INFINITY, c = INFINITY;
    for (int r = 1; r <= LFD_KNN_RMAX; ++r) {
        for (int da = -r; da <= r; ++da) {
            const long long K0 = k0 + da;
            if (K0 < 0 || K0 >= E0) continue;
            for (int db = -r; db <= r; ++db) {
                const long long K1 = k1 + db;
                if (K1 < 0 || K1 >= E1) continue;
                const unsigned long long base = ((unsigned long long)K0 * (unsigned long long)E1 + (unsigned long long)K1) * (unsigned long long)E2;
                const long long z0 = k2 - r, z1 = k2 + r;
                if (r == 1 || da == -r || da == r || db == -r || db == r) {
                    lfd_knn_walk(skey, spt, n, j, me, base + (unsigned long long)(z0 < 0 ? 0 : z0), base + (unsigned long long)(z1 >= E2 ? E2 - 1 : z1),
                                 a, b, c);
                } else {
                    if (z0 >= 0) lfd_knn_walk(skey, spt, n, j, me, base + (unsigned long long)z0, base + (unsigned long long)z0, a, b, c);
                    if (z1 < E2) lfd_knn_walk(skey, spt, n, j, me, base + (unsigned long long)z1, base + (unsigned long long)z1, a, b, c);
                }
            }
        }
        if (c <= lfd_knn_bound(g, r)) {
            *mean = lfd_knn_mean(a, b, c);
            return true;
        }
    }
    return false;
}

// The largest f32 that is <= (r h)^2 (1 - 2^-19) - 2^-148, or 0 where that is not positive.  A point outside rings 0 .. r lies r + 1 or more cells
// from the scanning point along some axis; the two scaled coordinates carry two f64 roundings each (below 2^-22 cells while they are below 2^30),
// so the true distance along that axis exceeds r h (1 - 2^-20.9); the f32 difference, its square (2^-24 relative each, 2^-150 absolute where the
// square is subnormal) and two additions of non-negative values (monotone) leave d2 > (r h)^2 (1 - 2^-19.8) - 2^-150.
inline float lfd_knn_stop_bound(int r, double h) {
    const double rh = (double)r * h;
    const double bd = rh * rh * (1.0 - 0x1p-19) - 0x1p-148;
    if (!(bd > 0.0)) return 0.0f;                // (a third-best d2 of 0 stops a point anyway: no d2 is negative)
    float bf = bd >= 3.4028234663852886e38 ? 3.4028234663852886e38f : (float)bd;
    if ((double)bf > bd) bf = nextafterf(bf, 0.0f);
    return bf;
}

// The grid of a call from the min / max of its (finite) coordinates.  False: more than 2^30 cells along an axis, or a linear key beyond 63 bits.
inline bool lfd_knn_grid(const float* lo, const float* hi, double h, LfdKnnGrid& g) {
    static_assert(LFD_KNN_RMAX == 3, "lfd_knn_bound names three bounds");
    g.h = h;
    for (int c = 0; c < 3; ++c) {
        g.origin[c] = (double)lo[c];
        const double kmax = floor(((double)hi[c] - g.origin[c]) / h);               // the cell is monotone in the coordinate
        if (!(kmax < LFD_KNN_MAX_AXIS)) return false;
        g.e[c] = (unsigned long long)kmax + 1ull;
    }
    const unsigned __int128 cells = (unsigned __int128)g.e[0] * g.e[1] * g.e[2];    // < 2^91
    if (cells > ((unsigned __int128)1 << 63)) return false;
    const unsigned long long max_key = (unsigned long long)cells - 1ull;
    g.bits = max_key ? 64 - __builtin_clzll(max_key) : 0;
    g.bound1 = lfd_knn_stop_bound(1, h);
    g.bound2 = lfd_knn_stop_bound(2, h);
    g.bound3 = lfd_knn_stop_bound(3, h);
    return true;
}

// The automatic cell size's first guess: 2 L / ceil(sqrt(n)), L the longest side of the bounding box - the spacing of n points spread over a
// surface of that extent, doubled; 1 where the box has no extent.  f64 on the host, the same for device and twin.
inline double lfd_knn_auto_h(const float* lo, const float* hi, long long n) {
    double L = 0.0;
    for (int c = 0; c < 3; ++c) L = fmax(L, (double)hi[c] - (double)lo[c]);
    if (!(L > 0.0)) return 1.0;
    const double h = 2.0 * L / ceil(sqrt((double)n));
    return h > 0.0 ? h : 1.0;                    // (a box so small that the quotient underflows)
}

// whether the automatic rule goes on refining behind a grid with `occupied` cells; far outliers inflate the box and put a whole cloud into one cell
inline bool lfd_knn_refine_more(long long n, long long occupied, int rebuilds) {
    return rebuilds < LFD_KNN_REFINE_MAX && n > (long long)LFD_KNN_REFINE_DENSITY * occupied;
}

#define LFD_KNN_TOO_FEW "fewer than four points: a point has no three neighbours"
#define LFD_KNN_NONFINITE "non-finite coordinate in the input"
#define LFD_KNN_KEY_RANGE "key range: more than 2^30 cells along an axis or a linear cell key beyond 63 bits"

// What is wrong with the arguments of lfd_knn_dist2 / lfd_knn_dist2_host (the context apart), or null.
inline const char* lfd_knn_check(const float* xyz, int64_t n, double cell_size, const float* dist2_out) {
    if (n < 0 || n > 0x7fffffffLL) return "n must be in [0, 2^31 - 1]";
    if (!(cell_size >= 0.0) || !(cell_size <= 1.7976931348623157e308)) return "cell_size must be finite and >= 0 (0 = automatic)";
    if (n > 0 && (!xyz || !dist2_out)) return "null xyz / dist2_out";
    if (n >= 1 && n <= 3) return LFD_KNN_TOO_FEW;
    if (n > 0) {
        const uintptr_t a0 = reinterpret_cast<uintptr_t>(xyz), a1 = a0 + (uintptr_t)(12 * n);
        const uintptr_t b0 = reinterpret_cast<uintptr_t>(dist2_out), b1 = b0 + (uintptr_t)(4 * n);
        if (a0 < b1 && b0 < a1) return "in and out arrays overlap";
    }
    return nullptr;
}

// ---- the 68-byte record of lfd_pack_gaussians: x y z nx ny nz f_dc_0..2 opacity scale_0..2 rot_0..3, 17 f32 -----------------------------------
#define LFD_GAUSS_FLOATS 17
#define LFD_GAUSS_SH_C0 0.28209479177387814f
#define LFD_GAUSS_MIN_DIST2 1e-7f                /* the 3DGS clamp of the mean squared distance */
#define LFD_GAUSS_FLIP_BELOW 1.1920929e-7f       /* 2^-23: 1 + nz below it (0 or 2^-24 for a unit normal) means the normal is -z */

// the u8 the 27-byte writer stores for a colour (lfd_quantise_u8 / to_uint8_rgb: f32 product, round half to even, clipped, NaN -> 0)
LFD_HD float lfd_gauss_u8(float c) {
    const float v = rintf(c * 255.0f);
    if (!(v == v)) return 0.0f;
    return v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);
}

LFD_HD float lfd_gauss_dc(float c) {
    const float t = lfd_gauss_u8(c) / 255.0f;
    const float u = t - 0.5f;
    return u / LFD_GAUSS_SH_C0;
}

// (w, x, y, z) of the shortest-arc rotation that takes +z onto the normal n: (1 + nz, -ny, nx, 0) normalised in f32; (0, 1, 0, 0) where 1 + nz is
// below LFD_GAUSS_FLIP_BELOW; the identity for a normal that is zero or not finite
LFD_HD void lfd_gauss_rot(float nx, float ny, float nz, float* q) {
    q[0] = 1.0f; q[1] = 0.0f; q[2] = 0.0f; q[3] = 0.0f;
    if (!(__builtin_isfinite(nx) && __builtin_isfinite(ny) && __builtin_isfinite(nz))) return;
    if (nx == 0.0f && ny == 0.0f && nz == 0.0f) return;
    const float w = 1.0f + nz;
    if (w < LFD_GAUSS_FLIP_BELOW) { q[0] = 0.0f; q[1] = 1.0f; return; }
    const float x = -ny, y = nx;
    const float ww = w * w, xx = x * x, yy = y * y;
    const float wx = ww + xx;
    const float s = wx + yy;
    const float l = sqrtf(s);
    if (!(l > 0.0f) || !__builtin_isfinite(l)) return;
    q[0] = w / l; q[1] = x / l; q[2] = y / l;
}

// opacity: the f32 logit; log_flatten = log(gaussian_flatten) in f64; max_m: (f32) max_scale^2, or 0 for no cap
LFD_HD void lfd_gauss_record(const float* xyz, const float* nrm, const float* rgb, float dist2, float opacity, double log_flatten, float max_m,
                             float* o) {
    o[0] = xyz[0]; o[1] = xyz[1]; o[2] = xyz[2];
    o[3] = nrm[0]; o[4] = nrm[1]; o[5] = nrm[2];
    o[6] = lfd_gauss_dc(rgb[0]); o[7] = lfd_gauss_dc(rgb[1]); o[8] = lfd_gauss_dc(rgb[2]);
    o[9] = opacity;
    float m = dist2 > LFD_GAUSS_MIN_DIST2 ? dist2 : LFD_GAUSS_MIN_DIST2;
    if (max_m > 0.0f && m > max_m) m = max_m;
    const double ls = 0.5 * log((double)m);
    o[10] = (float)ls; o[11] = (float)ls;
    o[12] = (float)(ls + log_flatten);
    lfd_gauss_rot(nrm[0], nrm[1], nrm[2], o + 13);
}

inline const char* lfd_gauss_check(const float* xyz, const float* nrm, const float* rgb, const float* dist2, int64_t n, float opacity,
                                   double log_flatten, double max_scale, const uint8_t* out) {
    if (n < 0 || n > 0x7fffffffLL) return "n must be in [0, 2^31 - 1]";
    if (!__builtin_isfinite(opacity)) return "opacity_logit must be finite";
    if (!(log_flatten <= 0.0) || !(log_flatten >= -1.7976931348623157e308)) return "log_flatten must be finite and <= 0";
    if (!(max_scale >= 0.0) || !(max_scale <= 1.7976931348623157e308)) return "max_scale must be finite and >= 0 (0 = none)";
    if (n > 0 && (!xyz || !nrm || !rgb || !dist2 || !out)) return "null xyz / normals / rgb / dist2 / out";
    if (reinterpret_cast<uintptr_t>(out) & 3u) return "out must be 4-byte aligned";
    return nullptr;
}

// (f32) max_scale^2 as the record's cap; a positive max_scale whose square rounds to 0 caps at the smallest positive f32
inline float lfd_gauss_max_m(double max_scale) {
    if (!(max_scale > 0.0)) return 0.0f;
    const double sq = max_scale * max_scale;
    const float m = sq >= 3.4028234663852886e38 ? 3.4028234663852886e38f : (float)sq;
    return m > 0.0f ? m : 1.4012985e-45f;
}
