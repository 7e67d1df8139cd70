// Cross-reference consensus filter (lfd_consensus_filter): what the kernels (lfd_consensus.hip) and the twin (lfd_host.hip) share - the
// agreement test, the cell key, the per-point count over the sorted cloud, the grid of a call and the checks of its arguments.
//
// Two points agree when the f32 distance between them, every rounding written out and nothing contracted (the build uses -ffp-contract=off),
// is at most the radius:  d2 = (dx dx + dy dy) + dz dz <= radius radius.  The test is symmetric bit for bit (dx changes its sign only) and a
// NaN never agrees.  c_i counts the DISTINCT references other than the point's own that own a point agreeing with it, capped.
//
// Neighbours are found through a grid of cells of side h = 1.000001 radius (f64), whose linear keys are sorted: two agreeing points lie in cells
// at most 1 apart per axis (lfd_consensus_grid), so the 27 cells around a point hold every candidate; what is counted does not depend on the grid.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/lfd_densify.h"

#if defined(__HIPCC__)
#define LFD_HD __host__ __device__ __forceinline__
#else
#define LFD_HD inline
#endif

struct LfdConsensusPt {          // one point of the cloud in cell order: what a candidate costs the scan is one 16-byte load
    float x, y, z;
    int32_t ref;                 // the reference that owns it
};

LFD_HD bool lfd_consensus_finite(float x, float y, float z) { return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z); }

LFD_HD bool lfd_consensus_agree(float xi, float yi, float zi, float xj, float yj, float zj, float r2) {
    const float dx = xi - xj, dy = yi - yj, dz = zi - zj;
    const float sx = dx * dx, sy = dy * dy, sz = dz * dz;
    const float sxy = sx + sy;
    const float d2 = sxy + sz;
    return d2 <= r2;                       // a NaN anywhere rejects
}

// linear cell key of a point: key_c = floor(((f64) x_c - origin_c) / h) + 1 (IEEE subtract and divide), k0 E1 E2 + k1 E2 + k2; a point with a
// non-finite coordinate gets `sentinel`, which is larger than every cell's key
LFD_HD unsigned long long lfd_consensus_key(float x, float y, float z, double o0, double o1, double o2, double h, unsigned long long e1,
                                            unsigned long long e2, unsigned long long sentinel) {
    if (!lfd_consensus_finite(x, y, z)) return sentinel;
    const double k0 = floor(((double)x - o0) / h) + 1.0;
    const double k1 = floor(((double)y - o1) / h) + 1.0;
    const double k2 = floor(((double)z - o2) / h) + 1.0;
    return ((unsigned long long)k0 * e1 + (unsigned long long)k1) * e2 + (unsigned long long)k2;
}

// c of the point at sorted position j (not a sentinel one), counted up to `bound` <= CAP.  skey: the n keys in ascending order, spt: the points in
// that order.  Per (k0 + a, k1 + b) row the cells k2 - 1 .. k2 + 1 are ONE key range (E_c = max key_c + 2: a neighbour's key never wraps into the
// next row or plane): one binary search, then a walk.  The sort is stable and the input grouped by reference, so a cell's points form runs of
// ascending reference: `last` - the lane's own reference, then the one that vouched last - skips a run with one compare; the list of vouching
// references is looked up only where a run starts.  The list lives in registers: every index into it is a compile-time constant.
template <int CAP>
LFD_HD int lfd_consensus_count_point(const unsigned long long* skey, const LfdConsensusPt* spt, long long n, long long j, unsigned long long e1,
                                     unsigned long long e2, float r2, int bound) {
    const LfdConsensusPt me = spt[j];
    const unsigned long long key = skey[j];
    int ids[CAP];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int e = 0; e < CAP; ++e) ids[e] = -1;
    int cnt = 0, last = me.ref;
    for (int a = -1; a <= 1; ++a)
        for (int b = -1; b <= 1; ++b) {
            if (cnt >= bound) return cnt;
            const long long off = ((long long)a * (long long)e1 + (long long)b) * (long long)e2;
            const unsigned long long lo = key + (unsigned long long)off - 1ull, hi = lo + 2ull;      // k0, k1, k2 >= 1: never below 0
            long long l = 0, h = n;
            while (l < h) {
                const long long mid = (l + h) >> 1;
                if (skey[mid] < lo) l = mid + 1; else h = mid;
            }
            for (long long q = l; q < n && cnt < bound; ++q) {
                if (skey[q] > hi) break;
                const LfdConsensusPt p = spt[q];
                if (p.ref == last || p.ref == me.ref) continue;
                bool listed = false;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
                for (int e = 0; e < CAP; ++e) listed = listed || ids[e] == p.ref;
                if (listed) { last = p.ref; continue; }
                if (!lfd_consensus_agree(me.x, me.y, me.z, p.x, p.y, p.z, r2)) continue;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
                for (int e = 0; e < CAP; ++e) ids[e] = e == cnt ? p.ref : ids[e];
                ++cnt;
                last = p.ref;
            }
        }
    return cnt;
}

#define LFD_CONSENSUS_MAX_AXIS 1073741824.0      // 2^30 cells per axis: beyond it the f64 roundings of a key use up the margin of h

struct LfdConsensusGrid {
    double origin[3], h;
    unsigned long long e[3], sentinel;           // extents E_c = max key_c + 2; sentinel = E0 E1 E2, one past the largest cell key
    int bits;                                    // significant bits of the sentinel: what the radix sort has to look at
};

// The grid of a call from the min / max of the finite points.  h = 1.000001 radius: the f32 test admits true distances up to radius (1 + 3e-7)
// (five roundings of 2^-24 on d2, one on radius radius, halved by the root), so per axis |x_i - x_j| / h <= 1 - 7e-7 for an agreeing pair; each
// scaled coordinate carries two f64 roundings, at most 2^-52 of its value, which stays below that slack while it is below 2^30: the floors of
// two agreeing points differ by at most 1.  False: more than 2^30 cells along an axis, or a linear key beyond 63 bits.
inline bool lfd_consensus_grid(const float* lo, const float* hi, float radius, LfdConsensusGrid& g) {
    g.h = 1.000001 * (double)radius;
    for (int c = 0; c < 3; ++c) {
        g.origin[c] = (double)lo[c];
        const double kmax = floor(((double)hi[c] - g.origin[c]) / g.h) + 1.0;          // the key is monotone in the coordinate
        if (!(kmax < LFD_CONSENSUS_MAX_AXIS)) return false;
        g.e[c] = (unsigned long long)kmax + 2ull;
    }
    unsigned __int128 cells = (unsigned __int128)g.e[0] * g.e[1] * g.e[2];            // < 2^93
    if (cells > ((unsigned __int128)1 << 63)) return false;
    g.sentinel = (unsigned long long)cells;
    g.bits = 64 - __builtin_clzll(g.sentinel);
    return true;
}

// radius radius as the test uses it; the square has to be a normal f32 with room below it, or the distances it admits are not the radius any more
LFD_HD float lfd_consensus_r2(float radius) { return radius * radius; }

// What is wrong with the arguments of lfd_consensus_filter / lfd_consensus_filter_host (the context apart), or null.
inline const char* lfd_consensus_check(const float* xyz, const float* rgb, const float* err, int64_t n, const int64_t* offs, int32_t n_refs,
                                       float radius, int32_t min_refs, const float* xyz_out, const float* rgb_out, const float* err_out,
                                       const int64_t* offs_out, const uint8_t* consensus, const int64_t* n_out) {
    if (!offs || !offs_out || !n_out) return "null ref_offsets_host / ref_offsets_out_host / n_out_host";
    if (n < 0 || n > 0x7fffffffLL) return "n must be in [0, 2^31 - 1]";
    if (n_refs < 1) return "n_refs must be >= 1";
    if (n > 0 && (!xyz || !xyz_out)) return "null xyz / xyz_out";
    if ((rgb == nullptr) != (rgb_out == nullptr) || (err == nullptr) != (err_out == nullptr)) return "rgb / rgb_out and err / err_out must both be given or both be null";
    if (offs[0] != 0 || offs[n_refs] != n) return "ref_offsets_host must start at 0 and end at n";
    for (int32_t r = 0; r < n_refs; ++r)
        if (offs[r + 1] < offs[r]) return "ref_offsets_host must not decrease";
    const float r2 = lfd_consensus_r2(radius);
    if (!(radius > 0.0f) || !(radius <= 3.4028234e38f)) return "radius must be finite and > 0";
    if (!(r2 >= 1.9721523e-31f) || !(r2 <= 3.4028234e38f)) return "radius must be finite and > 0, with a square that is a normal f32 of at least 2^-102";
    if (min_refs < 1 || min_refs > LFD_CONSENSUS_CAP) return "min_refs must be in [1, LFD_CONSENSUS_CAP]";
    const struct { const void* p; long long elem; } a[3] = {{xyz, 12}, {rgb, 12}, {err, 4}}, b[4] = {{xyz_out, 12}, {rgb_out, 12}, {err_out, 4}, {consensus, 1}};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) {
            if (!a[i].p || !b[j].p) continue;
            const uintptr_t a0 = reinterpret_cast<uintptr_t>(a[i].p), a1 = a0 + (uintptr_t)(a[i].elem * n);
            const uintptr_t b0 = reinterpret_cast<uintptr_t>(b[j].p), b1 = b0 + (uintptr_t)(b[j].elem * n);
            if (a0 < b1 && b0 < a1) return "in and out arrays overlap";
        }
    return nullptr;
}
