// Spatial point cap (lfd_cap_spatial): what the kernels (lfd_cap.hip) and the twin (lfd_host.hip) share - the Morton key of a point,
// the level at which two keys part, the level a budget selects, the pick predicate along the curve, the rank of an error and the checks of the
// arguments.
//
// The rule, over n points and a budget m: key every point by its 21-bit cell per axis in the cube of side L (the longest side of the bounding box)
// at the box's minimum, 63-bit Morton order; cells(l) is the number of distinct key prefixes of 3 l bits; lev is the smallest level with
// cells(lev) >= m (21 when there is none); of the c = cells(lev) cells in Morton order, m are picked evenly along the curve (all of them when
// c < m); a picked cell is represented by its point of smallest error (lowest input index on ties); the output is the representatives' input
// indices, ascending.  Every step is integer arithmetic or a single IEEE f64 operation written out as a statement of its own (the build uses
// -ffp-contract=off), so the device, the twin and a NumPy reference agree on the index set element for element.
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

#define LFD_CAP_LEVELS 21                        /* bits per axis of a key; levels are 0 .. LFD_CAP_LEVELS */
#define LFD_CAP_SCALE 2097152.0                  /* 2^21 cells along the cube's side at the finest level */
#define LFD_CAP_QMAX 2097151ull

struct LfdCapBox {
    double origin[3];            // the f32 minimum per axis
    double L;                    // the longest side, f64 from the f32 min and max; 0: every point is in cell 0
};

inline LfdCapBox lfd_cap_box(const float* lo, const float* hi) {
    LfdCapBox b;
    b.L = 0.0;
    for (int c = 0; c < 3; ++c) {
        b.origin[c] = (double)lo[c];
        const double side = (double)hi[c] - (double)lo[c];
        b.L = side > b.L ? side : b.L;
    }
    return b;
}

// cell of a coordinate at the finest level: 0 .. 2^21 - 1 (x >= o, so t >= 0; t <= 1 up to the division's rounding, which the clamp absorbs)
LFD_HD unsigned long long lfd_cap_cell(float x, double o, double L) {
    if (!(L > 0.0)) return 0ull;
    const double d = (double)x - o;
    const double t = d / L;
    const double u = t * LFD_CAP_SCALE;
    return u >= 2097151.0 ? LFD_CAP_QMAX : (unsigned long long)floor(u);
}

// the 21 bits of q spread to every third bit (bit i -> bit 3 i)
LFD_HD unsigned long long lfd_cap_spread(unsigned long long q) {
    q &= 0x1fffffull;
    q = (q | (q << 32)) & 0x001f00000000ffffull;
    q = (q | (q << 16)) & 0x001f0000ff0000ffull;
    q = (q | (q << 8)) & 0x100f00f00f00f00full;
    q = (q | (q << 4)) & 0x10c30c30c30c30c3ull;
    q = (q | (q << 2)) & 0x1249249249249249ull;
    return q;
}

// 63-bit Morton key: axis 0 is the most significant bit of every triple
LFD_HD unsigned long long lfd_cap_key(float x, float y, float z, const LfdCapBox& b) {
    const unsigned long long q0 = lfd_cap_cell(x, b.origin[0], b.L), q1 = lfd_cap_cell(y, b.origin[1], b.L), q2 = lfd_cap_cell(z, b.origin[2], b.L);
    return (lfd_cap_spread(q0) << 2) | (lfd_cap_spread(q1) << 1) | lfd_cap_spread(q2);
}

// the first level (1 .. 21) at which two different keys lie in different cells: the level of their highest differing bit triple; 0 for equal keys
LFD_HD int lfd_cap_pair_level(unsigned long long a, unsigned long long b) {
    const unsigned long long d = a ^ b;
    if (d == 0ull) return 0;
    const int hb = 63 - __builtin_clzll(d);                            // 0 .. 62
    return LFD_CAP_LEVELS - hb / 3;
}

// the key of a point's cell at level lev
LFD_HD unsigned long long lfd_cap_cell_key(unsigned long long key, int lev) { return key >> (3 * (LFD_CAP_LEVELS - lev)); }

// whether cell k of c (Morton order) is picked for a budget m <= c: floor((k + 1) m / c) > floor(k m / c); k, m, c < 2^31, so the products fit
LFD_HD bool lfd_cap_pick(unsigned long long k, unsigned long long m, unsigned long long c) {
    if (c <= m) return true;
    return ((k + 1ull) * m) / c > (k * m) / c;
}

// the monotone integer image of an f32 bit pattern: a < b as integers iff the floats compare so, with -0 < +0 and the NaN patterns by their bits
LFD_HD uint32_t lfd_cap_rank(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u); }

LFD_HD unsigned long long lfd_cap_pack(uint32_t rank, uint32_t index) { return ((unsigned long long)rank << 32) | (unsigned long long)index; }

// From hist[l] = adjacent pairs of sorted keys that part at level l (l = 1 .. 21; hist[0] unused) to cells[0 .. 21], the level of a budget and the
// call's statistics {lev, cells(lev), cells(lev - 1) (0 at level 0), L}.  n >= 1.
inline int lfd_cap_level(const unsigned long long* hist, long long budget, double L, long long* cells_out, double* stats) {
    long long cells[LFD_CAP_LEVELS + 1];
    cells[0] = 1;
    for (int l = 1; l <= LFD_CAP_LEVELS; ++l) cells[l] = cells[l - 1] + (long long)hist[l];
    int lev = LFD_CAP_LEVELS;
    for (int l = 0; l <= LFD_CAP_LEVELS; ++l)
        if (cells[l] >= budget) { lev = l; break; }
    *cells_out = cells[lev];
    if (stats) {
        stats[0] = (double)lev;
        stats[1] = (double)cells[lev];
        stats[2] = lev > 0 ? (double)cells[lev - 1] : 0.0;
        stats[3] = L;
    }
    return lev;
}

#define LFD_CAP_NONFINITE "non-finite coordinate in the input"

// What is wrong with the arguments of lfd_cap_spatial / lfd_cap_spatial_host (the context apart), or null.
inline const char* lfd_cap_check(const float* xyz, const float* err, int64_t n, int64_t budget, const int64_t* keep_out, const int64_t* n_keep_host) {
    if (n < 0 || n > 0x7fffffffLL) return "n must be in [0, 2^31 - 1]";
    if (budget < 1) return "budget must be >= 1";
    if (!n_keep_host) return "null n_keep_host";
    if (n > 0 && (!xyz || !keep_out)) return "null xyz / keep_out";
    if (n > 0) {
        const int64_t m = budget < n ? budget : n;
        const uintptr_t o0 = reinterpret_cast<uintptr_t>(keep_out), o1 = o0 + (uintptr_t)(8 * m);
        const uintptr_t a0 = reinterpret_cast<uintptr_t>(xyz), a1 = a0 + (uintptr_t)(12 * n);
        if (a0 < o1 && o0 < a1) return "in and out arrays overlap";
        if (err) {
            const uintptr_t e0 = reinterpret_cast<uintptr_t>(err), e1 = e0 + (uintptr_t)(4 * n);
            if (e0 < o1 && o0 < e1) return "in and out arrays overlap";
        }
    }
    return nullptr;
}
