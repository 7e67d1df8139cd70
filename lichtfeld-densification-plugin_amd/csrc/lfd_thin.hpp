// Footprint-adaptive thinning of the final cloud (lfd_thin_footprint): what the kernels (lfd_thin.hip) and the twin (lfd_host.hip)
// share - the octree level a point's own camera gives it, its location code, the checks of the arguments and the twin's walk.
//
// The rule, over n points grouped by reference: the box and the 63-bit Morton key are the cap's (lfd_cap.hpp).  A point at depth z of its reference
// camera (z = the third row of [R | t] applied to it, f64) has the footprint g = (z tan_cell) thin_cells: thin_cells match-grid cells of that camera
// at that depth.  Its level is the deepest one (0 .. 20) whose cell side L / 2^level is still at least g, read from the exponent of q = L / g; its
// code is the linear-octree location code (1 << 3 level) | (key >> 3 (21 - level)), unique across levels.  Points of equal code form a cell; a
// cell keeps its point of smallest error rank (lowest input index on ties); the output is the kept input indices, ascending.  Every step is integer
// arithmetic or a single IEEE f64 operation written out as a statement of its own (the build uses -ffp-contract=off), so the device, the twin and a
// NumPy reference agree on the index set element for element.
#pragma once

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "lfd_cap.hpp"

#define LFD_THIN_MAX_LEVEL 20                    /* the deepest level: 3 * 20 key bits under the marker bit, a code below 2^61 */
#define LFD_THIN_LEVELS 21                       /* levels 0 .. 20 */
#define LFD_THIN_CODE_BITS 61
#define LFD_THIN_ROW 5                           /* f64 per reference: r3x r3y r3z t3 tan_cell */
#define LFD_THIN_STATS (2 * LFD_THIN_LEVELS + 1) /* points per level, cells per level, L */

// depth of a point in its reference camera: the third row of the world-to-camera [R | t], f64 from the f32 coordinates, one rounding per statement
LFD_HD double lfd_thin_depth(const double* row, float x, float y, float z) {
    const double ax = row[0] * (double)x;
    const double ay = row[1] * (double)y;
    const double az = row[2] * (double)z;
    const double s0 = ax + ay;
    const double s1 = s0 + az;
    return s1 + row[3];
}

// the level of a footprint g in a cube of side L: 20 where there is no positive finite footprint or no extent; else from q = L / g, 0 below 1 and
// otherwise the unbiased binary exponent of q (its bit pattern's; an infinite q reads 1024), at most 20.  L / 2^level >= g, and < 2 g unless clamped.
LFD_HD int lfd_thin_level(double depth, double tan_cell, double thin_cells, double L) {
    const double a = depth * tan_cell;
    const double g = a * thin_cells;
    if (!(g > 0.0) || g > 1.7976931348623157e308 || !(L > 0.0)) return LFD_THIN_MAX_LEVEL;
    const double q = L / g;
    if (q < 1.0) return 0;
    const unsigned long long bits = __builtin_bit_cast(unsigned long long, q);
    const int e = (int)((bits >> 52) & 0x7ffull) - 1023;               // q >= 1: the sign bit is clear and e >= 0
    return e < LFD_THIN_MAX_LEVEL ? e : LFD_THIN_MAX_LEVEL;
}

LFD_HD unsigned long long lfd_thin_code(unsigned long long key, int level) {
    return (1ull << (3 * level)) | (key >> (3 * (LFD_CAP_LEVELS - level)));
}

// the level of a code: its marker bit is bit 3 level
LFD_HD int lfd_thin_code_level(unsigned long long code) { return (63 - __builtin_clzll(code | 1ull)) / 3; }

#define LFD_THIN_NONFINITE LFD_CAP_NONFINITE

// What is wrong with the arguments of lfd_thin_footprint / lfd_thin_footprint_host (the context apart), or null.
inline const char* lfd_thin_check(const float* xyz, const float* err, int64_t n, const int64_t* offs, int32_t n_refs, const double* rows,
                                  double thin_cells, const int64_t* keep_out, const int64_t* n_keep_host, const int64_t* offs_out) {
    if (!offs || !offs_out || !n_keep_host || !rows) return "null ref_offsets_host / ref_offsets_out_host / n_keep_host / ref_rows_host";
    if (n < 0 || n > 0x7fffffffLL) return "n must be in [0, 2^31 - 1]";
    if (n_refs < 1) return "n_refs must be >= 1";
    if (n > 0 && (!xyz || !keep_out)) return "null xyz / keep_out";
    if (offs[0] != 0 || offs[n_refs] != n) return "ref_offsets_host must start at 0 and end at n";
    for (int32_t r = 0; r < n_refs; ++r)
        if (offs[r + 1] < offs[r]) return "ref_offsets_host must not decrease";
    if (!(thin_cells > 0.0) || !(thin_cells <= 1.7976931348623157e308)) return "thin_cells must be finite and > 0";
    for (int32_t r = 0; r < n_refs; ++r) {
        const double t = rows[LFD_THIN_ROW * (size_t)r + 4];
        if (!(t > 0.0) || !(t <= 1.7976931348623157e308)) return "every tan_cell must be finite and > 0";
    }
    if (n > 0) {
        const uintptr_t o0 = reinterpret_cast<uintptr_t>(keep_out), o1 = o0 + (uintptr_t)(8 * n);
        const uintptr_t a0 = reinterpret_cast<uintptr_t>(xyz), a1 = a0 + (uintptr_t)(12 * n);
        if (a0 < o1 && o0 < a1) return "in and out arrays overlap";
        if (err) {
            const uintptr_t e0 = reinterpret_cast<uintptr_t>(err), e1 = e0 + (uintptr_t)(4 * n);
            if (e0 < o1 && o0 < e1) return "in and out arrays overlap";
        }
    }
    return nullptr;
}

// The twin's walk behind the argument checks, n >= 1: one ordered pass over a stable sort of (code, index) pairs, whatever the thread count.
// keep_out: n entries; offs_out: n_refs + 1; stats: LFD_THIN_STATS or null.  Returns the number of kept points, or -1 for a non-finite coordinate
// (nothing is written then).
inline long long lfd_thin_walk(const float* xyz, const float* err, long long n, const int64_t* offs, int32_t n_refs, const double* rows,
                               double thin_cells, int64_t* keep_out, int64_t* offs_out, double* stats) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long long i = 0; i < 3 * n; ++i) {
        const int c = (int)(i % 3);
        if (!(xyz[i] - xyz[i] == 0.0f)) return -1;                      // infinite or NaN
        lo[c] = xyz[i] < lo[c] ? xyz[i] : lo[c];
        hi[c] = xyz[i] > hi[c] ? xyz[i] : hi[c];
    }
    const LfdCapBox box = lfd_cap_box(lo, hi);
    unsigned long long points[LFD_THIN_LEVELS] = {}, cells[LFD_THIN_LEVELS] = {};
    std::vector<std::pair<unsigned long long, unsigned>> order((size_t)n);
    for (int32_t r = 0; r < n_refs; ++r) {
        const double* row = rows + LFD_THIN_ROW * (size_t)r;
        for (long long i = offs[r]; i < offs[r + 1]; ++i) {
            const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
            const int lev = lfd_thin_level(lfd_thin_depth(row, x, y, z), row[4], thin_cells, box.L);
            ++points[lev];
            order[(size_t)i] = {lfd_thin_code(lfd_cap_key(x, y, z, box), lev), (unsigned)i};
        }
    }
    std::stable_sort(order.begin(), order.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    std::vector<uint8_t> keep((size_t)n, 0);
    for (long long a = 0; a < n;) {
        const unsigned long long code = order[(size_t)a].first;
        unsigned long long best = ~0ull;
        long long b = a;
        for (; b < n && order[(size_t)b].first == code; ++b) {
            const unsigned i = order[(size_t)b].second;
            uint32_t bits = 0u;
            if (err) memcpy(&bits, err + i, sizeof(bits));
            const unsigned long long v = lfd_cap_pack(err ? lfd_cap_rank(bits) : 0u, i);
            best = v < best ? v : best;
        }
        keep[(size_t)(best & 0xffffffffull)] = 1;
        ++cells[lfd_thin_code_level(code)];
        a = b;
    }
    long long kept = 0;
    for (int32_t r = 0; r < n_refs; ++r) {
        offs_out[r] = kept;
        for (long long i = offs[r]; i < offs[r + 1]; ++i)
            if (keep[(size_t)i]) keep_out[kept++] = i;
    }
    offs_out[n_refs] = kept;
    if (stats) {
        for (int l = 0; l < LFD_THIN_LEVELS; ++l) { stats[l] = (double)points[l]; stats[LFD_THIN_LEVELS + l] = (double)cells[l]; }
        stats[2 * LFD_THIN_LEVELS] = box.L;
    }
    return kept;
}
