// Per-camera depth and normal maps rendered from the final cloud (lfd_render_depth): what the kernels (lfd_depth.hip) and the twin
// (lfd_host.hip) share - the key of a (point, camera) pair, the keep test of a cell and the checks of a call's arguments.  The camera and the
// projection are lfd_freespace.hpp's, unchanged.
//
// Every camera renders into its own pw x ph plane of u64 keys.  A key is the f32 bits of the depth above the point's index, so one integer
// minimum picks the nearest point and, at equal depth, the lowest index: the result does not depend on the order of the points.
//   splat        K[cell] = the smallest key of all points whose own cell lies within Chebyshev distance r of `cell` (the part of the window inside the
//                plane): a square footprint of 2r + 1 cells that carries the winner's constant depth
//   visibility   D = depth of K[cell], m = the smallest finite depth of K within distance R of `cell`; the cell is kept iff D <= m + tol m (f32, every
//                rounding written out).  A point cloud is not watertight: what shows through the gaps of a nearer surface fails this test.
// Two identities (a minimum of minima is a minimum; DESIGN 4.22 has the argument for the plane's border): K is a (2r + 1)^2 min-filter over the
// r = 0 splat, and m is a (2 (R + r) + 1)^2 min-filter over the r = 0 depths.  The device uses both, the twin neither.
#pragma once

#include <stdint.h>

#include "lfd_freespace.hpp"

#define LFD_DEPTH_EMPTY 0x7f800000ffffffffull      // the bits of +inf above the index nobody has (n <= 2^31 - 1): a cell nobody wrote
#define LFD_DEPTH_MAX_SPLAT 3                      // r: 0 .. 3
#define LFD_DEPTH_MAX_WINDOW 8                     // R: 0 .. 8
#define LFD_DEPTH_KEY_BYTES (256ull << 20)         // cams_per_batch = 0: as many cameras as keep a batch's keys at or below this

LFD_HD uint64_t lfd_depth_key(float d, uint32_t i) {                    // d finite and > 0 (lfd_freespace_project), i < 2^31
    uint32_t bits;
    __builtin_memcpy(&bits, &d, 4);
    return ((uint64_t)bits << 32) | (uint64_t)i;
}

LFD_HD uint32_t lfd_depth_key_bits(uint64_t key) { return (uint32_t)(key >> 32); }
LFD_HD uint32_t lfd_depth_key_index(uint64_t key) { return (uint32_t)key; }
LFD_HD bool lfd_depth_key_empty(uint64_t key) { return lfd_depth_key_bits(key) >= LFD_FREESPACE_EMPTY; }

// A cell whose winner has the depth bits `dbits` (finite: the cell is not empty), `mbits` the smallest finite depth bits of its window (the cell
// itself belongs to the window, so mbits <= dbits): kept iff D <= m + tol m.
LFD_HD bool lfd_depth_keep(uint32_t dbits, uint32_t mbits, float tol) {
    float D, m;
    __builtin_memcpy(&D, &dbits, 4);
    __builtin_memcpy(&m, &mbits, 4);
    const float t = tol * m;
    const float hi = m + t;
    return D <= hi;
}

// Cameras of one batch: the argument taken literally when non-zero, else as many as keep the batch's u64 planes at or below LFD_DEPTH_KEY_BYTES.
inline int32_t lfd_depth_batch(int32_t n_cams, int32_t pw, int32_t ph, int32_t cams_per_batch) {
    long long per = cams_per_batch;
    if (per == 0) {
        per = (long long)(LFD_DEPTH_KEY_BYTES / ((unsigned long long)pw * (unsigned long long)ph * 8ull));
        per = per < 1 ? 1 : per;
    }
    return (int32_t)(per < n_cams ? per : n_cams);
}

// What is wrong with the arguments of lfd_render_depth / lfd_render_depth_host (the context apart), or null.
inline const char* lfd_depth_check(const float* xyz, int64_t n, const float* normals, const float* cam_P, const int32_t* cam_wh, int32_t n_cams,
                                   int32_t pw, int32_t ph, int32_t r, int32_t R, float tol, int32_t cams_per_batch, const float* depth_out,
                                   const int32_t* index_out, const float* normal_out) {
    if (!cam_P || !cam_wh) return "null cam_P_host / cam_wh_host";
    if (!depth_out) return "null depth_out";
    if (n < 0 || n > 0x7fffffffLL) return "n must be in [0, 2^31 - 1]";
    if (n > 0 && !xyz) return "null xyz";
    if ((normals == nullptr) != (normal_out == nullptr)) return "normals and normal_out must both be given or both be null";
    if (n_cams < 1) return "n_cams must be >= 1";
    if (pw < 1 || ph < 1) return "the plane pw x ph must be at least 1 x 1";
    if ((long long)n_cams * (long long)pw > 0x7fffffffLL || (long long)n_cams * (long long)pw * (long long)ph > 0x7fffffffLL)
        return "n_cams * pw * ph must be at most 2^31 - 1 cells";
    for (int32_t c = 0; c < n_cams; ++c) {
        if (cam_wh[2 * c] < 1 || cam_wh[2 * c + 1] < 1) return "a camera's image size w, h must be at least 1 x 1";
        for (int e = 0; e < 12; ++e)
            if (!(cam_P[12 * c + e] - cam_P[12 * c + e] == 0.0f)) return "a camera's P has an entry that is not finite";
    }
    if (r < 0 || r > LFD_DEPTH_MAX_SPLAT) return "splat_cells must be in [0, 3]";
    if (R < 0 || R > LFD_DEPTH_MAX_WINDOW) return "window_cells must be in [0, 8]";
    if (!(tol > 0.0f) || !(tol < 1.0f)) return "tol must be in (0, 1)";
    if (cams_per_batch < 0) return "cams_per_batch must be >= 0 (0 = automatic)";
    const long long cells = (long long)n_cams * pw * ph;
    const struct { const void* p; long long bytes; } a[2] = {{xyz, 12 * (long long)n}, {normals, 12 * (long long)n}},
                                                     b[3] = {{depth_out, 4 * cells}, {index_out, 4 * cells}, {normal_out, 12 * cells}};
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 3; ++j) {
            if (!a[i].p || !b[j].p || a[i].bytes == 0) continue;
            const uintptr_t a0 = reinterpret_cast<uintptr_t>(a[i].p), a1 = a0 + (uintptr_t)a[i].bytes;
            const uintptr_t b0 = reinterpret_cast<uintptr_t>(b[j].p), b1 = b0 + (uintptr_t)b[j].bytes;
            if (a0 < b1 && b0 < a1) return "in and out arrays overlap";
        }
    for (int i = 0; i < 3; ++i)
        for (int j = i + 1; j < 3; ++j) {
            if (!b[i].p || !b[j].p) continue;
            const uintptr_t a0 = reinterpret_cast<uintptr_t>(b[i].p), a1 = a0 + (uintptr_t)b[i].bytes;
            const uintptr_t b0 = reinterpret_cast<uintptr_t>(b[j].p), b1 = b0 + (uintptr_t)b[j].bytes;
            if (a0 < b1 && b0 < a1) return "out arrays overlap each other";
        }
    return nullptr;
}
