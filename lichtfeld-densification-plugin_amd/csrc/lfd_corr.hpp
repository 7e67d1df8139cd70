// Local correlation (lfd_local_corr): the per-sample arithmetic, compiled for the device (lfd_corr.hip) and for the host
// (lfd_host.hip's twin).
//
//   out[b, n, k] = sum_c A[b, n, c] * bilinear(Bf[b, :, :, c]; warp[b, n, k])
//
// with the sampling of F.grid_sample(mode="bilinear", padding_mode="zeros", align_corners=False): ix = ((x + 1) W1 - 1) / 2 in f32, the
// four texels around (ix, iy), a texel outside the map contributes nothing.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LFD_CORR_HD __host__ __device__ __forceinline__
#else
#define LFD_CORR_HD inline
#endif

// The four texels of one sample, tap j = (row y[j >> 1], column x[j & 1]): CLAMPED indices, always inside the map whatever the coordinate
// was, and the blend weight, 0 for a texel outside the map.
struct LfdCorrTaps {
    int32_t x[2], y[2];
    int32_t x0, y0;     // floor of the position, NOT clamped (in [-1, W1 - 1] x [-1, H1 - 1]); 0 when the sample touches nothing
    float w[4];         // (y0, x0) (y0, x1) (y1, x0) (y1, x1)
    bool live[4];       // the texel lies inside the map: only then is its value read into the sum
};

// false: the sample touches no texel of the map (it lies outside, or its coordinate is inf / NaN / too large to index with) and contributes
// exactly 0; `t` then names texel 0 four times, all dead, so that a caller without branches still reads inside the map.  No address is ever
// formed from an unclamped coordinate: the comparisons below are false for NaN, and a coordinate that passes them has -1 < ix < W1 <= 2^15,
// so floorf(ix) converts exactly (lfd_local_corr refuses larger maps).
LFD_CORR_HD bool lfd_corr_taps(float x, float y, int32_t W1, int32_t H1, LfdCorrTaps& t) {
    const float ix = ((x + 1.0f) * (float)W1 - 1.0f) / 2.0f;
    const float iy = ((y + 1.0f) * (float)H1 - 1.0f) / 2.0f;
    const bool inside = ix > -1.0f && ix < (float)W1 && iy > -1.0f && iy < (float)H1;
    const float sx = inside ? ix : 0.0f, sy = inside ? iy : 0.0f;
    const float fx = __builtin_floorf(sx), fy = __builtin_floorf(sy);
    const int32_t x0 = (int32_t)fx, y0 = (int32_t)fy;                 // in [-1, W1 - 1], [-1, H1 - 1]
    const float wx1 = sx - fx, wy1 = sy - fy;
    const float wx0 = (fx + 1.0f) - sx, wy0 = (fy + 1.0f) - sy;
    const bool lx0 = inside && x0 >= 0, lx1 = inside && x0 + 1 < W1, ly0 = inside && y0 >= 0, ly1 = inside && y0 + 1 < H1;
    const int32_t cx0 = lx0 ? x0 : 0, cx1 = lx1 ? x0 + 1 : (inside ? W1 - 1 : 0);
    const int32_t cy0 = ly0 ? y0 : 0, cy1 = ly1 ? y0 + 1 : (inside ? H1 - 1 : 0);
    t.x[0] = cx0; t.x[1] = cx1; t.y[0] = cy0; t.y[1] = cy1;
    t.x0 = x0; t.y0 = y0;
    t.live[0] = ly0 && lx0; t.live[1] = ly0 && lx1; t.live[2] = ly1 && lx0; t.live[3] = ly1 && lx1;
    t.w[0] = t.live[0] ? wy0 * wx0 : 0.0f; t.w[1] = t.live[1] ? wy0 * wx1 : 0.0f;
    t.w[2] = t.live[2] ? wy1 * wx0 : 0.0f; t.w[3] = t.live[3] ? wy1 * wx1 : 0.0f;
    return inside;
}

// One output element, channels in ascending order, any element strides: one running sum per texel, blended at the end.  `a` points at
// A[b, n, 0], `bf` at Bf[b, 0, 0, 0]; sy / sx / sc are Bf's element strides of row, column and channel.
LFD_CORR_HD float lfd_corr_sample(const float* a, int64_t sa_c, const float* bf, int64_t sy, int64_t sx, int64_t sc, int32_t C, int32_t W1,
                                  int32_t H1, float x, float y) {
    LfdCorrTaps t;
    if (!lfd_corr_taps(x, y, W1, H1, t)) return 0.0f;
    float out = 0.0f;
    for (int j = 0; j < 4; ++j) {
        if (!t.live[j]) continue;
        const float* p = bf + (int64_t)t.y[j >> 1] * sy + (int64_t)t.x[j & 1] * sx;
        float acc = 0.0f;
        for (int32_t c = 0; c < C; ++c) acc = acc + a[(int64_t)c * sa_c] * p[(int64_t)c * sc];
        out = out + t.w[j] * acc;
    }
    return out;
}

// What a launch (or the twin) works on.  warp (B, N, K, 2) and out (B, N, K) are contiguous; A and Bf come with element strides.
struct LfdCorrArgs {
    const float* a;
    const float* bf;
    const float* warp;
    float* out;
    int32_t B, N, C, K, H1, W1;
    int64_t sa_b, sa_n, sa_c;            // A (B, N, C)
    int64_t sb_b, sb_y, sb_x, sb_c;      // Bf (B, H1, W1, C)
};

// the fast layout: channels adjacent, C a multiple of 4, every row of channels 16-byte aligned
inline bool lfd_corr_vector_layout(const LfdCorrArgs& p) {
    const auto m4 = [](int64_t v) { return (v & 3) == 0; };
    return p.sa_c == 1 && p.sb_c == 1 && (p.C & 3) == 0 && m4(p.sa_b) && m4(p.sa_n) && m4(p.sb_b) && m4(p.sb_y) && m4(p.sb_x) &&
           (reinterpret_cast<uintptr_t>(p.a) & 15u) == 0 && (reinterpret_cast<uintptr_t>(p.bf) & 15u) == 0;
}

// Arguments of lfd_local_corr / lfd_local_corr_host -> LfdCorrArgs; what is wrong with them, or null.  Null strides: contiguous.
inline const char* lfd_corr_fill(const float* A, const float* Bf, const float* warp, int32_t B, int32_t N, int32_t C, int32_t K, int32_t H1, int32_t W1,
                                 const int64_t* a_strides, const int64_t* bf_strides, float* out, LfdCorrArgs& p) {
    if (B < 0 || N < 0 || K < 0 || C < 1 || H1 < 1 || W1 < 1) return "B, N, K must be >= 0 and C, H1, W1 >= 1";
    if (H1 > 32768 || W1 > 32768) return "H1 and W1 are at most 32768";
    if ((long long)B * N > 0x3ffffffLL || (long long)B * N * K > 0x7fffffffLL) return "B * N is at most 2^26 - 1 and B * N * K at most 2^31 - 1";
    if ((long long)B * N * K > 0 && (!A || !Bf || !warp || !out)) return "null pointer";
    p.a = A; p.bf = Bf; p.warp = warp; p.out = out;
    p.B = B; p.N = N; p.C = C; p.K = K; p.H1 = H1; p.W1 = W1;
    p.sa_c = a_strides ? a_strides[2] : 1; p.sa_n = a_strides ? a_strides[1] : C; p.sa_b = a_strides ? a_strides[0] : (int64_t)N * C;
    p.sb_c = bf_strides ? bf_strides[3] : 1; p.sb_x = bf_strides ? bf_strides[2] : C; p.sb_y = bf_strides ? bf_strides[1] : (int64_t)W1 * C;
    p.sb_b = bf_strides ? bf_strides[0] : (int64_t)H1 * W1 * C;
    if (p.sa_b < 0 || p.sa_n < 0 || p.sa_c < 0 || p.sb_b < 0 || p.sb_y < 0 || p.sb_x < 0 || p.sb_c < 0) return "negative stride";
    return nullptr;
}
