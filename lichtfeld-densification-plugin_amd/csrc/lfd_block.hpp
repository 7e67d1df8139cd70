// One conv block of RoMa-v2's refiners (lfd_refiner_block): depthwise 5x5 convolution, eval-mode BatchNorm folded into an
// affine, ReLU and - for the width-32 refiner - the 1x1 convolution, in one pass.  The arithmetic, compiled for the device (lfd_block.hip) and
// for the host (lfd_host.hip's twin); every rounding is written out and the order is fixed, so the two agree bit for bit:
//
//   x      the input rounded to bf16 (an f32 input is rounded on load, as autocast does)
//   a      = 0; for ky = 0..4, kx = 0..4: a = fmaf(w[c][5 ky + kx], x[y + ky - 2][x + kx - 2], a), a tap outside the plane SKIPPED
//   g      = fmaf(s[c], a, t[c])
//   h      = g <= 0 ? +0 : g (a NaN stays), rounded to bf16                                        -> the output without the pointwise part
//   z[o]   = pb[o]; for c = 0..C-1: z[o] = fmaf(Wt[c][o], h[c], z[o]), rounded to bf16            -> the output with it
//
// bf16 is handled as its 16 bits: round to nearest even in integer arithmetic, a NaN stays a quiet NaN.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LFD_BLOCK_HD __host__ __device__ __forceinline__
#else
#define LFD_BLOCK_HD inline
#endif

#define LFD_BLOCK_K 5                 // the window's side
#define LFD_BLOCK_R 2                 // ... and its radius
#define LFD_BLOCK_PW_C 32             // the only channel count the pointwise part is fused for

LFD_BLOCK_HD uint32_t lfd_block_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
LFD_BLOCK_HD float lfd_block_float(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }

// f32 -> the 16 bits of the nearest bf16, ties to even; a NaN keeps its sign and payload's top bits and gets the quiet bit
LFD_BLOCK_HD uint16_t lfd_block_bf16(float f) {
    const uint32_t u = lfd_block_bits(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x0040u);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
LFD_BLOCK_HD float lfd_block_widen(uint16_t h) { return lfd_block_float((uint32_t)h << 16); }
LFD_BLOCK_HD float lfd_block_round(float f) { return lfd_block_widen(lfd_block_bf16(f)); }           // f32 -> the bf16 value, as f32

// element i of the input as the bf16 value the block computes on
LFD_BLOCK_HD float lfd_block_load(const void* x, bool is_f32, int64_t i) {
    return is_f32 ? lfd_block_round(static_cast<const float*>(x)[i]) : lfd_block_widen(static_cast<const uint16_t*>(x)[i]);
}

LFD_BLOCK_HD float lfd_block_tap(float w, float v, float a) { return __builtin_fmaf(w, v, a); }
// affine, ReLU, rounding: the hidden value (a bf16 value held as f32)
LFD_BLOCK_HD float lfd_block_hidden(float s, float a, float t) {
    const float g = __builtin_fmaf(s, a, t);
    return lfd_block_round(g <= 0.0f ? 0.0f : g);
}
LFD_BLOCK_HD float lfd_block_mix(float wt, float h, float z) { return __builtin_fmaf(wt, h, z); }

// What a launch (or the twin) works on: x and out contiguous NCHW.
struct LfdBlockArgs {
    const void* x;
    const float* w;        // (C, 25)
    const float* s;        // (C)
    const float* t;        // (C)
    const float* wt;       // (C, C) transposed: row c multiplies hidden channel c; null without the pointwise part
    const float* pb;       // (C)
    uint16_t* out;
    int32_t x_is_f32, B, C, H, W;
};

// The hidden value of channel c at (y, x) of the plane that starts at element `plane` of the input: the reference form of the tap loop
LFD_BLOCK_HD float lfd_block_hidden_at(const LfdBlockArgs& p, int64_t plane, int32_t c, int32_t y, int32_t x) {
    const float* w = p.w + (int64_t)c * (LFD_BLOCK_K * LFD_BLOCK_K);
    float a = 0.0f;
    for (int ky = 0; ky < LFD_BLOCK_K; ++ky) {
        const int32_t yy = y + ky - LFD_BLOCK_R;
        if (yy < 0 || yy >= p.H) continue;
        for (int kx = 0; kx < LFD_BLOCK_K; ++kx) {
            const int32_t xx = x + kx - LFD_BLOCK_R;
            if (xx < 0 || xx >= p.W) continue;
            a = lfd_block_tap(w[LFD_BLOCK_K * ky + kx], lfd_block_load(p.x, p.x_is_f32 != 0, plane + (int64_t)yy * p.W + xx), a);
        }
    }
    return lfd_block_hidden(p.s[c], a, p.t[c]);
}

// One pixel (b, y, x) of the output, all its channels with the pointwise part (C == 32), channel c alone without it
inline void lfd_block_pixel(const LfdBlockArgs& p, int32_t b, int32_t c, int32_t y, int32_t x) {
    const int64_t hw = (int64_t)p.H * p.W, at = (int64_t)y * p.W + x;
    if (!p.wt) {
        const int64_t plane = ((int64_t)b * p.C + c) * hw;
        p.out[plane + at] = lfd_block_bf16(lfd_block_hidden_at(p, plane, c, y, x));
        return;
    }
    float z[LFD_BLOCK_PW_C];
    for (int o = 0; o < LFD_BLOCK_PW_C; ++o) z[o] = p.pb[o];
    for (int cc = 0; cc < LFD_BLOCK_PW_C; ++cc) {
        const float h = lfd_block_hidden_at(p, ((int64_t)b * p.C + cc) * hw, cc, y, x);
        for (int o = 0; o < LFD_BLOCK_PW_C; ++o) z[o] = lfd_block_mix(p.wt[cc * LFD_BLOCK_PW_C + o], h, z[o]);
    }
    for (int o = 0; o < LFD_BLOCK_PW_C; ++o) p.out[((int64_t)b * p.C + o) * hw + at] = lfd_block_bf16(z[o]);
}

// Arguments of lfd_refiner_block / lfd_refiner_block_host -> LfdBlockArgs; what is wrong with them, or null.
inline const char* lfd_block_fill(const void* x, int32_t x_is_f32, int32_t B, int32_t C, int32_t H, int32_t W, const float* dw_w, const float* scale,
                                  const float* shift, const float* pw_wT, const float* pw_b, uint16_t* out, LfdBlockArgs& p) {
    if (!x || !dw_w || !scale || !shift || !out) return "null pointer";
    if ((pw_wT == nullptr) != (pw_b == nullptr)) return "pw_wT and pw_b must both be given or both be null";
    if (B < 1 || C < 1 || H < 1 || W < 1) return "B, C, H, W must be >= 1";
    if (pw_wT && C != LFD_BLOCK_PW_C) return "pointwise fusion implements C == 32 only";
    if (H > 32768 || W > 32768) return "H and W are at most 32768";
    const long long n = (long long)B * C;                     // < 2^62
    if (n > 0x7fffffffLL || n * H > 0x7fffffffLL || n * H * W > 0x7fffffffLL) return "B * C * H * W is at most 2^31 - 1";
    const uintptr_t x0 = reinterpret_cast<uintptr_t>(x), x1 = x0 + (uintptr_t)(n * H * W) * (x_is_f32 ? 4u : 2u);
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(out), o1 = o0 + (uintptr_t)(n * H * W) * 2u;
    if (o0 < x1 && x0 < o1) return "out overlaps x";
    p.x = x; p.w = dw_w; p.s = scale; p.t = shift; p.wt = pw_wT; p.pb = pw_b; p.out = out;
    p.x_is_f32 = x_is_f32 != 0; p.B = B; p.C = C; p.H = H; p.W = W;
    return nullptr;
}
