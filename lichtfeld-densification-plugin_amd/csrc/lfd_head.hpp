// The output head of RoMa-v2's refiners (lfd_refiner_head): what the model runs behind the ninth conv block - two 1x1 convolutions
// (hidden -> 2 and hidden -> 4), the warp update, the Cholesky-to-precision conversion of the confidence and the addition of the previous state -
// in one pass over z.  The arithmetic, compiled for the device (lfd_head.hip) and for the host (lfd_host.hip's twin); every rounding is written
// out and the order is fixed:
//
//   a[o]   = head_b[o]; for c = 0..C-1: a[o] = fmaf(head_w[o][c], z[c], a[o])                       o = 0..5, six independent f32 chains
//   warp.x = prev_warp.x + a[0] / qx,  warp.y = prev_warp.y + a[1] / qy                              qx = refine_init * (float)W, qy = ... (float)H, in f32
//   sp(v)  = v > 20 ? v : (float)log1p(exp((double)v))                                              a NaN fails the compare and stays a NaN
//   l00 = sp(a[3]) + 1e-6f, l10 = a[4], l11 = sp(a[5]) + 1e-6f
//   d = (a[2], l00 l00, l00 l10, l10 l10 + l11 l11)                                                 two rounded products, then one add
//   conf[k] = prev[k] + d[k]        prev_dim 4; prev_dim 1: prev[1..3] = +0, added like any other; prev_dim 0: conf = d
//
// warp and conf[0] contain no libm call: device and twin agree on them bit for bit.  conf[1..3] pass through exp and log1p of the device's and
// the host's own libraries and may differ by the bound derived in DESIGN 4.20.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LFD_HEAD_HD __host__ __device__ __forceinline__
#else
#define LFD_HEAD_HD inline
#endif

#define LFD_HEAD_OUT 6                 // rows of head_w: 2 of the warp head, 4 of the confidence head
#define LFD_HEAD_SP_THRESHOLD 20.0f    // F.softplus's default threshold (beta 1)
#define LFD_HEAD_CHOL_EPS 1e-6f

// element i of z as f32: a bf16 word widened (exact), an f32 as it is
LFD_HEAD_HD float lfd_head_load(const void* z, bool is_f32, int64_t i) {
    if (is_f32) return static_cast<const float*>(z)[i];
    const uint32_t u = (uint32_t)static_cast<const uint16_t*>(z)[i] << 16;
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}

LFD_HEAD_HD float lfd_head_mix(float w, float z, float a) { return __builtin_fmaf(w, z, a); }

LFD_HEAD_HD float lfd_head_softplus(float v) { return v > LFD_HEAD_SP_THRESHOLD ? v : (float)log1p(exp((double)v)); }

// The six sums of a pixel -> its outputs.  pw: the previous warp; pc: the previous confidence, its first prev_dim values read.
LFD_HEAD_HD void lfd_head_finish(const float a[LFD_HEAD_OUT], float qx, float qy, const float pw[2], const float pc[4], int prev_dim, float warp[2],
                                 float conf[4]) {
    warp[0] = pw[0] + a[0] / qx;
    warp[1] = pw[1] + a[1] / qy;
    const float l00 = lfd_head_softplus(a[3]) + LFD_HEAD_CHOL_EPS, l10 = a[4], l11 = lfd_head_softplus(a[5]) + LFD_HEAD_CHOL_EPS;
    const float s0 = l10 * l10, s1 = l11 * l11;
    const float d0 = a[2], d1 = l00 * l00, d2 = l00 * l10, d3 = s0 + s1;
    if (prev_dim == 0) {
        conf[0] = d0; conf[1] = d1; conf[2] = d2; conf[3] = d3;
    } else {
        const bool all = prev_dim == 4;
        conf[0] = pc[0] + d0;
        conf[1] = (all ? pc[1] : 0.0f) + d1;
        conf[2] = (all ? pc[2] : 0.0f) + d2;
        conf[3] = (all ? pc[3] : 0.0f) + d3;
    }
}

// What a launch (or the twin) works on: z contiguous NCHW, warp (B, H, W, 2) and conf (B, H, W, 4) contiguous, the previous state through strides.
struct LfdHeadArgs {
    const void* z;
    const float* w;        // (6, C)
    const float* bias;     // (6)
    const float* pw;       // (B, H, W, 2) through sw
    const float* pc;       // (B, H, W, prev_dim) through sc; null with prev_dim 0
    float* warp;
    float* conf;
    int64_t sw[4], sc[4];  // element strides in the order b, y, x, c
    float qx, qy;          // refine_init * (float)W, refine_init * (float)H
    int32_t z_is_f32, B, C, H, W, prev_dim;
};

// One pixel (b, y, x) of both outputs: the reference form of the channel loop
inline void lfd_head_pixel(const LfdHeadArgs& p, int32_t b, int32_t y, int32_t x) {
    const int64_t hw = (int64_t)p.H * p.W, at = (int64_t)y * p.W + x;
    float a[LFD_HEAD_OUT];
    for (int o = 0; o < LFD_HEAD_OUT; ++o) a[o] = p.bias[o];
    for (int32_t c = 0; c < p.C; ++c) {
        const float v = lfd_head_load(p.z, p.z_is_f32 != 0, ((int64_t)b * p.C + c) * hw + at);
        for (int o = 0; o < LFD_HEAD_OUT; ++o) a[o] = lfd_head_mix(p.w[(int64_t)o * p.C + c], v, a[o]);
    }
    const float* q = p.pw + b * p.sw[0] + y * p.sw[1] + x * p.sw[2];
    const float pw[2] = {q[0], q[p.sw[3]]};
    float pc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (p.prev_dim) {
        const float* r = p.pc + b * p.sc[0] + y * p.sc[1] + x * p.sc[2];
        for (int k = 0; k < p.prev_dim; ++k) pc[k] = r[k * p.sc[3]];
    }
    const int64_t px = (int64_t)b * hw + at;
    lfd_head_finish(a, p.qx, p.qy, pw, pc, p.prev_dim, p.warp + 2 * px, p.conf + 4 * px);
}

// [lo, hi) in bytes of a (B, H, W, D) f32 array read through element strides s
inline void lfd_head_span(const float* base, const int64_t s[4], int32_t B, int32_t H, int32_t W, int32_t D, uintptr_t& lo, uintptr_t& hi) {
    const uint64_t last = (uint64_t)(B - 1) * (uint64_t)s[0] + (uint64_t)(H - 1) * (uint64_t)s[1] + (uint64_t)(W - 1) * (uint64_t)s[2] + (uint64_t)(D - 1) * (uint64_t)s[3];
    lo = reinterpret_cast<uintptr_t>(base);
    hi = lo + (uintptr_t)((last + 1) * 4u);
}

// Arguments of lfd_refiner_head / lfd_refiner_head_host -> LfdHeadArgs; what is wrong with them, or null.
inline const char* lfd_head_fill(const void* z, int32_t z_is_f32, int32_t B, int32_t C, int32_t H, int32_t W, const float* head_w, const float* head_b,
                                 const float* prev_warp, const int64_t* warp_strides, const float* prev_conf, const int64_t* conf_strides,
                                 int32_t prev_dim, float refine_init, float* warp, float* conf, LfdHeadArgs& p) {
    if (!z || !head_w || !head_b || !prev_warp || !warp || !conf) return "null pointer";
    if (prev_dim != 0 && prev_dim != 1 && prev_dim != 4) return "prev_dim must be 0, 1 or 4";
    if ((prev_dim == 0) != (prev_conf == nullptr)) return "prev_conf must be given with prev_dim 1 or 4 and null with prev_dim 0";
    if (B < 1 || C < 1 || H < 1 || W < 1) return "B, C, H, W must be >= 1";
    if (H > 32768 || W > 32768) return "H and W are at most 32768";
    const long long n = (long long)B * C;                     // < 2^62
    if (n > 0x7fffffffLL || n * H > 0x7fffffffLL || n * H * W > 0x7fffffffLL) return "B * C * H * W is at most 2^31 - 1";
    if (!(refine_init > 0.0f) || !(refine_init <= 3.402823466e+38f)) return "refine_init must be finite and > 0";
    const long long pixels = (long long)B * H * W;            // <= B C H W
    p.sw[0] = (int64_t)H * W * 2; p.sw[1] = (int64_t)W * 2; p.sw[2] = 2; p.sw[3] = 1;
    const int64_t d = prev_dim ? prev_dim : 1;
    p.sc[0] = (int64_t)H * W * d; p.sc[1] = (int64_t)W * d; p.sc[2] = d; p.sc[3] = 1;
    for (int k = 0; k < 4; ++k) {
        if (warp_strides) p.sw[k] = warp_strides[k];
        if (conf_strides && prev_dim) p.sc[k] = conf_strides[k];
        if (p.sw[k] < 0 || p.sc[k] < 0) return "negative stride";
        if (p.sw[k] > 0x7fffffffLL || p.sc[k] > 0x7fffffffLL) return "a stride is at most 2^31 - 1";
    }
    uintptr_t in_lo[5], in_hi[5];
    in_lo[0] = reinterpret_cast<uintptr_t>(z); in_hi[0] = in_lo[0] + (uintptr_t)(n * H * W) * (z_is_f32 ? 4u : 2u);
    in_lo[1] = reinterpret_cast<uintptr_t>(head_w); in_hi[1] = in_lo[1] + (uintptr_t)C * LFD_HEAD_OUT * 4u;
    in_lo[2] = reinterpret_cast<uintptr_t>(head_b); in_hi[2] = in_lo[2] + LFD_HEAD_OUT * 4u;
    lfd_head_span(prev_warp, p.sw, B, H, W, 2, in_lo[3], in_hi[3]);
    in_lo[4] = in_hi[4] = 0;
    if (prev_dim) lfd_head_span(prev_conf, p.sc, B, H, W, prev_dim, in_lo[4], in_hi[4]);
    const uintptr_t w0 = reinterpret_cast<uintptr_t>(warp), w1 = w0 + (uintptr_t)pixels * 8u;
    const uintptr_t c0 = reinterpret_cast<uintptr_t>(conf), c1 = c0 + (uintptr_t)pixels * 16u;
    if (w0 < c1 && c0 < w1) return "warp overlaps conf";
    static const char* const names[5] = {"an output overlaps z", "an output overlaps head_w", "an output overlaps head_b", "an output overlaps prev_warp",
                                         "an output overlaps prev_conf"};
    for (int k = 0; k < 5; ++k)
        if ((w0 < in_hi[k] && in_lo[k] < w1) || (c0 < in_hi[k] && in_lo[k] < c1)) return names[k];
    p.z = z; p.w = head_w; p.bias = head_b; p.pw = prev_warp; p.pc = prev_dim ? prev_conf : nullptr; p.warp = warp; p.conf = conf;
    p.qx = refine_init * (float)W; p.qy = refine_init * (float)H;
    p.z_is_f32 = z_is_f32 != 0; p.B = B; p.C = C; p.H = H; p.W = W; p.prev_dim = prev_dim;
    return nullptr;
}
