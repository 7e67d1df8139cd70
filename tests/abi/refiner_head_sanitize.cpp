// Stand-alone host program around the shared routine of the fused refiner head (csrc/lfd_head.hpp): lfd_head_fill and lfd_head_pixel exactly as
// the twin drives them, on (1, 3, 4, 5), (1, 1, 2, 131) and (2, 32, 7, 9), from bf16 and from f32 input, with prev_dim 0, 1 and 4, the previous
// state contiguous and as a planar (B, D, H, W) array read through strides, over heap arrays of exactly the needed size, and checked against a
// plain f64 evaluation within a loose bound (the exact bound is the Python tests' business).  Built with -fsanitize=address,undefined by
// tests/test_refiner_head_sanitized.py and run on its own: a read outside an input, a write behind an output or an out-of-range conversion ends
// it with a report and a non-zero status.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "lfd_head.hpp"

static long long mismatches = 0;

static uint16_t to_bf16(float f) {                               // truncation is enough here: the program computes on what it stored
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return (uint16_t)(u >> 16);
}

static void run(int B, int C, int H, int W, bool f32, int prev_dim, bool planar) {
    std::mt19937 rng((unsigned)(B * 1000 + C * 100 + H * 10 + W + prev_dim));
    std::normal_distribution<float> n01(0.0f, 1.0f);
    const size_t hw = (size_t)H * W, n = (size_t)B * C * hw, pixels = (size_t)B * hw;
    std::vector<float> zf(f32 ? n : 0);
    std::vector<uint16_t> zh(f32 ? 0 : n);
    std::vector<double> zv(n);
    for (size_t i = 0; i < n; ++i) {
        const float v = n01(rng);
        if (f32) { zf[i] = v; zv[i] = (double)v; }
        else { zh[i] = to_bf16(v); zv[i] = (double)lfd_head_load(zh.data(), false, (int64_t)i); }
    }
    std::vector<float> w((size_t)6 * C), bias(6), pw(pixels * 2), pc(pixels * (size_t)prev_dim);
    for (auto& v : w) v = n01(rng) / std::sqrt((float)C);
    for (auto& v : bias) v = 0.1f * n01(rng);
    for (auto& v : pw) v = n01(rng);
    for (auto& v : pc) v = n01(rng);
    // element strides in the order b, y, x, c: contiguous (B, H, W, D), or planar (B, D, H, W)
    const int64_t sw[4] = {(int64_t)hw * 2, planar ? W : 2 * W, planar ? 1 : 2, planar ? (int64_t)hw : 1};
    const int64_t d = prev_dim ? prev_dim : 1;
    const int64_t sc[4] = {(int64_t)hw * d, planar ? W : d * W, planar ? 1 : d, planar ? (int64_t)hw : 1};
    std::vector<float> warp(pixels * 2, NAN), conf(pixels * 4, NAN);
    LfdHeadArgs p;
    const void* z = f32 ? (const void*)zf.data() : (const void*)zh.data();
    const char* why = lfd_head_fill(z, f32 ? 1 : 0, B, C, H, W, w.data(), bias.data(), pw.data(), planar ? sw : nullptr, prev_dim ? pc.data() : nullptr,
                                    (planar && prev_dim) ? sc : nullptr, prev_dim, 4.0f, warp.data(), conf.data(), p);
    if (why) { std::printf("refused: %s\n", why); ++mismatches; return; }
    for (int b = 0; b < B; ++b)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) lfd_head_pixel(p, b, y, x);
    long long bad = 0;
    for (int b = 0; b < B; ++b)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                double a[6];
                for (int o = 0; o < 6; ++o) {
                    a[o] = (double)bias[o];
                    for (int c = 0; c < C; ++c) a[o] += (double)w[(size_t)o * C + c] * zv[((size_t)b * C + c) * hw + (size_t)y * W + x];
                }
                const size_t px = (size_t)b * hw + (size_t)y * W + x;
                auto prev = [&](const std::vector<float>& v, const int64_t* s, int k) { return (double)v[(size_t)(b * s[0] + y * s[1] + x * s[2] + k * s[3])]; };
                const double l00 = std::log1p(std::exp(a[3])) + 1e-6, l10 = a[4], l11 = std::log1p(std::exp(a[5])) + 1e-6;
                const double want_w[2] = {prev(pw, sw, 0) + a[0] / (4.0 * W), prev(pw, sw, 1) + a[1] / (4.0 * H)};
                double want_c[4] = {a[2], l00 * l00, l00 * l10, l10 * l10 + l11 * l11};
                for (int k = 0; k < prev_dim; ++k) want_c[k] += prev(pc, sc, k);
                for (int k = 0; k < 2; ++k)
                    if (!(std::fabs((double)warp[2 * px + k] - want_w[k]) <= 1e-5 * (1.0 + std::fabs(want_w[k])))) ++bad;
                for (int k = 0; k < 4; ++k)
                    if (!(std::fabs((double)conf[4 * px + k] - want_c[k]) <= 1e-4 * (1.0 + std::fabs(want_c[k])))) ++bad;
            }
    std::printf("(%d, %d, %d, %d) %s prev_dim %d %s: %lld mismatches\n", B, C, H, W, f32 ? "f32" : "bf16", prev_dim, planar ? "planar" : "contiguous", bad);
    mismatches += bad;
}

int main() {
    const int shapes[3][4] = {{1, 3, 4, 5}, {1, 1, 2, 131}, {2, 32, 7, 9}};
    const int dims[3] = {0, 1, 4};
    for (int f32 = 0; f32 < 2; ++f32)
        for (const auto& s : shapes)
            for (int prev_dim : dims)
                for (int planar = 0; planar < 2; ++planar) run(s[0], s[1], s[2], s[3], f32 != 0, prev_dim, planar != 0);
    // softplus at its edges: the threshold's two sides, both infinities, a NaN
    if (lfd_head_softplus(20.0001f) != 20.0001f || lfd_head_softplus(20.0f) != (float)std::log1p(std::exp(20.0)) || lfd_head_softplus(INFINITY) != INFINITY ||
        lfd_head_softplus(-INFINITY) != 0.0f || !std::isnan(lfd_head_softplus(NAN)))
        ++mismatches;
    // the refusals touch nothing
    LfdHeadArgs p;
    float in[8] = {0}, out_w[2], out_c[4];
    const int64_t negative[4] = {2, 2, -2, 1}, fine[4] = {2, 2, 2, 1};
    if (!lfd_head_fill(nullptr, 1, 1, 1, 1, 1, in, in, in, nullptr, nullptr, nullptr, 0, 4.0f, out_w, out_c, p) ||
        !lfd_head_fill(in, 1, 1, 1, 1, 1, in, in, in, nullptr, nullptr, nullptr, 2, 4.0f, out_w, out_c, p) ||
        !lfd_head_fill(in, 1, 1, 1, 1, 1, in, in, in, nullptr, in, nullptr, 0, 4.0f, out_w, out_c, p) ||
        !lfd_head_fill(in, 1, 1, 1, 1, 1, in, in, in, nullptr, nullptr, nullptr, 4, 4.0f, out_w, out_c, p) ||
        !lfd_head_fill(in, 1, 65536, 32768, 1, 1, in, in, in, nullptr, nullptr, nullptr, 0, 4.0f, out_w, out_c, p) ||
        !lfd_head_fill(in, 1, 1, 1, 1, 1, in, in, in, negative, nullptr, nullptr, 0, 4.0f, out_w, out_c, p) ||
        !lfd_head_fill(in, 1, 1, 1, 1, 1, in, in, in, nullptr, nullptr, nullptr, 0, INFINITY, out_w, out_c, p) ||
        !lfd_head_fill(in, 1, 1, 1, 1, 1, in, in, in, nullptr, nullptr, nullptr, 0, 4.0f, in, out_c, p) ||
        !lfd_head_fill(in, 1, 1, 1, 1, 1, in, in, in, nullptr, nullptr, nullptr, 0, 4.0f, out_c, out_c, p) ||
        lfd_head_fill(in, 1, 1, 1, 1, 1, in, in, in, fine, nullptr, nullptr, 0, 4.0f, out_w, out_c, p))
        ++mismatches;
    std::printf("ok (%lld mismatches)\n", mismatches);
    return mismatches ? 1 : 0;
}
