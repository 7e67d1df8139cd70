// Stand-alone host program around the shared routine of the fused refiner block (csrc/lfd_block.hpp): lfd_block_fill and lfd_block_pixel exactly
// as the twin drives them, on (1, 3, 4, 5) - an image smaller than the window, every tap pattern at a border -, (1, 1, 2, 131) and (2, 32, 7, 9)
// with and without the pointwise part, from bf16 and from f32 input, over heap arrays of exactly the needed size, and checked against a plain
// f64 evaluation within a loose bound (the exact bound is the Python tests' business).  Built with -fsanitize=address,undefined by
// tests/test_refiner_block_sanitized.py and run on its own: a read outside the input or the weights, a write behind the output or an
// out-of-range conversion ends it with a report and a non-zero status.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "lfd_block.hpp"

static long long mismatches = 0;

static void run(int B, int C, int H, int W, bool f32, bool pointwise) {
    std::mt19937 rng((unsigned)(B * 1000 + C * 100 + H * 10 + W));
    std::normal_distribution<float> n01(0.0f, 1.0f);
    const size_t n = (size_t)B * C * H * W;
    std::vector<float> xf(f32 ? n : 0);
    std::vector<uint16_t> xh(f32 ? 0 : n);
    std::vector<double> xv(n);                                   // the bf16 values the block computes on
    for (size_t i = 0; i < n; ++i) {
        const float v = n01(rng);
        if (f32) xf[i] = v; else xh[i] = lfd_block_bf16(v);
        xv[i] = (double)lfd_block_round(v);
    }
    std::vector<float> w((size_t)C * 25), s((size_t)C), t((size_t)C), wt(pointwise ? (size_t)C * C : 0), pb(pointwise ? (size_t)C : 0);
    for (auto& v : w) v = 0.2f * n01(rng);
    for (auto& v : s) v = 1.0f + 0.2f * n01(rng);
    for (auto& v : t) v = 0.2f * n01(rng);
    for (auto& v : wt) v = n01(rng) / std::sqrt((float)C);
    for (auto& v : pb) v = 0.1f * n01(rng);
    std::vector<uint16_t> out(n, (uint16_t)0xffff);
    LfdBlockArgs p;
    const void* x = f32 ? (const void*)xf.data() : (const void*)xh.data();
    const char* why = lfd_block_fill(x, f32 ? 1 : 0, B, C, H, W, w.data(), s.data(), t.data(), pointwise ? wt.data() : nullptr,
                                     pointwise ? pb.data() : nullptr, out.data(), p);
    if (why) { std::printf("refused: %s\n", why); ++mismatches; return; }
    for (int b = 0; b < B; ++b)
        for (int c = 0; c < (pointwise ? 1 : C); ++c)
            for (int y = 0; y < H; ++y)
                for (int xx = 0; xx < W; ++xx) lfd_block_pixel(p, b, c, y, xx);
    // f64, taps outside the plane skipped
    std::vector<double> h(n);
    for (int b = 0; b < B; ++b)
        for (int c = 0; c < C; ++c)
            for (int y = 0; y < H; ++y)
                for (int xx = 0; xx < W; ++xx) {
                    double a = 0.0;
                    for (int ky = 0; ky < 5; ++ky)
                        for (int kx = 0; kx < 5; ++kx) {
                            const int yy = y + ky - 2, xc = xx + kx - 2;
                            if (yy < 0 || yy >= H || xc < 0 || xc >= W) continue;
                            a += (double)w[(size_t)c * 25 + 5 * ky + kx] * xv[(((size_t)b * C + c) * H + yy) * W + xc];
                        }
                    const double g = (double)s[c] * a + (double)t[c];
                    h[(((size_t)b * C + c) * H + y) * W + xx] = g > 0.0 ? g : 0.0;
                }
    long long bad = 0;
    for (int b = 0; b < B; ++b)
        for (int o = 0; o < C; ++o)
            for (int y = 0; y < H; ++y)
                for (int xx = 0; xx < W; ++xx) {
                    const size_t at = (((size_t)b * C + o) * H + y) * W + xx;
                    double want = h[at];
                    if (pointwise) {
                        want = (double)pb[o];
                        for (int c = 0; c < C; ++c) want += (double)wt[(size_t)c * C + o] * h[(((size_t)b * C + c) * H + y) * W + xx];
                    }
                    const double got = (double)lfd_block_widen(out[at]);
                    if (!(std::fabs(got - want) <= 0.02 * std::fabs(want) + 0.05)) ++bad;
                }
    std::printf("(%d, %d, %d, %d) %s %s: %lld mismatches\n", B, C, H, W, f32 ? "f32" : "bf16", pointwise ? "pointwise" : "depthwise", bad);
    mismatches += bad;
}

int main() {
    for (int f32 = 0; f32 < 2; ++f32) {
        run(1, 3, 4, 5, f32 != 0, false);
        run(1, 1, 2, 131, f32 != 0, false);
        run(2, 32, 7, 9, f32 != 0, false);
        run(2, 32, 7, 9, f32 != 0, true);
    }
    // the rounding at its edges: ties to even, the largest finite value, NaN
    if (lfd_block_bf16(1.00390625f) != 0x3f80 || lfd_block_bf16(1.01171875f) != 0x3f82 || lfd_block_bf16(lfd_block_float(0x7f7f8000u)) != 0x7f80 ||
        lfd_block_bf16(-0.0f) != 0x8000 || (lfd_block_bf16(NAN) & 0x7fc0) != 0x7fc0 || lfd_block_bf16(lfd_block_float(0x7f800001u)) != 0x7fc0)
        ++mismatches;
    // the refusals touch nothing
    LfdBlockArgs p;
    float one = 0.0f;
    uint16_t o16 = 0;
    if (!lfd_block_fill(&one, 1, 1, 1, 1, 1, &one, &one, &one, &one, nullptr, &o16, p) || !lfd_block_fill(&one, 1, 1, 1, 1, 1, &one, &one, &one, &one, &one, &o16, p) ||
        !lfd_block_fill(&one, 1, 65536, 32768, 1, 1, &one, &one, &one, nullptr, nullptr, &o16, p) ||
        !lfd_block_fill(&one, 1, 1, 1, 1, 1, &one, &one, &one, nullptr, nullptr, (uint16_t*)&one, p) ||
        lfd_block_fill(&one, 1, 1, 1, 1, 1, &one, &one, &one, nullptr, nullptr, &o16, p))
        ++mismatches;
    std::printf("ok (%lld mismatches)\n", mismatches);
    return mismatches ? 1 : 0;
}
