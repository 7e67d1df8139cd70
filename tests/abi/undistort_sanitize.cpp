// Stand-alone host program around the per-pixel routine of the image undistortion (csrc/lfd_undistort.hpp): lfd_undistort_pixel exactly as the
// twin drives it, on random images and camera parameters - among them parameters whose intermediate values overflow, divide by zero or are
// not numbers - checked against a straightforward second implementation below.  Built with -fsanitize=address,undefined by
// tests/test_undistort_sanitized.py and run on its own: a tap outside the image, a signed overflow in an index or the conversion of a value
// that is no integer's ends it with a report and a non-zero status.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "lfd_undistort.hpp"

// the contract, written down once more: whole-image, plain indices, std::vector::at for every tap
static long long second_opinion(const std::vector<uint8_t>& src, int w, int h, int ch, bool nearest, const double* in, const double* d,
                                std::vector<uint8_t>& dst, std::vector<uint8_t>& valid) {
    long long bad = 0;
    for (int i = 0; i < h; ++i)
        for (int j = 0; j < w; ++j) {
            const double x = ((j + 0.5) - in[2]) / in[0], y = ((i + 0.5) - in[3]) / in[1];
            const double xx = x * x, yy = y * y, r2 = xx + yy, r4 = r2 * r2, r6 = r4 * r2, xy = x * y;
            const double num = ((1.0 + d[0] * r2) + d[1] * r4) + d[4] * r6, den = ((1.0 + d[5] * r2) + d[6] * r4) + d[7] * r6;
            const double rad = num / den;
            const double xd = (x * rad + (2.0 * d[2]) * xy) + d[3] * (r2 + 2.0 * xx);
            const double yd = (y * rad + (2.0 * d[3]) * xy) + d[2] * (r2 + 2.0 * yy);
            const double su = (in[0] * xd + in[2]) - 0.5, sv = (in[1] * yd + in[3]) - 0.5;
            const bool ok = std::isfinite(su) && std::isfinite(sv) && su >= -0.5 && su <= w - 0.5 && sv >= -0.5 && sv <= h - 0.5;
            const size_t o = (size_t)i * w + j;
            valid.at(o) = ok ? 255 : 0;
            if (!ok) { ++bad; for (int c = 0; c < ch; ++c) dst.at(o * ch + c) = 0; continue; }
            auto clampi = [](long long v, long long hi) { return v < 0 ? 0 : (v > hi ? hi : v); };
            if (nearest) {
                const long long xs = clampi((long long)std::floor(su + 0.5), w - 1), ys = clampi((long long)std::floor(sv + 0.5), h - 1);
                for (int c = 0; c < ch; ++c) dst.at(o * ch + c) = src.at((size_t)(ys * w + xs) * ch + c);
                continue;
            }
            const long long x0 = (long long)std::floor(su), y0 = (long long)std::floor(sv);
            const double ax = su - (double)x0, ay = sv - (double)y0;
            const long long xa = clampi(x0, w - 1), xb = clampi(x0 + 1, w - 1), ya = clampi(y0, h - 1), yb = clampi(y0 + 1, h - 1);
            for (int c = 0; c < ch; ++c) {
                const double p00 = src.at((size_t)(ya * w + xa) * ch + c), p01 = src.at((size_t)(ya * w + xb) * ch + c);
                const double p10 = src.at((size_t)(yb * w + xa) * ch + c), p11 = src.at((size_t)(yb * w + xb) * ch + c);
                const double top = p00 + ax * (p01 - p00), bot = p10 + ax * (p11 - p10);
                dst.at(o * ch + c) = (uint8_t)std::floor((top + ay * (bot - top)) + 0.5);
            }
        }
    return bad;
}

static int run_case(unsigned seed, int w, int h, int ch, bool nearest, int wild) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> uni(-1.0, 1.0);
    // exact-size buffers on the heap: AddressSanitizer sees the first byte outside them
    std::vector<uint8_t> src((size_t)w * h * ch), dst((size_t)w * h * ch, 7), valid((size_t)w * h, 7), dst2(dst), valid2(valid);
    for (auto& v : src) v = (uint8_t)(rng() & 255u);
    double in[4] = {0.9 * w + 40.0 * (uni(rng) + 1.5), 0.9 * w + 40.0 * (uni(rng) + 1.5), 0.5 * w + 3.0 * uni(rng), 0.5 * h + 3.0 * uni(rng)};
    double d[8];
    const double scale[8] = {0.3, 0.1, 0.01, 0.01, 0.05, 0.3, 0.1, 0.05};
    for (int e = 0; e < 8; ++e) d[e] = scale[e] * uni(rng);
    if (wild == 1) { d[0] = 1e300; d[1] = -1e300; }                               // inf - inf inside num: not a number
    if (wild == 2) { d[5] = -1.0 / ((0.25 / in[0]) * (0.25 / in[0]) * 2.0); }      // a denominator that passes through zero near the centre
    if (wild == 3) { in[0] = 1e-300; in[1] = 1e-300; d[0] = 1e10; }               // x, y overflow: infinities everywhere but one pixel
    if (wild == 4) { in[2] = -1e15; in[3] = 1e15; }                               // finite, far outside: no conversion of 1e15-sized values
    if (wild == 5) { d[2] = 1e200; d[3] = 1e200; d[0] = -1e200; }                 // huge finite coefficients
    if (wild == 6) { for (int e = 0; e < 8; ++e) d[e] = 0.0; }                    // the identity
    const LfdUndistortArgs p = lfd_undistort_args(src.data(), w, h, ch, nearest ? 1 : 0, in, d, dst.data(), valid.data());
    long long bad = 0;
    for (int i = 0; i < h; ++i)
        for (int j = 0; j < w; ++j) bad += lfd_undistort_pixel(p, i, j) ? 0 : 1;
    const long long bad2 = second_opinion(src, w, h, ch, nearest, in, d, dst2, valid2);
    int mismatches = (bad != bad2) ? 1 : 0;
    for (size_t k = 0; k < dst.size(); ++k) mismatches += dst[k] != dst2[k];
    for (size_t k = 0; k < valid.size(); ++k) mismatches += valid[k] != valid2[k];
    if (wild == 6 && (bad != 0 || dst != src)) ++mismatches;
    if (mismatches) std::printf("seed %u (%d x %d x %d, nearest %d, wild %d): %d mismatches, invalid %lld / %lld\n", seed, w, h, ch, (int)nearest, wild,
                                mismatches, bad, bad2);
    return mismatches;
}

int main() {
    int bad = 0;
    unsigned seed = 1;
    const int sizes[5][2] = {{1, 1}, {2, 2}, {67, 41}, {257, 3}, {96, 80}};
    for (const auto& s : sizes)
        for (int ch = 1; ch <= 3; ch += 2)
            for (int nearest = 0; nearest < 2; ++nearest)
                for (int wild = 0; wild <= 6; ++wild) bad += run_case(seed++, s[0], s[1], ch, nearest != 0, wild);
    // the checks of a call's arguments
    uint8_t a[64] = {0}, b[64] = {0};
    double in[4] = {10.0, 10.0, 2.0, 2.0}, d[8] = {0};
    bad += lfd_undistort_check(a, 4, 4, 3, in, d, b, nullptr) != nullptr;
    bad += lfd_undistort_check(a, 4, 4, 3, in, d, a + 8, nullptr) == nullptr;
    bad += lfd_undistort_check(a, 4, 4, 2, in, d, b, nullptr) == nullptr;
    bad += lfd_undistort_check(a, 0x10000, 0x8000, 1, in, d, b, nullptr) == nullptr;
    std::printf(bad ? "FAILED: %d mismatches\n" : "ok (%d mismatches)\n", bad);
    return bad ? 1 : 0;
}
