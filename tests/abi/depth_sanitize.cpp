// Stand-alone host program around the shared routines of the depth-map renderer (csrc/lfd_depth.hpp): keys, the keep test, the batch rule and the
// argument check, driven as the twin drives them - every point into every cell of its footprint, every cell's window walked - on heap planes of
// exactly pw * ph words, with random clouds that include non-finite points, points far outside and planes smaller than the windows.  The result
// is compared with the device's formulation written as brute force: the (2r + 1)^2 minimum over the r = 0 splat and the (2(R + r) + 1)^2 minimum
// over its depths.  Built with -fsanitize=address,undefined by tests/test_depth_maps_sanitized.py and run on its own: a write outside a plane, an
// out-of-range conversion of a cell index or a signed overflow ends it with a report and a non-zero status.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "lfd_depth.hpp"

static long long run_case(unsigned seed, long long n, int pw, int ph, int r, int R, float tol) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> uni(-2.0f, 2.0f), deep(1.0f, 6.0f);
    const int w = 64, h = 40;
    const float P[12] = {58.0f, 0.0f, 32.0f, 1.5f, 0.0f, 58.0f, 20.0f, -0.5f, 0.0f, 0.0f, 1.0f, 0.25f};
    const int32_t wh[2] = {w, h};
    LfdFreespaceCam cam;
    lfd_freespace_cam(P, w, h, cam);
    std::vector<float> xyz((size_t)(3 * n));
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (long long i = 0; i < n; ++i) {
        float* X = &xyz[(size_t)(3 * i)];
        X[0] = uni(rng); X[1] = uni(rng); X[2] = (rng() % 4 == 0) ? 2.0f : deep(rng);      // a quarter on one plane: equal depth bits meet
        const unsigned roll = rng() % 40;
        if (roll == 0) X[rng() % 3] = nan;
        else if (roll == 1) X[rng() % 3] = (rng() & 1) ? inf : -inf;
        else if (roll == 2) X[rng() % 3] = 3e38f;
        else if (roll == 3) X[2] = -X[2];
        else if (roll == 4) { X[0] *= 1e6f; X[1] *= -1e6f; }
    }
    const size_t cells = (size_t)pw * (size_t)ph;
    float* depth_out = new float[cells];
    if (lfd_depth_check(xyz.data(), n, nullptr, P, wh, 1, pw, ph, r, R, tol, 0, depth_out, nullptr, nullptr)) { std::printf("good arguments refused\n"); std::exit(2); }
    if (lfd_depth_batch(7, pw, ph, 0) < 1 || lfd_depth_batch(7, pw, ph, 3) != 3 || lfd_depth_batch(2, pw, ph, 3) != 2) { std::printf("batch rule\n"); std::exit(2); }
    // heap planes of exactly pw * ph words, so that one word past a plane's end is a report
    uint64_t* K = new uint64_t[cells];
    uint64_t* raw = new uint64_t[cells];
    for (size_t k = 0; k < cells; ++k) K[k] = raw[k] = LFD_DEPTH_EMPTY;
    long long inside = 0;
    for (long long i = 0; i < n; ++i) {
        int cx, cy;
        float d;
        if (!lfd_freespace_project(cam, (double)pw, (double)ph, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], cx, cy, d)) continue;
        if (cx < 0 || cx >= pw || cy < 0 || cy >= ph) { std::printf("cell (%d, %d) outside the %d x %d plane\n", cx, cy, pw, ph); std::exit(2); }
        const uint64_t key = lfd_depth_key(d, (uint32_t)i);
        float back;
        const uint32_t bits = lfd_depth_key_bits(key);
        std::memcpy(&back, &bits, 4);
        if (back != d || lfd_depth_key_index(key) != (uint32_t)i || lfd_depth_key_empty(key)) { std::printf("key round trip\n"); std::exit(2); }
        raw[(size_t)cy * pw + cx] = std::min(raw[(size_t)cy * pw + cx], key);
        for (int yy = std::max(0, cy - r); yy <= std::min(ph - 1, cy + r); ++yy)
            for (int xx = std::max(0, cx - r); xx <= std::min(pw - 1, cx + r); ++xx) K[(size_t)yy * pw + xx] = std::min(K[(size_t)yy * pw + xx], key);
        ++inside;
    }
    long long bad = 0, kept = 0, dropped = 0;
    for (int y = 0; y < ph; ++y)
        for (int x = 0; x < pw; ++x) {
            // the definition, as the twin walks it
            const uint64_t key = K[(size_t)y * pw + x];
            bool keep = !lfd_depth_key_empty(key);
            if (keep) {
                uint32_t m = LFD_FREESPACE_EMPTY;
                for (int yy = std::max(0, y - R); yy <= std::min(ph - 1, y + R); ++yy)
                    for (int xx = std::max(0, x - R); xx <= std::min(pw - 1, x + R); ++xx) m = std::min(m, lfd_depth_key_bits(K[(size_t)yy * pw + xx]));
                keep = lfd_depth_keep(lfd_depth_key_bits(key), m, tol);
            }
            // both identities, over the r = 0 splat
            uint64_t key2 = LFD_DEPTH_EMPTY;
            for (int yy = std::max(0, y - r); yy <= std::min(ph - 1, y + r); ++yy)
                for (int xx = std::max(0, x - r); xx <= std::min(pw - 1, x + r); ++xx) key2 = std::min(key2, raw[(size_t)yy * pw + xx]);
            uint32_t m2 = LFD_FREESPACE_EMPTY;
            const int H = R + r;
            for (int yy = std::max(0, y - H); yy <= std::min(ph - 1, y + H); ++yy)
                for (int xx = std::max(0, x - H); xx <= std::min(pw - 1, x + H); ++xx) m2 = std::min(m2, lfd_depth_key_bits(raw[(size_t)yy * pw + xx]));
            const bool keep2 = !lfd_depth_key_empty(key2) && lfd_depth_keep(lfd_depth_key_bits(key2), m2, tol);
            bad += (key != key2 || keep != keep2) ? 1 : 0;
            kept += keep ? 1 : 0;
            dropped += (!keep && !lfd_depth_key_empty(key)) ? 1 : 0;
            depth_out[(size_t)y * pw + x] = keep ? 1.0f : 0.0f;
        }
    delete[] K;
    delete[] raw;
    delete[] depth_out;
    std::printf("seed %u: %lld points (%lld inside), %d x %d, r %d, R %d: %lld cells kept, %lld dropped, %lld mismatches\n", seed, n, inside, pw, ph, r, R,
                kept, dropped, bad);
    return bad + (inside == 0 || kept == 0 ? 1 : 0);
}

int main() {
    long long bad = 0;
    bad += run_case(1, 3000, 37, 23, 1, 3, 0.02f);
    bad += run_case(2, 2000, 8, 6, 3, 8, 0.02f);         // windows larger than the plane
    bad += run_case(3, 500, 1, 1, 3, 8, 0.02f);
    bad += run_case(4, 4000, 130, 67, 0, 0, 0.02f);
    bad += run_case(5, 2500, 64, 40, 0, 8, 0.2f);
    bad += run_case(6, 2500, 5, 97, 3, 0, 0.02f);
    std::printf(bad == 0 ? "ok (0 mismatches)\n" : "FAILED (%lld)\n", bad);
    return bad == 0 ? 0 : 1;
}
