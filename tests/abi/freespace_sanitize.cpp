// Stand-alone host program around the shared routines of the free-space filter (csrc/lfd_freespace.hpp): the camera table, the z-buffers and
// lfd_freespace_count_point exactly as the twin drives them, on heap arrays of exactly n_refs * pw * ph words, with random clouds that include
// non-finite points and points on the image borders, checked against a brute-force count that knows no window loop.  Built with
// -fsanitize=address,undefined by tests/test_freespace_sanitized.py and run on its own: a read outside a plane, an out-of-range conversion of a
// cell index or a signed overflow ends it with a report and a non-zero status.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "lfd_freespace.hpp"

struct Cam { float P[12]; int w, h; };

// a camera on a ring of radius 4 at height 2 that looks at the origin: P = K [R | t], pixels
static Cam ring_cam(int i, int n, int w, int h) {
    const double th = 6.283185307179586 * i / n, c[3] = {4.0 * std::cos(th), 4.0 * std::sin(th), 2.0};
    double f[3] = {-c[0], -c[1], -c[2]};
    const double fn = std::sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
    for (double& v : f) v /= fn;
    double r[3] = {f[1], -f[0], 0.0};                                     // f x (0, 0, 1)
    const double rn = std::sqrt(r[0] * r[0] + r[1] * r[1]);
    for (double& v : r) v /= rn;
    const double d[3] = {f[1] * r[2] - f[2] * r[1], f[2] * r[0] - f[0] * r[2], f[0] * r[1] - f[1] * r[0]};
    const double* R[3] = {r, d, f};
    const double K[3][3] = {{0.75 * w, 0.0, 0.5 * w}, {0.0, 0.75 * w, 0.5 * h}, {0.0, 0.0, 1.0}};
    double Rt[3][4];
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) Rt[a][b] = R[a][b];
        Rt[a][3] = -(R[a][0] * c[0] + R[a][1] * c[1] + R[a][2] * c[2]);
    }
    Cam cam;
    cam.w = w; cam.h = h;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 4; ++b) cam.P[4 * a + b] = (float)(K[a][0] * Rt[0][b] + K[a][1] * Rt[1][b] + K[a][2] * Rt[2][b]);
    return cam;
}

// the definition once more, cell by cell with explicit bounds, on the f32 planes
static void brute(const std::vector<LfdFreespaceCam>& cams, const std::vector<float>& Z, int n_refs, int own, int pw, int ph, const float* X,
                  float tol, int& v, int& s) {
    v = s = 0;
    for (int j = 0; j < n_refs; ++j) {
        if (j == own) continue;
        int cx, cy;
        float d;
        if (!lfd_freespace_project(cams[(size_t)j], (double)pw, (double)ph, X[0], X[1], X[2], cx, cy, d)) continue;
        bool support = false, any = false;
        float dmin = std::numeric_limits<float>::infinity();
        for (int yy = std::max(0, cy - 1); yy <= std::min(ph - 1, cy + 1); ++yy)
            for (int xx = std::max(0, cx - 1); xx <= std::min(pw - 1, cx + 1); ++xx) {
                const float D = Z.at(((size_t)j * (size_t)ph + (size_t)yy) * (size_t)pw + (size_t)xx);
                if (!std::isfinite(D)) continue;
                any = true;
                const float t = tol * D;
                const float lo = D - t, hi = D + t;
                if (lo <= d && d <= hi) support = true;
                dmin = std::min(dmin, D);
            }
        if (support) { ++s; continue; }
        if (!any) continue;
        const float t = tol * dmin;
        const float lo = dmin - t;
        if (d < lo) ++v;
    }
}

static long long run_case(unsigned seed, long long n, int n_refs, int pw, int ph, float tol) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> uni(-1.5f, 1.5f), lift(0.1f, 1.5f);
    const int w = 640, h = 416;
    std::vector<Cam> raw;
    std::vector<LfdFreespaceCam> cams((size_t)n_refs);
    for (int r = 0; r < n_refs; ++r) {
        raw.push_back(ring_cam(r, n_refs, w, h));
        lfd_freespace_cam(raw.back().P, raw.back().w, raw.back().h, cams[(size_t)r]);
    }
    std::vector<float> xyz((size_t)(3 * n));
    std::vector<int> ref((size_t)n);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (long long i = 0; i < n; ++i) {
        ref[(size_t)i] = (int)((i * n_refs) / n);                        // grouped by reference, ascending
        float* X = &xyz[(size_t)(3 * i)];
        X[0] = uni(rng); X[1] = uni(rng); X[2] = (rng() % 5 == 0) ? lift(rng) : 0.0f;
        const unsigned roll = rng() % 50;
        if (roll == 0) X[rng() % 3] = nan;
        else if (roll == 1) X[rng() % 3] = (rng() & 1) ? inf : -inf;
        else if (roll == 2) X[rng() % 3] = 1e30f;
        else if (roll == 3) { X[0] *= 40.0f; X[1] *= 40.0f; X[2] = 30.0f; }    // behind cameras, outside every frustum
        else if (roll < 8) {
            // on the border of its own reference's image: the ray through pixel (u, v) of a corner or an edge, at depth 3 .. 5, by inverting
            // P = [M | p4]:  X = M^-1 (depth (u, v, 1) - p4), in f64
            const Cam& c = raw[(size_t)ref[(size_t)i]];
            const double us[4] = {0.0, (double)c.w - 1e-3, (double)c.w, 0.5 * c.w}, vs[4] = {0.0, (double)c.h - 1e-3, (double)c.h, 0.5 * c.h};
            const double u = us[rng() % 4], v = vs[rng() % 4], depth = 3.0 + (rng() % 3);
            const double M[3][3] = {{c.P[0], c.P[1], c.P[2]}, {c.P[4], c.P[5], c.P[6]}, {c.P[8], c.P[9], c.P[10]}};
            const double b[3] = {depth * u - c.P[3], depth * v - c.P[7], depth - c.P[11]};
            const double det = M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
                               M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
            for (int k = 0; k < 3; ++k) {
                double A[3][3];
                for (int a = 0; a < 3; ++a)
                    for (int q = 0; q < 3; ++q) A[a][q] = q == k ? b[a] : M[a][q];
                const double dk = A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
                                  A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
                X[k] = (float)(dk / det);
            }
        }
    }
    // z-buffers: heap arrays of exactly n_refs * pw * ph words, so that one word past a plane's end is a report
    const size_t words = (size_t)n_refs * (size_t)pw * (size_t)ph;
    uint32_t* zbuf = new uint32_t[words];
    for (size_t k = 0; k < words; ++k) zbuf[k] = LFD_FREESPACE_EMPTY;
    long long splats = 0;
    for (long long i = 0; i < n; ++i) {
        int cx, cy;
        float d;
        const int r = ref[(size_t)i];
        if (!lfd_freespace_project(cams[(size_t)r], (double)pw, (double)ph, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], cx, cy, d)) continue;
        if (cx < 0 || cx >= pw || cy < 0 || cy >= ph) { std::printf("cell (%d, %d) outside the %d x %d plane\n", cx, cy, pw, ph); std::exit(2); }
        uint32_t bits;
        std::memcpy(&bits, &d, 4);
        uint32_t& cell = zbuf[((size_t)r * (size_t)ph + (size_t)cy) * (size_t)pw + (size_t)cx];
        cell = std::min(cell, bits);
        ++splats;
    }
    std::vector<float> Z(words);
    std::memcpy(Z.data(), zbuf, words * 4);
    long long bad = 0, judged = 0;
    for (long long i = 0; i < n; ++i) {
        int v, s, bv, bs;
        lfd_freespace_count_point(cams.data(), zbuf, n_refs, ref[(size_t)i], pw, ph, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], tol, v, s);
        brute(cams, Z, n_refs, ref[(size_t)i], pw, ph, &xyz[(size_t)(3 * i)], tol, bv, bs);
        bad += (v != bv || s != bs) ? 1 : 0;
        judged += v + s;
        (void)lfd_freespace_keep(v, s, 1);
        (void)lfd_freespace_u8(v);
    }
    delete[] zbuf;
    std::printf("seed %u: %lld points, %d references, %d x %d: %lld splats, %lld verdicts, %lld mismatches\n", seed, n, n_refs, pw, ph, splats, judged, bad);
    return bad + (splats == 0 || judged == 0 ? 1 : 0);
}

int main() {
    long long bad = 0;
    bad += run_case(1, 3000, 5, 96, 62, 0.02f);
    bad += run_case(2, 2000, 9, 8, 6, 0.2f);
    bad += run_case(3, 1500, 3, 1, 1, 0.02f);
    bad += run_case(4, 4000, 40, 33, 17, 0.02f);
    bad += run_case(5, 2500, 7, 192, 124, 0.05f);
    std::printf(bad == 0 ? "ok (0 mismatches)\n" : "FAILED (%lld)\n", bad);
    return bad == 0 ? 0 : 1;
}
