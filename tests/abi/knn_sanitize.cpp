// Stand-alone host program around the shared routines of the Gaussian-ready output (csrc/lfd_knn.hpp): the grid with its stop bounds, the keys,
// the sort, the ring scan of every point and the brute-force finish exactly as the twin drives them, over heap arrays of exactly n entries, on the
// clouds (c), (d) and (g) of the tests - duplicates, a lattice with points on cell faces, a surface with three far outliers - at several cell
// sizes, checked bit for bit against a brute-force loop that knows nothing of the grid; then the 68-byte record into an array of exactly 17 n
// floats.  Built with -fsanitize=address,undefined by tests/test_knn_sanitized.py and run on its own: a read outside the cloud, a write behind the
// outputs or an out-of-range conversion ends it with a report and a non-zero status.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <utility>
#include <vector>

#include "lfd_knn.hpp"

static std::vector<float> brute(const std::vector<float>& xyz, long long n) {
    std::vector<float> out((size_t)n);
    for (long long i = 0; i < n; ++i) {
        float a = INFINITY, b = INFINITY, c = INFINITY;
        for (long long j = 0; j < n; ++j) {
            if (j == i) continue;
            lfd_knn_insert(lfd_knn_d2(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], xyz[3 * j], xyz[3 * j + 1], xyz[3 * j + 2]), a, b, c);
        }
        out[(size_t)i] = lfd_knn_mean(a, b, c);
    }
    return out;
}

// the twin's call; cell_size 0 = automatic.  Returns the number of points the rings did not settle, -1 for a key-range refusal.
static long long through_the_grid(const std::vector<float>& xyz, long long n, double cell_size, std::vector<float>& out, double* h_used) {
    float lo[3], hi[3];
    for (int c = 0; c < 3; ++c) { lo[c] = std::numeric_limits<float>::infinity(); hi[c] = -lo[c]; }
    for (long long i = 0; i < 3 * n; ++i) { lo[i % 3] = std::min(lo[i % 3], xyz[(size_t)i]); hi[i % 3] = std::max(hi[i % 3], xyz[(size_t)i]); }
    double h = cell_size > 0.0 ? cell_size : lfd_knn_auto_h(lo, hi, n);
    LfdKnnGrid g;
    if (!lfd_knn_grid(lo, hi, h, g)) return -1;
    std::vector<std::pair<unsigned long long, unsigned>> order((size_t)n);
    for (int rebuilds = 0;;) {
        for (long long i = 0; i < n; ++i) order[(size_t)i] = {lfd_knn_key(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], g), (unsigned)i};
        std::sort(order.begin(), order.end());
        long long occupied = 0;
        for (long long a = 0; a < n; ++a) occupied += (a == 0 || order[(size_t)a].first != order[(size_t)a - 1].first) ? 1 : 0;
        LfdKnnGrid finer;
        if (cell_size > 0.0 || !lfd_knn_refine_more(n, occupied, rebuilds) || !lfd_knn_grid(lo, hi, h / 4.0, finer)) break;
        h = h / 4.0;
        g = finer;
        ++rebuilds;
    }
    *h_used = h;
    std::vector<unsigned long long> skey((size_t)n);
    std::vector<LfdKnnPt> spt((size_t)n);
    for (long long j = 0; j < n; ++j) {
        const unsigned i = order[(size_t)j].second;
        skey[(size_t)j] = order[(size_t)j].first;
        spt[(size_t)j] = {xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], i};
    }
    out.assign((size_t)n, -1.0f);
    long long open_points = 0;
    for (long long j = 0; j < n; ++j) {
        float mean;
        if (lfd_knn_scan_point(skey.data(), spt.data(), n, j, g, &mean)) { out[spt[(size_t)j].idx] = mean; continue; }
        ++open_points;
        float a = INFINITY, b = INFINITY, c = INFINITY;
        for (long long q = 0; q < n; ++q) {
            if (q == j) continue;
            lfd_knn_insert(lfd_knn_d2(spt[(size_t)j].x, spt[(size_t)j].y, spt[(size_t)j].z, spt[(size_t)q].x, spt[(size_t)q].y, spt[(size_t)q].z), a, b, c);
        }
        out[spt[(size_t)j].idx] = lfd_knn_mean(a, b, c);
    }
    return open_points;
}

static long long mismatches = 0;

static void run(const char* name, const std::vector<float>& xyz, const std::vector<double>& sizes) {
    const long long n = (long long)xyz.size() / 3;
    const std::vector<float> want = brute(xyz, n);
    for (double cs : sizes) {
        std::vector<float> got;
        double h = 0.0;
        const long long open_points = through_the_grid(xyz, n, cs, got, &h);
        if (open_points < 0) { std::printf("%s cell_size %g: refused\n", name, cs); ++mismatches; continue; }
        long long bad = 0;
        for (long long i = 0; i < n; ++i) bad += std::memcmp(&got[(size_t)i], &want[(size_t)i], 4) ? 1 : 0;
        std::printf("%s n %lld cell_size %g -> h %g: %lld by brute force, %lld mismatches\n", name, n, cs, h, open_points, bad);
        mismatches += bad;
    }
    // the record, into exactly 17 n floats
    std::mt19937 rng(5);
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    std::vector<float> nrm((size_t)(3 * n)), rgb((size_t)(3 * n)), rec((size_t)(LFD_GAUSS_FLOATS * n));
    for (auto& v : nrm) v = u(rng);
    for (auto& v : rgb) v = 0.6f * u(rng) + 0.5f;
    nrm[0] = 0.0f; nrm[1] = 0.0f; nrm[2] = -1.0f;
    nrm[3] = NAN;
    nrm[6] = 0.0f; nrm[7] = 0.0f; nrm[8] = 0.0f;
    rgb[0] = NAN; rgb[1] = 1e30f; rgb[2] = -1e30f;
    for (long long i = 0; i < n; ++i)
        lfd_gauss_record(xyz.data() + 3 * i, nrm.data() + 3 * i, rgb.data() + 3 * i, want[(size_t)i], -2.1972246f, std::log(0.1), lfd_gauss_max_m(0.5),
                         rec.data() + LFD_GAUSS_FLOATS * i);
    for (long long i = 0; i < n; ++i) {
        const float* r = rec.data() + LFD_GAUSS_FLOATS * i;
        const float q2 = r[13] * r[13] + r[14] * r[14] + r[15] * r[15] + r[16] * r[16];
        if (!(std::fabs(q2 - 1.0f) < 1e-5f) || !(r[10] == r[11]) || !(r[12] < r[10]) || std::memcmp(r, xyz.data() + 3 * i, 12)) ++mismatches;
    }
}

int main() {
    std::mt19937 rng(11);
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    std::normal_distribution<float> g01(0.0f, 0.01f);
    std::vector<float> c;
    for (int i = 0; i < 4; ++i) { c.push_back(0.25f); c.push_back(-0.5f); c.push_back(0.125f); }
    for (int i = 0; i < 180; ++i) c.push_back(u(rng));
    run("(c) duplicates", c, {0.0, 0.02, 2.0, 20.0});
    std::vector<float> d;
    for (int x = 0; x < 6; ++x) for (int y = 0; y < 6; ++y) for (int z = 0; z < 6; ++z) { d.push_back((float)x); d.push_back((float)y); d.push_back((float)z); }
    run("(d) lattice", d, {0.0, 1.0, 2.0, 0.5, 0.05, 5.0, 50.0});
    std::vector<float> g;
    for (int i = 0; i < 1200; ++i) { g.push_back(u(rng)); g.push_back(u(rng)); g.push_back(g01(rng)); }
    const float far_pts[9] = {1000.0f, 0.0f, 0.0f, -500.0f, 3.0f, 2.0f, -500.0f, 3.0f, 2.001f};
    g.insert(g.end(), far_pts, far_pts + 9);
    run("(g) surface with far outliers", g, {0.0, 15.0, 1500.0, 15000.0});
    // the limits of the grid: refused, nothing touched
    float lo[3] = {0.0f, 0.0f, 0.0f}, hi[3] = {1.0f, 1.0f, 1.0f};
    LfdKnnGrid grid;
    if (lfd_knn_grid(lo, hi, 1e-12, grid) || lfd_knn_grid(lo, hi, 3e-8, grid) || !lfd_knn_grid(lo, hi, 1e-3, grid)) ++mismatches;
    hi[0] = 3.0e38f; lo[0] = -3.0e38f;
    if (lfd_knn_grid(lo, hi, 1.0, grid) || !lfd_knn_grid(lo, hi, 1e300, grid)) ++mismatches;
    std::printf("ok (%lld mismatches)\n", mismatches);
    return mismatches ? 1 : 0;
}
