// Stand-alone host program around the shared routines of oriented voxel fusion (csrc/lfd_fuse.hpp): the grid, the keys, the sort and the walk
// over the voxels with lfd_fuse_flag / lfd_fuse_add / lfd_fuse_emit exactly as the twin drives them, into heap arrays of exactly the rows the
// contract promises, on random clouds whose normals include zeros, NaN and infinities, checked bit for bit against a brute-force loop that
// knows nothing of the sort.  Built with -fsanitize=address,undefined by tests/test_fuse_sanitized.py and run on its own: a write behind the
// rows, a read outside the cloud or an out-of-range conversion ends it with a report and a non-zero status.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <set>
#include <utility>
#include <vector>

#include "lfd_fuse.hpp"

struct Rows {
    std::vector<float> xyz, nrm, rgb;
    std::vector<uint32_t> cnt;
};

static bool grid_of(const std::vector<float>& xyz, const std::vector<float>& rgb, long long n, double h, LfdFuseGrid& g, double& cscale) {
    float lo[3], hi[3], cmax = -std::numeric_limits<float>::infinity();
    for (int c = 0; c < 3; ++c) { lo[c] = std::numeric_limits<float>::infinity(); hi[c] = -lo[c]; }
    bool nan_rgb = false;
    for (long long i = 0; i < 3 * n; ++i) {
        const int c = (int)(i % 3);
        lo[c] = std::min(lo[c], xyz[(size_t)i]);
        hi[c] = std::max(hi[c], xyz[(size_t)i]);
        if (rgb[(size_t)i] != rgb[(size_t)i]) nan_rgb = true;
        else cmax = std::max(cmax, rgb[(size_t)i]);
    }
    cscale = lfd_fuse_cscale(cmax, nan_rgb);
    return lfd_fuse_grid(lo, hi, h, g);
}

// the twin's walk; the output arrays hold exactly `cap` rows
static long long walk(const std::vector<float>& xyz, const std::vector<float>& nrm, const std::vector<float>& rgb, long long n,
                      const std::vector<unsigned long long>& key, double cscale, long long cap, Rows& out) {
    std::vector<std::pair<unsigned long long, unsigned>> order((size_t)n);
    for (long long i = 0; i < n; ++i) order[(size_t)i] = {key[(size_t)i], (unsigned)i};
    std::sort(order.begin(), order.end());
    out.xyz.assign((size_t)(3 * cap), 0.0f); out.nrm.assign((size_t)(3 * cap), 0.0f); out.rgb.assign((size_t)(3 * cap), 0.0f);
    out.cnt.assign((size_t)cap, 0u);
    long long r = 0;
    for (long long a = 0; a < n;) {
        long long b = a + 1;
        while (b < n && order[(size_t)b].first == order[(size_t)a].first) ++b;
        LfdFuseAcc side[2];
        lfd_fuse_clear(side[0]);
        lfd_fuse_clear(side[1]);
        float piv[3] = {0.0f, 0.0f, 0.0f};
        bool has = false;
        for (long long j = a; j < b; ++j) {
            const long long i = order[(size_t)j].second;
            const float* nn = nrm.data() + 3 * i;
            const unsigned f = lfd_fuse_flag(nn, has, piv);
            if (!has && (f & LFD_FUSE_USABLE)) { has = true; piv[0] = nn[0]; piv[1] = nn[1]; piv[2] = nn[2]; }
            lfd_fuse_add(side[f & LFD_FUSE_SIDE], xyz.data() + 3 * i, nn, rgb.data() + 3 * i, (f & LFD_FUSE_USABLE) != 0u, cscale);
        }
        for (int s = 0; s < 2; ++s) {
            if (!side[s].cnt) continue;
            lfd_fuse_emit(side[s], out.xyz.data() + 3 * r, out.nrm.data() + 3 * r, out.rgb.data() + 3 * r);
            out.cnt[(size_t)r] = side[s].cnt;
            ++r;
        }
        a = b;
    }
    return r;
}

// the definition, voxel by voxel over the whole cloud in input order
static long long brute(const std::vector<float>& xyz, const std::vector<float>& nrm, const std::vector<float>& rgb, long long n,
                       const std::vector<unsigned long long>& key, double cscale, Rows& out) {
    const std::set<unsigned long long> voxels(key.begin(), key.end());
    out.xyz.clear(); out.nrm.clear(); out.rgb.clear(); out.cnt.clear();
    for (unsigned long long k : voxels) {
        long long pivot = -1;
        for (long long i = 0; i < n && pivot < 0; ++i)
            if (key[(size_t)i] == k && lfd_fuse_usable(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2])) pivot = i;
        for (int s = 0; s < 2; ++s) {
            double p[3] = {0, 0, 0}, c[3] = {0, 0, 0}, N[3] = {0, 0, 0};
            long long cnt = 0;
            for (long long i = 0; i < n; ++i) {
                if (key[(size_t)i] != k) continue;
                const bool ok = lfd_fuse_usable(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]);
                int side = 0;
                if (ok && pivot >= 0) {
                    const double d = ((double)nrm[3 * i] * (double)nrm[3 * pivot] + (double)nrm[3 * i + 1] * (double)nrm[3 * pivot + 1]) +
                                     (double)nrm[3 * i + 2] * (double)nrm[3 * pivot + 2];
                    side = d < 0.0 ? 1 : 0;
                }
                if (side != s) continue;
                for (int e = 0; e < 3; ++e) {
                    p[e] += (double)xyz[3 * i + e];
                    c[e] += (double)rgb[3 * i + e] / cscale;
                    if (ok) N[e] += (double)nrm[3 * i + e];
                }
                ++cnt;
            }
            if (!cnt) continue;
            const double q = (N[0] * N[0] + N[1] * N[1]) + N[2] * N[2];
            const bool unit = q > 0.0 && q <= std::numeric_limits<double>::max();
            for (int e = 0; e < 3; ++e) {
                out.xyz.push_back((float)(p[e] / (double)cnt));
                out.rgb.push_back((float)(c[e] / (double)cnt));
                out.nrm.push_back(unit ? (float)(N[e] / sqrt(q)) : 0.0f);
            }
            out.cnt.push_back((uint32_t)cnt);
        }
    }
    return (long long)out.cnt.size();
}

static int run_case(unsigned seed, long long n, double h, float extent, bool clustered, bool colours255) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> uni(-extent, extent), unit(-1.0f, 1.0f), col(0.0f, colours255 ? 255.0f : 1.0f);
    std::normal_distribution<float> jitter(0.0f, (float)h);
    std::vector<float> xyz((size_t)(3 * n)), nrm((size_t)(3 * n)), rgb((size_t)(3 * n)), centres;
    for (int c = 0; c < 12; ++c) centres.push_back(uni(rng));
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (long long i = 0; i < n; ++i) {
        for (int c = 0; c < 3; ++c) {
            xyz[(size_t)(3 * i + c)] = clustered ? centres[(size_t)((rng() % 4) * 3 + c)] + jitter(rng) : uni(rng);
            nrm[(size_t)(3 * i + c)] = unit(rng);
            rgb[(size_t)(3 * i + c)] = col(rng);
        }
        const unsigned roll = rng() % 16;                                       // a quarter of the normals are degenerate
        if (roll == 0) nrm[(size_t)(3 * i)] = nrm[(size_t)(3 * i + 1)] = nrm[(size_t)(3 * i + 2)] = 0.0f;
        else if (roll == 1) nrm[(size_t)(3 * i + (long long)(rng() % 3))] = nan;
        else if (roll == 2) nrm[(size_t)(3 * i + (long long)(rng() % 3))] = (rng() & 1u) ? inf : -inf;
        else if (roll == 3) nrm[(size_t)(3 * i + (long long)(rng() % 3))] = 3.0e38f;
        if (seed % 5 == 0 && i == n / 2) rgb[(size_t)(3 * i)] = nan;
    }
    LfdFuseGrid g;
    double cscale = 1.0;
    if (!grid_of(xyz, rgb, n, h, g, cscale)) { std::printf("case %u: the key range was refused\n", seed); return 1; }
    std::vector<unsigned long long> key((size_t)n);
    for (long long i = 0; i < n; ++i)
        key[(size_t)i] = lfd_fuse_key(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], g.origin[0], g.origin[1], g.origin[2], h, g.e[1], g.e[2]);
    Rows want, got;
    const long long rows = brute(xyz, nrm, rgb, n, key, cscale, want);
    if (rows > n) { std::printf("case %u: more rows than points\n", seed); return 1; }
    const long long r = walk(xyz, nrm, rgb, n, key, cscale, rows, got);         // exactly `rows` rows of room
    int bad = r != rows;
    if (!bad) {
        bad += std::memcmp(got.xyz.data(), want.xyz.data(), sizeof(float) * 3 * (size_t)rows) != 0;
        bad += std::memcmp(got.nrm.data(), want.nrm.data(), sizeof(float) * 3 * (size_t)rows) != 0;
        bad += std::memcmp(got.rgb.data(), want.rgb.data(), sizeof(float) * 3 * (size_t)rows) != 0;
        bad += std::memcmp(got.cnt.data(), want.cnt.data(), sizeof(uint32_t) * (size_t)rows) != 0;
    }
    if (bad) std::printf("case %u (n %lld, h %g): %lld rows against %lld, %d arrays differ\n", seed, n, h, r, rows, bad);
    return bad;
}

int main() {
    int bad = 0;
    unsigned seed = 1;
    for (long long n : {1LL, 2LL, 65LL, 700LL, 1500LL})
        for (double h : {1e-3, 0.05, 0.4, 50.0})
            for (int clustered = 0; clustered < 2; ++clustered, ++seed) bad += run_case(seed, n, h, 1.0f, clustered != 0, (seed & 1u) != 0u);
    // the checks of the arguments: the overlap arithmetic at the ends of the address space, every refusal once
    float a[6] = {0}, b[6] = {0}, c[6] = {0}, xo[6], no[6], ro[6];
    uint32_t cnt[2];
    int64_t rows = 0, vox = 0;
    bad += lfd_fuse_check(a, b, c, 2, 0.1, xo, no, ro, cnt, &rows, &vox) != nullptr;
    bad += lfd_fuse_check(a, b, c, 2, 0.1, a + 3, no, ro, cnt, &rows, &vox) == nullptr;
    bad += lfd_fuse_check(a, b, c, 2, 0.1, xo, xo + 5, ro, cnt, &rows, &vox) == nullptr;
    bad += lfd_fuse_check(a, b, c, 2, 0.0, xo, no, ro, nullptr, &rows, &vox) == nullptr;
    bad += lfd_fuse_check(a, b, c, -1, 0.1, xo, no, ro, nullptr, &rows, &vox) == nullptr;
    bad += lfd_fuse_check(nullptr, nullptr, nullptr, 0, 0.1, nullptr, nullptr, nullptr, nullptr, &rows, &vox) != nullptr;
    // the key-range refusal: nothing is converted out of range on the way to it
    LfdFuseGrid g;
    const float lo[3] = {-3.0e38f, -3.0e38f, -3.0e38f}, hi[3] = {3.0e38f, 3.0e38f, 3.0e38f};
    bad += lfd_fuse_grid(lo, hi, 1e-30, g);
    bad += lfd_fuse_grid(lo, hi, 1e25, g);
    const float lo1[3] = {-3.0e38f, 0.0f, 0.0f}, hi1[3] = {3.0e38f, 0.0f, 0.0f};        // 6e18 voxels along one axis: just inside 63 bits
    bad += !lfd_fuse_grid(lo1, hi1, 1e20, g);
    std::printf("ok (%d mismatches)\n", bad);
    return bad ? 1 : 0;
}
