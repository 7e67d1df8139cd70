// Stand-alone host program around the shared routines of the spatial point cap (csrc/lfd_cap.hpp): the box, the keys, the stable sort, the level
// histogram, the level of a budget, the walk over the cells with the pick predicate and the error ranks exactly as the twin drives them, into a
// heap array of exactly min(budget, n) indices and a heap array of exactly four statistics, on the clouds (c), (d) and (g) of the tests -
// duplicates, a lattice with points on cell faces and the clamp at its maximum corner, two densities with a far outlier -, checked element for
// element against a loop that knows nothing of the sort: cells in an ordered map, the pick in 128-bit integers, the bits interleaved one by one.
// Built with -fsanitize=address,undefined by tests/test_cap_sanitized.py and run on its own: a read outside the cloud, a write behind the outputs
// or an out-of-range conversion ends it with a report and a non-zero status.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <random>
#include <utility>
#include <vector>

#include "lfd_cap.hpp"

// the twin's call (lfd_cap_spatial_host behind its argument checks); keep_out holds exactly min(budget, n) entries, stats exactly four
static long long through_the_header(const std::vector<float>& xyz, const float* err, long long n, long long budget, long long* keep_out, double* stats) {
    float lo[3], hi[3];
    for (int c = 0; c < 3; ++c) { lo[c] = std::numeric_limits<float>::infinity(); hi[c] = -lo[c]; }
    for (long long i = 0; i < 3 * n; ++i) { lo[i % 3] = std::min(lo[i % 3], xyz[(size_t)i]); hi[i % 3] = std::max(hi[i % 3], xyz[(size_t)i]); }
    const LfdCapBox box = lfd_cap_box(lo, hi);
    std::vector<std::pair<unsigned long long, unsigned>> order((size_t)n);
    for (long long i = 0; i < n; ++i) order[(size_t)i] = {lfd_cap_key(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], box), (unsigned)i};
    std::stable_sort(order.begin(), order.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    unsigned long long hist[LFD_CAP_LEVELS + 1] = {};
    for (long long j = 1; j < n; ++j) ++hist[lfd_cap_pair_level(order[(size_t)j].first, order[(size_t)j - 1].first)];
    long long cells = 0;
    const int lev = lfd_cap_level(hist, budget, box.L, &cells, stats);
    if (n <= budget) {
        for (long long i = 0; i < n; ++i) keep_out[i] = i;
        return n;
    }
    std::vector<uint8_t> keep((size_t)n, 0);
    long long k = 0;
    for (long long a = 0; a < n; ++k) {
        const unsigned long long cell = lfd_cap_cell_key(order[(size_t)a].first, lev);
        long long b = a;
        unsigned long long best = ~0ull;
        for (; b < n && lfd_cap_cell_key(order[(size_t)b].first, lev) == cell; ++b) {
            const unsigned i = order[(size_t)b].second;
            uint32_t bits = 0u;
            if (err) std::memcpy(&bits, err + i, sizeof(bits));
            best = std::min(best, lfd_cap_pack(err ? lfd_cap_rank(bits) : 0u, i));
        }
        if (lfd_cap_pick((unsigned long long)k, (unsigned long long)budget, (unsigned long long)cells)) keep[(size_t)(best & 0xffffffffull)] = 1;
        a = b;
    }
    long long kept = 0;
    for (long long i = 0; i < n; ++i)
        if (keep[(size_t)i]) keep_out[kept++] = i;                         // (a pick too many would write behind the array: the sanitizer's to see)
    return kept;
}

// the rule as the header of the C-ABI words it, without a sort
static std::vector<long long> brute(const std::vector<float>& xyz, const float* err, long long n, long long m, double* stats) {
    float lo[3], hi[3];
    for (int c = 0; c < 3; ++c) { lo[c] = xyz[(size_t)c]; hi[c] = xyz[(size_t)c]; }
    for (long long i = 0; i < n; ++i)
        for (int c = 0; c < 3; ++c) { lo[c] = std::min(lo[c], xyz[(size_t)(3 * i + c)]); hi[c] = std::max(hi[c], xyz[(size_t)(3 * i + c)]); }
    double L = 0.0;
    for (int c = 0; c < 3; ++c) L = std::max(L, (double)hi[c] - (double)lo[c]);
    std::vector<unsigned long long> key((size_t)n, 0ull);
    for (long long i = 0; i < n; ++i) {
        for (int c = 0; c < 3; ++c) {
            unsigned long long q = 0;
            if (L > 0.0) {
                const double t = ((double)xyz[(size_t)(3 * i + c)] - (double)lo[c]) / L;
                const double u = t * 2097152.0;
                q = u >= 2097151.0 ? 2097151ull : (unsigned long long)std::floor(u);
            }
            for (int bit = 0; bit < 21; ++bit) key[(size_t)i] |= ((q >> bit) & 1ull) << (3 * bit + 2 - c);
        }
    }
    long long cells[22];
    for (int l = 0; l <= 21; ++l) {
        std::map<unsigned long long, int> seen;
        for (long long i = 0; i < n; ++i) seen[key[(size_t)i] >> (3 * (21 - l))] = 1;
        cells[l] = (long long)seen.size();
    }
    int lev = 21;
    for (int l = 21; l >= 0; --l)
        if (cells[l] >= m) lev = l;
    stats[0] = lev; stats[1] = (double)cells[lev]; stats[2] = lev > 0 ? (double)cells[lev - 1] : 0.0; stats[3] = L;
    std::vector<long long> out;
    if (n <= m) {
        for (long long i = 0; i < n; ++i) out.push_back(i);
        return out;
    }
    std::map<unsigned long long, long long> rep;                           // cell -> representative, cells in Morton order
    for (long long i = 0; i < n; ++i) {
        const unsigned long long cell = key[(size_t)i] >> (3 * (21 - lev));
        auto it = rep.find(cell);
        if (it == rep.end()) { rep[cell] = i; continue; }
        if (!err) continue;                                                // the lowest index came first
        uint32_t a, b;
        std::memcpy(&a, err + i, 4);
        std::memcpy(&b, err + it->second, 4);
        const long long ra = (a & 0x80000000u) ? -(long long)(a & 0x7fffffffu) - 1 : (long long)a;      // sign-magnitude to a signed order, -0 below +0
        const long long rb = (b & 0x80000000u) ? -(long long)(b & 0x7fffffffu) - 1 : (long long)b;
        if (ra < rb) it->second = i;
    }
    const long long c = cells[lev];
    long long k = 0;
    for (const auto& kv : rep) {
        const unsigned __int128 hi_q = ((unsigned __int128)(k + 1) * (unsigned __int128)m) / (unsigned __int128)c;
        const unsigned __int128 lo_q = ((unsigned __int128)k * (unsigned __int128)m) / (unsigned __int128)c;
        if (c < m || hi_q > lo_q) out.push_back(kv.second);
        ++k;
    }
    std::sort(out.begin(), out.end());
    return out;
}

static long long check(const char* name, const std::vector<float>& xyz, const std::vector<float>* err, long long m) {
    const long long n = (long long)(xyz.size() / 3);
    long long* keep = new long long[(size_t)std::min(m, n)];               // exactly the documented sizes, on the heap
    double* stats = new double[4];
    double want_stats[4];
    const long long kept = through_the_header(xyz, err ? err->data() : nullptr, n, m, keep, stats);
    const std::vector<long long> want = brute(xyz, err ? err->data() : nullptr, n, m, want_stats);
    long long bad = kept == (long long)want.size() ? 0 : 1;
    for (long long i = 0; i < std::min<long long>(kept, (long long)want.size()); ++i) bad += keep[i] == want[(size_t)i] ? 0 : 1;
    for (int s = 0; s < 4; ++s) bad += stats[s] == want_stats[s] ? 0 : 1;
    std::printf("%-14s n %6lld m %5lld kept %5lld level %2d cells %6d above %6d  %s\n", name, n, m, kept, (int)stats[0], (int)stats[1], (int)stats[2],
                bad ? "MISMATCH" : "ok");
    delete[] keep;
    delete[] stats;
    return bad;
}

int main() {
    std::mt19937 gen(7);
    std::uniform_real_distribution<float> uni(0.0f, 1.0f);
    std::normal_distribution<float> thin(0.0f, 0.002f);
    long long bad = 0;
    auto errors = [&](size_t n) {
        std::vector<float> e(n);
        for (float& v : e) v = std::floor(uni(gen) * 8.0f) / 8.0f;          // few values: ties in every cell
        return e;
    };

    // (c) 40 copies of one point among 60 others; 50 identical points
    std::vector<float> c1;
    for (int i = 0; i < 100; ++i) {
        const bool copy = i % 5 < 2;
        c1.push_back(copy ? 0.3f : 3.0f * uni(gen) - 1.0f); c1.push_back(copy ? -0.7f : 3.0f * uni(gen) - 1.0f); c1.push_back(copy ? 1.1f : 3.0f * uni(gen) - 1.0f);
    }
    std::vector<float> e1 = errors(100);
    e1[3] = -0.0f; e1[4] = std::numeric_limits<float>::quiet_NaN(); e1[8] = -std::numeric_limits<float>::quiet_NaN();
    for (long long m : {30, 80, 100, 101}) { bad += check("c-mixed", c1, &e1, m); bad += check("c-mixed-noerr", c1, nullptr, m); }
    std::vector<float> c2;
    for (int i = 0; i < 50; ++i) { c2.push_back(0.3f); c2.push_back(-0.7f); c2.push_back(1.1f); }
    std::vector<float> e2 = errors(50);
    bad += check("c-identical", c2, &e2, 10);
    bad += check("c-identical", c2, nullptr, 1);

    // (d) the 8 x 8 x 8 integer lattice: points on cell faces, the maximum corner at the clamp
    std::vector<float> d;
    for (int x = 0; x < 8; ++x)
        for (int y = 0; y < 8; ++y)
            for (int z = 0; z < 8; ++z) { d.push_back((float)x); d.push_back((float)y); d.push_back((float)z); }
    std::vector<float> ed = errors(512);
    for (long long m : {1, 7, 64, 100, 511}) bad += check("d-lattice", d, &ed, m);

    // (g) two densities side by side and a far outlier
    std::vector<float> g;
    for (int i = 0; i < 22000; ++i) {
        const bool sparse = i % 11 == 10;
        g.push_back(uni(gen) + (sparse ? 1.0f : 0.0f)); g.push_back(uni(gen)); g.push_back(thin(gen));
    }
    g.push_back(1000.0f); g.push_back(0.0f); g.push_back(0.0f);
    std::vector<float> eg = errors(22001);
    for (long long m : {1000, 257}) bad += check("g-two-density", g, &eg, m);
    bad += check("g-two-density", g, nullptr, 22000);

    std::printf("%s (%lld mismatches)\n", bad ? "FAILED" : "ok", bad);
    return bad ? 1 : 0;
}
