// Stand-alone host program around the shared routines of the component filter (csrc/lfd_component.hpp): the keys, the sort, lfd_component_links
// and lfd_component_unite / lfd_component_find exactly as the twin drives them, on random clouds that include NaN and infinite coordinates,
// checked against a brute-force partition (every pair, a breadth-first search).  Built with -fsanitize=address,undefined by
// tests/test_component_sanitized.py and run on its own: a read outside the sorted arrays or parent[], a signed overflow in the key offsets or
// an out-of-range conversion ends it with a report and a non-zero status.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <utility>
#include <vector>

#include "lfd_component.hpp"

// label (smallest index of the component) of every point, from all pairs
static std::vector<uint32_t> brute(const std::vector<float>& xyz, long long n, float r2) {
    std::vector<uint32_t> label((size_t)n, 0xffffffffu);
    std::vector<long long> queue;
    for (long long s = 0; s < n; ++s) {
        if (label[(size_t)s] != 0xffffffffu) continue;
        label[(size_t)s] = (uint32_t)s;                                  // s is the smallest index not reached yet
        queue.assign(1, s);
        while (!queue.empty()) {
            const long long i = queue.back();
            queue.pop_back();
            if (!lfd_consensus_finite(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2])) continue;
            for (long long j = 0; j < n; ++j) {
                if (label[(size_t)j] != 0xffffffffu || !lfd_consensus_finite(xyz[3 * j], xyz[3 * j + 1], xyz[3 * j + 2])) continue;
                if (!lfd_consensus_agree(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], xyz[3 * j], xyz[3 * j + 1], xyz[3 * j + 2], r2)) continue;
                label[(size_t)j] = (uint32_t)s;
                queue.push_back(j);
            }
        }
    }
    return label;
}

template <bool SHORTEN>
static int run_case(unsigned seed, long long n, float radius, float extent, bool clustered) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> uni(-extent, extent);
    std::normal_distribution<float> jitter(0.0f, radius);
    std::vector<float> xyz((size_t)(3 * n));
    std::vector<float> centres;
    for (int c = 0; c < 12; ++c) centres.push_back(uni(rng));
    for (long long i = 0; i < n; ++i) {
        for (int c = 0; c < 3; ++c)
            xyz[(size_t)(3 * i + c)] = clustered ? centres[(size_t)((rng() % 4) * 3 + c)] + jitter(rng) : uni(rng);
        const unsigned roll = rng() % 40;
        if (roll == 0) xyz[(size_t)(3 * i + (long long)(rng() % 3))] = std::numeric_limits<float>::quiet_NaN();
        if (roll == 1) xyz[(size_t)(3 * i + (long long)(rng() % 3))] = (rng() & 1) ? std::numeric_limits<float>::infinity() : -std::numeric_limits<float>::infinity();
        if (seed == 7) for (int c = 0; c < 3; ++c) xyz[(size_t)(3 * i + c)] = std::numeric_limits<float>::quiet_NaN();      // no finite point at all
    }
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long long i = 0; i < n; ++i) {
        if (!lfd_consensus_finite(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2])) continue;
        for (int c = 0; c < 3; ++c) { lo[c] = std::min(lo[c], xyz[3 * i + c]); hi[c] = std::max(hi[c], xyz[3 * i + c]); }
    }
    LfdConsensusGrid g;
    if (!lfd_component_grid(lo, hi, radius, g)) { std::printf("seed %u: key range refused\n", seed); return 1; }
    std::vector<std::pair<unsigned long long, unsigned>> order((size_t)n);
    for (long long i = 0; i < n; ++i)
        order[(size_t)i] = {lfd_consensus_key(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], g.origin[0], g.origin[1], g.origin[2], g.h, g.e[1], g.e[2], g.sentinel),
                            (unsigned)i};
    std::sort(order.begin(), order.end());
    std::vector<unsigned long long> skey((size_t)n);
    std::vector<LfdComponentPt> spt((size_t)n);
    std::vector<uint32_t> parent((size_t)n);
    for (long long j = 0; j < n; ++j) {
        const long long i = order[(size_t)j].second;
        skey[(size_t)j] = order[(size_t)j].first;
        spt[(size_t)j] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], (uint32_t)i};
        parent[(size_t)j] = (uint32_t)j;
    }
    const float r2 = lfd_consensus_r2(radius);
    long long links = 0;
    for (long long j = 0; j < n && skey[(size_t)j] != g.sentinel; ++j) {
        uint32_t mine = (uint32_t)j;
        lfd_component_links(skey.data(), spt.data(), j, g.e[1], g.e[2], r2, [&](uint32_t q) {
            ++links;
            mine = lfd_component_unite<LfdComponentSeq, SHORTEN>(parent.data(), mine, q);
        });
    }
    int bad = 0;
    for (long long j = 0; j < n; ++j)
        if (parent[(size_t)j] > (uint32_t)j) { ++bad; std::printf("seed %u: parent[%lld] = %u is above it\n", seed, j, parent[(size_t)j]); }
    std::vector<uint32_t> first((size_t)n, 0xffffffffu), count((size_t)n, 0u), root((size_t)n);
    int64_t summary[LFD_COMPONENT_SUMMARY] = {0};
    for (long long j = 0; j < n; ++j) {
        const uint32_t r = lfd_component_find<LfdComponentSeq>(parent.data(), (uint32_t)j);
        root[(size_t)j] = r;
        count[r] += 1u;
        first[r] = std::min(first[r], spt[(size_t)j].idx);
    }
    const std::vector<uint32_t> want = brute(xyz, n, r2);
    std::vector<uint32_t> want_size((size_t)n, 0u);
    for (long long i = 0; i < n; ++i) want_size[want[(size_t)i]] += 1u;
    long long pairs = 0;
    for (long long i = 0; i < n; ++i)
        for (long long k = i + 1; k < n; ++k)
            pairs += lfd_consensus_finite(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]) && lfd_consensus_finite(xyz[3 * k], xyz[3 * k + 1], xyz[3 * k + 2]) &&
                     lfd_consensus_agree(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], xyz[3 * k], xyz[3 * k + 1], xyz[3 * k + 2], r2);
    if (pairs != links) { ++bad; std::printf("seed %u: the walk found %lld links, all pairs %lld\n", seed, links, pairs); }      // every pair once
    int64_t total = 0;
    for (long long j = 0; j < n; ++j) {
        const uint32_t r = root[(size_t)j], i = spt[(size_t)j].idx;
        if (first[r] != want[i] || count[r] != want_size[want[i]]) {
            if (bad < 5) std::printf("seed %u point %u: label %u size %u, brute force %u %u\n", seed, i, first[r], count[r], want[i], want_size[want[i]]);
            ++bad;
        }
        if (r == (uint32_t)j) lfd_component_summary_add(summary, count[r]);
    }
    for (int b = 0; b < LFD_COMPONENT_BINS; ++b) total += summary[2 + LFD_COMPONENT_BINS + b];
    if (total != n) { ++bad; std::printf("seed %u: the summary holds %lld of %lld points\n", seed, (long long)total, n); }
    return bad;
}

int main() {
    int bad = 0;
    bad += run_case<true>(1, 1500, 0.05f, 1.0f, false);
    bad += run_case<false>(1, 1500, 0.05f, 1.0f, false);
    bad += run_case<true>(2, 1500, 0.2f, 1.0f, false);
    bad += run_case<true>(3, 1200, 0.01f, 50.0f, true);
    bad += run_case<false>(3, 1200, 0.01f, 50.0f, true);
    bad += run_case<true>(4, 800, 5.0f, 1.0f, false);             // everybody in one cell
    bad += run_case<true>(5, 1000, 1e-3f, 300.0f, true);          // large keys: 2e17 cells
    bad += run_case<true>(6, 1, 1.0f, 1.0f, false);
    bad += run_case<true>(7, 50, 1.0f, 1.0f, false);              // no finite point: the empty grid
    std::printf(bad ? "FAILED: %d mismatches\n" : "ok (%d mismatches)\n", bad);
    return bad ? 1 : 0;
}
