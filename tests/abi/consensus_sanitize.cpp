// Stand-alone host program around the per-point routine of the consensus filter (csrc/lfd_consensus.hpp): the keys, the sort and
// lfd_consensus_count_point exactly as the twin drives them, on random clouds that include NaN and infinite coordinates, checked against a
// brute-force count.  Built with -fsanitize=address,undefined by tests/test_consensus_sanitized.py and run on its own: a read outside the sorted
// arrays, a signed overflow in the key offsets or an out-of-range conversion ends it with a report and a non-zero status.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <utility>
#include <vector>

#include "lfd_consensus.hpp"

static int brute(const std::vector<float>& xyz, const std::vector<int>& ref, long long i, float r2, int n_refs) {
    if (!lfd_consensus_finite(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2])) return 0;
    std::vector<char> seen((size_t)n_refs, 0);
    int c = 0;
    const long long n = (long long)ref.size();
    for (long long j = 0; j < n; ++j) {
        if (ref[j] == ref[i] || seen[(size_t)ref[j]]) continue;
        if (!lfd_consensus_finite(xyz[3 * j], xyz[3 * j + 1], xyz[3 * j + 2])) continue;
        if (lfd_consensus_agree(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], xyz[3 * j], xyz[3 * j + 1], xyz[3 * j + 2], r2)) { seen[(size_t)ref[j]] = 1; ++c; }
    }
    return std::min(c, LFD_CONSENSUS_CAP);
}

static int run_case(unsigned seed, long long n, int n_refs, float radius, float extent, bool clustered) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> uni(-extent, extent);
    std::normal_distribution<float> jitter(0.0f, radius);
    std::vector<float> xyz((size_t)(3 * n));
    std::vector<int> ref((size_t)n);
    std::vector<float> centres;
    for (int c = 0; c < 12; ++c) centres.push_back(uni(rng));
    for (long long i = 0; i < n; ++i) {
        ref[(size_t)i] = (int)((i * n_refs) / n);                        // grouped by reference, ascending
        for (int c = 0; c < 3; ++c)
            xyz[(size_t)(3 * i + c)] = clustered ? centres[(size_t)((rng() % 4) * 3 + c)] + jitter(rng) : uni(rng);
        const unsigned roll = rng() % 40;
        if (roll == 0) xyz[(size_t)(3 * i + (long long)(rng() % 3))] = std::numeric_limits<float>::quiet_NaN();
        if (roll == 1) xyz[(size_t)(3 * i + (long long)(rng() % 3))] = (rng() & 1) ? std::numeric_limits<float>::infinity() : -std::numeric_limits<float>::infinity();
    }
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long long i = 0; i < n; ++i) {
        if (!lfd_consensus_finite(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2])) continue;
        for (int c = 0; c < 3; ++c) { lo[c] = std::min(lo[c], xyz[3 * i + c]); hi[c] = std::max(hi[c], xyz[3 * i + c]); }
    }
    if (!(lo[0] <= hi[0])) return 0;
    LfdConsensusGrid g;
    if (!lfd_consensus_grid(lo, hi, radius, g)) { std::printf("seed %u: key range refused\n", seed); return 1; }
    std::vector<std::pair<unsigned long long, unsigned>> order((size_t)n);
    for (long long i = 0; i < n; ++i)
        order[(size_t)i] = {lfd_consensus_key(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], g.origin[0], g.origin[1], g.origin[2], g.h, g.e[1], g.e[2], g.sentinel),
                            (unsigned)i};
    std::sort(order.begin(), order.end());
    std::vector<unsigned long long> skey((size_t)n);
    std::vector<LfdConsensusPt> spt((size_t)n);
    for (long long j = 0; j < n; ++j) {
        const long long i = order[(size_t)j].second;
        skey[(size_t)j] = order[(size_t)j].first;
        spt[(size_t)j] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], ref[(size_t)i]};
    }
    const float r2 = lfd_consensus_r2(radius);
    int bad = 0;
    for (long long j = 0; j < n; ++j) {
        const long long i = order[(size_t)j].second;
        const int want = brute(xyz, ref, i, r2, n_refs);
        for (int bound = 1; bound <= LFD_CONSENSUS_CAP; bound += 7) {           // min_refs = 1 without the counts, and the full count
            int got = 0;
            if (skey[(size_t)j] != g.sentinel)
                got = lfd_consensus_count_point<LFD_CONSENSUS_CAP>(skey.data(), spt.data(), n, j, g.e[1], g.e[2], r2, bound);
            if (got != std::min(want, bound)) {
                if (bad < 5) std::printf("seed %u point %lld bound %d: got %d, brute force %d\n", seed, i, bound, got, want);
                ++bad;
            }
        }
    }
    return bad;
}

int main() {
    int bad = 0;
    bad += run_case(1, 1500, 7, 0.05f, 1.0f, false);
    bad += run_case(2, 1500, 12, 0.2f, 1.0f, false);
    bad += run_case(3, 1200, 9, 0.01f, 50.0f, true);
    bad += run_case(4, 800, 3, 5.0f, 1.0f, false);            // everybody in one cell
    bad += run_case(5, 1000, 20, 1e-3f, 300.0f, true);         // large keys: 2e17 cells
    bad += run_case(6, 1, 1, 1.0f, 1.0f, false);
    std::printf(bad ? "FAILED: %d mismatches\n" : "ok (%d mismatches)\n", bad);
    return bad ? 1 : 0;
}
