// Stand-alone host program around the twin of the footprint-adaptive thinning (csrc/lfd_thin.hpp): lfd_thin_check and lfd_thin_walk - the very
// routine lfd_thin_footprint_host runs behind its context checks - driven into heap arrays of exactly the documented sizes (n indices, n_refs + 1
// offsets, 43 statistics) on clouds with duplicates, an empty reference in the middle and at the end, points behind their camera, identical
// points, a single point, and footprints that put every point on level 0 or on level 20, checked element for element against a loop that knows
// nothing of the sort: cells in an ordered map, the key's bits interleaved one by one, the level from frexp.  Built with
// -fsanitize=address,undefined by tests/test_thin_sanitized.py and run on its own: a read outside the cloud, a write behind the outputs, a shift
// beyond the word or an out-of-range conversion ends it with a report and a non-zero status.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <random>
#include <utility>
#include <vector>

#include "lfd_thin.hpp"

struct Want {
    std::vector<long long> keep, offs;
    double stats[LFD_THIN_STATS];
};

// the rule as the header of the C-ABI words it, without a sort
static Want brute(const std::vector<float>& xyz, const float* err, const std::vector<int64_t>& offs, const std::vector<double>& rows, double thin_cells) {
    const long long n = (long long)(xyz.size() / 3);
    const int n_refs = (int)offs.size() - 1;
    Want w;
    for (double& s : w.stats) s = 0.0;
    float lo[3], hi[3];
    for (int c = 0; c < 3; ++c) { lo[c] = xyz[(size_t)c]; hi[c] = xyz[(size_t)c]; }
    for (long long i = 0; i < n; ++i)
        for (int c = 0; c < 3; ++c) { lo[c] = std::min(lo[c], xyz[(size_t)(3 * i + c)]); hi[c] = std::max(hi[c], xyz[(size_t)(3 * i + c)]); }
    double L = 0.0;
    for (int c = 0; c < 3; ++c) L = std::max(L, (double)hi[c] - (double)lo[c]);
    std::map<unsigned long long, std::pair<long long, long long>> best;        // code -> (signed error order, index)
    for (int r = 0; r < n_refs; ++r)
        for (long long i = offs[(size_t)r]; i < offs[(size_t)r + 1]; ++i) {
            unsigned long long key = 0ull;
            for (int c = 0; c < 3; ++c) {
                unsigned long long q = 0;
                if (L > 0.0) {
                    const double t = ((double)xyz[(size_t)(3 * i + c)] - (double)lo[c]) / L;
                    const double u = t * 2097152.0;
                    q = u >= 2097151.0 ? 2097151ull : (unsigned long long)std::floor(u);
                }
                for (int bit = 0; bit < 21; ++bit) key |= ((q >> bit) & 1ull) << (3 * bit + 2 - c);
            }
            const double* row = rows.data() + 5 * (size_t)r;
            const double px = row[0] * (double)xyz[(size_t)(3 * i)];
            const double py = row[1] * (double)xyz[(size_t)(3 * i + 1)];
            const double pz = row[2] * (double)xyz[(size_t)(3 * i + 2)];
            const double s0 = px + py;
            const double s1 = s0 + pz;
            const double z = s1 + row[3];
            const double a = z * row[4];
            const double g = a * thin_cells;
            int lev = 20;
            if (g > 0.0 && !std::isinf(g) && L > 0.0) {
                const double q = L / g;
                if (q < 1.0) lev = 0;
                else if (std::isinf(q)) lev = 20;
                else {
                    int e = 0;
                    (void)std::frexp(q, &e);                                   // q = m 2^e with m in [0.5, 1): the binary exponent is e - 1
                    lev = std::min(e - 1, 20);
                }
            }
            w.stats[lev] += 1.0;
            unsigned long long code = 1ull;
            for (int l = 0; l < lev; ++l) code = (code << 3) | ((key >> (3 * (20 - l))) & 7ull);
            long long order = 0;
            if (err) {
                uint32_t b;
                std::memcpy(&b, err + i, 4);
                order = (b & 0x80000000u) ? -(long long)(b & 0x7fffffffu) - 1 : (long long)b;
            }
            auto it = best.find(code);
            if (it == best.end()) { best[code] = {order, i}; w.stats[21 + lev] += 1.0; }
            else if (std::make_pair(order, i) < it->second) it->second = {order, i};
        }
    for (const auto& kv : best) w.keep.push_back(kv.second.second);
    std::sort(w.keep.begin(), w.keep.end());
    for (int r = 0; r <= n_refs; ++r)
        w.offs.push_back((long long)(std::lower_bound(w.keep.begin(), w.keep.end(), (long long)offs[(size_t)r]) - w.keep.begin()));
    w.stats[42] = L;
    return w;
}

static long long check(const char* name, const std::vector<float>& xyz, const std::vector<float>* err, const std::vector<int64_t>& offs,
                       const std::vector<double>& rows, double thin_cells) {
    const long long n = (long long)(xyz.size() / 3);
    const int n_refs = (int)offs.size() - 1;
    int64_t* keep = new int64_t[(size_t)n];                                    // exactly the documented sizes, on the heap
    int64_t* offs_out = new int64_t[(size_t)n_refs + 1];
    double* stats = new double[LFD_THIN_STATS];
    int64_t n_keep = 0;
    long long bad = 0;
    const char* why = lfd_thin_check(xyz.data(), err ? err->data() : nullptr, n, offs.data(), n_refs, rows.data(), thin_cells, keep, &n_keep, offs_out);
    if (why) { std::printf("%-16s refused: %s\n", name, why); bad = 1; }
    const long long kept = why ? 0 : lfd_thin_walk(xyz.data(), err ? err->data() : nullptr, n, offs.data(), n_refs, rows.data(), thin_cells, keep, offs_out, stats);
    if (!why) {
        const Want want = brute(xyz, err ? err->data() : nullptr, offs, rows, thin_cells);
        bad += kept == (long long)want.keep.size() ? 0 : 1;
        for (long long i = 0; i < std::min<long long>(kept, (long long)want.keep.size()); ++i) bad += keep[i] == want.keep[(size_t)i] ? 0 : 1;
        for (int r = 0; r <= n_refs; ++r) bad += offs_out[r] == want.offs[(size_t)r] ? 0 : 1;
        for (int s = 0; s < LFD_THIN_STATS; ++s) bad += stats[s] == want.stats[s] ? 0 : 1;
        int levels = 0;
        for (int l = 0; l < 21; ++l) levels += stats[l] > 0.0 ? 1 : 0;
        std::printf("%-16s n %6lld refs %3d cells %-8g kept %6lld levels in use %2d  %s\n", name, n, n_refs, thin_cells, kept, levels, bad ? "MISMATCH" : "ok");
    }
    delete[] keep;
    delete[] offs_out;
    delete[] stats;
    return bad;
}

int main() {
    std::mt19937 gen(11);
    std::uniform_real_distribution<float> uni(0.0f, 1.0f);
    std::normal_distribution<double> nrm(0.0, 1.0);
    long long bad = 0;
    auto errors = [&](size_t n) {
        std::vector<float> e(n);
        for (float& v : e) v = std::floor(uni(gen) * 8.0f) / 8.0f;              // few values: ties in every cell
        return e;
    };
    auto cameras = [&](int n_refs) {
        std::vector<double> rows;
        for (int r = 0; r < n_refs; ++r) {
            double a[3] = {nrm(gen), nrm(gen), nrm(gen)};
            const double len = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
            for (double v : a) rows.push_back(v / len);
            rows.push_back(4.0 + 6.0 * uni(gen));                               // some points end up behind their camera
            rows.push_back(0.004 + 0.016 * uni(gen));
        }
        return rows;
    };

    // 3 000 points with some 50 copies of one, five references of which the third and the last are empty
    std::vector<float> a;
    for (int i = 0; i < 3000; ++i) {
        const bool copy = i % 75 < 1 || i < 10;
        a.push_back(copy ? 0.3f : 8.0f * uni(gen) - 3.0f); a.push_back(copy ? -0.7f : 8.0f * uni(gen) - 4.0f); a.push_back(copy ? 1.1f : 8.0f * uni(gen) - 4.0f);
    }
    std::vector<float> ea = errors(3000);
    ea[3] = -0.0f; ea[4] = std::numeric_limits<float>::quiet_NaN(); ea[8] = -std::numeric_limits<float>::quiet_NaN();
    const std::vector<int64_t> offs_a = {0, 700, 1900, 1900, 3000, 3000};
    const std::vector<double> rows_a = cameras(5);
    for (double cells : {0.5, 2.0, 7.0, 1e12, 1e-12}) { bad += check("mixed", a, &ea, offs_a, rows_a, cells); bad += check("mixed-noerr", a, nullptr, offs_a, rows_a, cells); }

    // identical points and a single point: no extent
    std::vector<float> same;
    for (int i = 0; i < 50; ++i) { same.push_back(0.3f); same.push_back(-0.7f); same.push_back(1.1f); }
    std::vector<float> es = errors(50);
    bad += check("identical", same, &es, {0, 20, 50}, cameras(2), 2.0);
    bad += check("one-point", {1.0f, 2.0f, 3.0f}, nullptr, {0, 1}, cameras(1), 2.0);

    // the 8 x 8 x 8 integer lattice: points on cell faces, the maximum corner at the key's clamp; depth = the z coordinate, -1 .. 6: two layers
    // lie behind the camera or in its plane
    std::vector<float> d;
    for (int x = 0; x < 8; ++x)
        for (int y = 0; y < 8; ++y)
            for (int z = 0; z < 8; ++z) { d.push_back((float)x); d.push_back((float)y); d.push_back((float)z - 1.0f); }
    std::vector<float> ed = errors(512);
    for (double cells : {1.0, 64.0, 7.0 / 2097152.0}) bad += check("lattice", d, &ed, {0, 512}, {0.0, 0.0, 1.0, 0.0, 0.125}, cells);

    std::printf("%s (%lld mismatches)\n", bad ? "FAILED" : "ok", bad);
    return bad ? 1 : 0;
}
