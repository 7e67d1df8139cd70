// Stand-alone host program around the routines of the per-image exposure gains (csrc/lfd_gain.hpp): lfd_gain_sample and the quantisation
// exactly as the twin drives them, per (cell, slot) of a small three-camera scene whose arrays - certainties, warps, masks, images, the
// table - are heap blocks of exactly the documented sizes, and lfd_gain_value over a colour array of exactly 3 n values.  The inputs include
// what the contract lists: observations off the image (border taps), a NaN observation of the winning slot, certainties of zero, colours
// outside [0.05, 0.95] on either side, clipped image values, non-finite colours for the apply.  Built with -fsanitize=address,undefined by
// tests/test_gain_sanitized.py and run on its own: a read outside an array, a signed overflow or an out-of-range float-to-integer
// conversion ends it with a report and a non-zero status; every sum is compared with a plain loop that calls the colour stage's routines
// itself and quantises in double precision.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "lfd_gain.hpp"

namespace {

constexpr int W_MATCH = 96, H_MATCH = 80, CAM_W = 1297, CAM_H = 840, K = 2;

LfdCam make_cam(float cx_world) {
    LfdCam c;
    const float f = 960.0f;
    const float Km[9] = {f, 0.0f, CAM_W / 2.0f, 0.0f, f, CAM_H / 2.0f, 0.0f, 0.0f, 1.0f};
    const float R[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    const float t[3] = {-cx_world, 0.0f, 0.0f};
    for (int i = 0; i < 9; ++i) { c.K[i] = Km[i]; c.R[i] = R[i]; }
    for (int i = 0; i < 3; ++i) { c.t[i] = t[i]; }
    for (int r = 0; r < 3; ++r)
        for (int col = 0; col < 4; ++col) {
            float v = 0.0f;
            for (int e = 0; e < 3; ++e) v += Km[3 * r + e] * (col < 3 ? R[3 * e + col] : t[e]);
            c.P[4 * r + col] = v;
        }
    c.C[0] = cx_world; c.C[1] = 0.0f; c.C[2] = 0.0f;
    c.w = CAM_W; c.h = CAM_H; c.pad[0] = c.pad[1] = 0;
    return c;
}

int mismatches = 0;

void expect(bool ok, const char* what, long long a, long long b) {
    if (!ok) { ++mismatches; std::printf("MISMATCH %s: %lld / %lld\n", what, a, b); }
}

void run_grid(int H, int W, int C, bool masks) {
    const LfdCam a = make_cam(0.0f), b0 = make_cam(0.6f), b1 = make_cam(-0.5f);
    const LfdCam* nb[K] = {&b0, &b1};
    LfdPairConst pc[K];
    lfd_make_pair_const(a, b0, 1, W_MATCH, H_MATCH, pc[0], nullptr);
    lfd_make_pair_const(a, b1, 2, W_MATCH, H_MATCH, pc[1], nullptr);
    const LfdAxis axx = lfd_make_axis(W), axy = lfd_make_axis(H);
    const size_t HW = (size_t)H * W;
    std::vector<float> cert[K], warp[K], xyz(HW * 3), rgb(HW * 3);
    std::vector<uint8_t> image[K], mask[K];
    for (int j = 0; j < K; ++j) {
        cert[j].resize(HW); warp[j].resize(HW * C);
        image[j].resize((size_t)W_MATCH * H_MATCH * 3);
        mask[j].assign((size_t)W_MATCH * H_MATCH, 1);
        for (size_t p = 0; p < image[j].size(); ++p) image[j][p] = (uint8_t)((p * 37u + (unsigned)j * 101u + (p / 3) * 5u) & 255u);   // 0 .. 255: both ends clip
        for (int y = 0; y < H_MATCH; ++y)
            for (int x = 20 + 10 * j; x < 30 + 10 * j; ++x) mask[j][(size_t)y * W_MATCH + x] = 0;
    }
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const double ua = ((double)lfd_axis_value(axx, x) + 1.0) * 0.5 * (W_MATCH - 1) * ((double)CAM_W / W_MATCH);
            const double va = ((double)lfd_axis_value(axy, y) + 1.0) * 0.5 * (H_MATCH - 1) * ((double)CAM_H / H_MATCH);
            const double dx = (ua - a.K[2]) / a.K[0], dy = (va - a.K[5]) / a.K[4];
            const double z = 4.0 / (1.0 - 0.5 * dy);
            const double X[3] = {dx * z, dy * z, z};
            const size_t q = (size_t)y * W + x;
            for (int e = 0; e < 3; ++e) xyz[3 * q + e] = (float)X[e];
            // the colour the point carries: mostly in range, some values below 0.05, above 0.95 and exactly on the limits
            for (int e = 0; e < 3; ++e) rgb[3 * q + e] = 0.03f + 0.94f * (float)((q * 7 + e * 3) % 17) / 16.0f;
            if (q % 11 == 0) rgb[3 * q] = 0.05f;
            if (q % 13 == 0) rgb[3 * q + 1] = 0.95f;
            for (int j = 0; j < K; ++j) {
                const double xc = X[0] - nb[j]->C[0];
                const double ub = nb[j]->K[0] * xc / z + nb[j]->K[2], vb = nb[j]->K[4] * X[1] / z + nb[j]->K[5];
                float* w = &warp[j][q * C];
                if (C == 4) { w[0] = lfd_axis_value(axx, x); w[1] = lfd_axis_value(axy, y); }
                w[C - 2] = (float)(2.0 * (ub / ((double)CAM_W / W_MATCH)) / (W_MATCH - 1) - 1.0);
                w[C - 1] = (float)(2.0 * (vb / ((double)CAM_H / H_MATCH)) / (H_MATCH - 1) - 1.0);
                cert[j][q] = (q % 5 == (size_t)j) ? 0.0f : 0.6f;
                if (q % 17 == 3) w[C - 1] += 0.2f;                     // disagrees with X: not a candidate
                if (q % 19 == 4) { w[C - 2] = 1.7f; }                  // off the image: the winner still samples the border
                if (q % 23 == 5) w[C - 2] = nan;
            }
        }
    LfdSupportGeom g;
    g.H = H; g.W = W; g.C = C; g.w_match = W_MATCH; g.h_match = H_MATCH;
    g.wm1 = (float)(W_MATCH - 1); g.hm1 = (float)(H_MATCH - 1);
    g.mask_sx = (float)W_MATCH / (float)W; g.mask_sy = (float)H_MATCH / (float)H;
    g.tau = 1.6f; g.reproj_thresh = 0.0f;
    LfdSlot sl[K];
    for (int j = 0; j < K; ++j) lfd_slot_fill(sl[j], cert[j].data(), warp[j].data(), masks ? mask[j].data() : nullptr, pc[j]);
    std::vector<uint64_t> table((size_t)K * LFD_GAIN_QUANTITIES, 0), want((size_t)K * LFD_GAIN_QUANTITIES, 0);      // exactly [k][7]
    long long parts = 0, dropped = 0;
    for (size_t q = 0; q < HW; ++q) {
        const int cell = (int)q, s = (int)(q & 1);
        const float X0 = xyz[3 * q], X1 = xyz[3 * q + 1], X2 = xyz[3 * q + 2];
        const float* c = &rgb[3 * q];
        if (lfd_colour_guarded(X0, X1, X2, c[0], c[1], c[2], cell, (long long)HW, s, K)) { expect(false, "guarded", cell, 0); continue; }
        const bool ref_ok = lfd_gain_in_range(c[0]) && lfd_gain_in_range(c[1]) && lfd_gain_in_range(c[2]);
        for (int j = 0; j < K; ++j) {
            const float* wv = sl[j].warp + q * C + (C - 2);
            uint32_t qn[3];
            if (lfd_gain_sample(sl[j], image[j].data(), g, j == s, ref_ok, sl[j].cert[q], wv[0], wv[1], X0, X1, X2, qn)) {
                uint64_t* t = &table[(size_t)j * LFD_GAIN_QUANTITIES];
                t[0] += 1;
                for (int e = 0; e < 3; ++e) { t[1 + e] += lfd_gain_quantise(c[e]); t[4 + e] += qn[e]; }
            }
            // the plain loop: the colour stage's own routines, the limits as decimal comparisons in double, the quantisation in double
            const bool part = (j == s) ? (std::isfinite(wv[0]) && std::isfinite(wv[1]))
                                       : lfd_support_candidate(sl[j], g, sl[j].cert[q], wv[0], wv[1], X0, X1, X2);
            if (!part) continue;
            ++parts;
            float v[3];
            lfd_colour_sample(image[j].data(), g, wv[0], wv[1], v);
            bool ok = true;
            for (int e = 0; e < 3; ++e) ok = ok && c[e] >= 0.05f && c[e] <= 0.95f && v[e] >= 0.05f && v[e] <= 0.95f;
            if (!ok) { ++dropped; continue; }
            uint64_t* t = &want[(size_t)j * LFD_GAIN_QUANTITIES];
            t[0] += 1;
            for (int e = 0; e < 3; ++e) {
                t[1 + e] += (uint64_t)std::floor((double)c[e] * 16777216.0);
                t[4 + e] += (uint64_t)std::floor((double)v[e] * 16777216.0);
            }
        }
    }
    for (size_t t = 0; t < table.size(); ++t) expect(table[t] == want[t], "table", (long long)table[t], (long long)want[t]);
    expect(parts > 0 && dropped > 0 && (long long)(want[0] + want[LFD_GAIN_QUANTITIES]) > 0 && parts > dropped, "both kinds of sample", parts, dropped);

    // the apply rule over exactly 3 n values, in place and apart
    std::vector<float> out(HW * 3), in_place(rgb);
    const float inf = std::numeric_limits<float>::infinity();
    in_place[0] = nan; in_place[1] = inf; in_place[2] = -inf; in_place[3] = -0.5f; in_place[4] = 0.9f;
    const std::vector<float> src(in_place);
    const float f[3] = {1.25f, 0.8f, 4.0f};
    for (size_t e = 0; e < src.size(); ++e) out[e] = lfd_gain_value(src[e], f[e % 3]);
    for (size_t e = 0; e < in_place.size(); ++e) in_place[e] = lfd_gain_value(in_place[e], f[e % 3]);
    expect(std::memcmp(out.data(), in_place.data(), out.size() * sizeof(float)) == 0, "in place", 0, 0);
    for (size_t e = 0; e < src.size(); ++e) {
        float w = src[e];
        if (std::isfinite(w)) { w = w * f[e % 3]; if (!(w < 1.0f)) w = 1.0f; }
        expect(std::memcmp(&w, &out[e], sizeof(float)) == 0, "apply", (long long)e, 0);
    }
    expect(out[4] == 0.9f * 0.8f && out[3] == -0.5f * 1.25f && out[5] <= 1.0f, "apply values", 0, 0);
}

}  // namespace

int main() {
    run_grid(20, 24, 2, false);
    run_grid(20, 24, 4, true);
    run_grid(6, 8, 2, true);
    run_grid(3, 2, 4, false);
    std::printf("ok (%d mismatches)\n", mismatches);
    return mismatches ? 1 : 0;
}
