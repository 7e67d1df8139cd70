// Stand-alone host program around the routines of the epipolar audit (csrc/lfd_audit.hpp): lfd_far_confident and lfd_audit_bin exactly as the
// twin drives them, per cell and slot of a small three-camera scene whose arrays - certainties, warps, masks, the table [k][66], the cell map
// [H W] - are heap blocks of exactly the documented sizes.  The inputs include what the contract lists: NaN certainties, a certainty exactly
// at the threshold, NaN and infinite observations, observations outside the neighbour's grid, NaN A-coordinates (four-channel warps), a pair
// whose F has rows 0 and 1 zero, and values that overflow the f64 products.  Built with -fsanitize=address,undefined by
// tests/test_audit_sanitized.py and run on its own: a read or write outside an array, a signed overflow or an out-of-range conversion ends it
// with a report and a non-zero status; every table is compared with a second accumulation in the opposite order, and every bin with the plain
// count of thresholds the header defines it as.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "lfd_audit.hpp"

namespace {

constexpr int W_MATCH = 48, H_MATCH = 40, CAM_W = 640, CAM_H = 400, K = 3;

LfdCam make_cam(float cx_world, float yaw) {
    LfdCam c;
    const float f = 500.0f;
    const float Km[9] = {f, 0.0f, CAM_W / 2.0f, 0.0f, f, CAM_H / 2.0f, 0.0f, 0.0f, 1.0f};
    const float cs = std::cos(yaw), sn = std::sin(yaw);
    const float R[9] = {cs, 0.0f, -sn, 0.0f, 1.0f, 0.0f, sn, 0.0f, cs};
    float t[3];
    for (int r = 0; r < 3; ++r) t[r] = -(R[3 * r] * cx_world);
    for (int i = 0; i < 9; ++i) { c.K[i] = Km[i]; c.R[i] = R[i]; }
    for (int i = 0; i < 3; ++i) c.t[i] = t[i];
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

// the header's definition of the bin, term by term
int plain_bin(const double* F, double ua, double va, double ub, double vb) {
    const double l0 = (F[0] * ua + F[1] * va) + F[2], l1 = (F[3] * ua + F[4] * va) + F[5], l2 = (F[6] * ua + F[7] * va) + F[8];
    const double num = (ub * l0 + vb * l1) + l2, n2 = l0 * l0 + l1 * l1, num2 = num * num;
    if (!(std::isfinite(num2) && std::isfinite(n2) && n2 > 0.0)) return -1;
    int n = 0;
    for (int b = 0; b <= 62; ++b) n += num2 >= ((double)((b + 1) * (b + 1)) / 64.0) * n2 ? 1 : 0;
    return n;
}

// one reference's cells into `table` [K][66] and `best` [H W], visiting them forwards or backwards; returns the confident samples
long long audit(int H, int W, int C, bool masks, bool backwards, std::vector<uint64_t>& table, std::vector<uint8_t>& best) {
    const LfdCam a = make_cam(0.0f, 0.0f), b0 = make_cam(0.4f, 0.02f), b1 = make_cam(-0.3f, -0.03f), b2 = make_cam(0.8f, 0.0f);
    const LfdCam* nb[K] = {&b0, &b1, &b2};
    LfdPairConst pc[K];
    for (int j = 0; j < K; ++j) lfd_make_pair_const(a, *nb[j], j + 1, W_MATCH, H_MATCH, pc[j], nullptr);
    for (int e = 0; e < 6; ++e) pc[2].F[e] = 0.0;                      // rows 0 and 1 zero: every sample of the pair is degenerate
    LfdRefConst rc;
    lfd_make_ref_const(a, W_MATCH, H_MATCH, rc);
    float M[9];
    lfd_far_dir_matrix(a, M);
    const LfdAxis axx = lfd_make_axis(W), axy = lfd_make_axis(H);
    const size_t HW = (size_t)H * W;
    std::vector<float> cert[K], warp[K];
    std::vector<uint8_t> mask[K], mask_a((size_t)W_MATCH * H_MATCH, 1);
    for (int x = 0; x < W_MATCH; ++x) mask_a[(size_t)3 * W_MATCH + x] = 0;
    const float wm1 = (float)(W_MATCH - 1), hm1 = (float)(H_MATCH - 1);
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    for (int j = 0; j < K; ++j) {
        cert[j].resize(HW); warp[j].resize(HW * C);
        mask[j].assign((size_t)W_MATCH * H_MATCH, 1);
        for (int y = 0; y < H_MATCH; ++y) mask[j][(size_t)y * W_MATCH + 5 + j] = 0;
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const size_t cell = (size_t)y * W + x;
                const float xan = lfd_axis_value(axx, x), yan = lfd_axis_value(axy, y);
                float d[3];
                lfd_far_direction(M, rc.sx, rc.sy, xan, yan, wm1, hm1, d);
                const float s = 2.0f + 0.05f * (float)x;               // a point a few units along the ray
                const float X[3] = {a.C[0] + s * d[0], a.C[1] + s * d[1], a.C[2] + s * d[2]};
                const float* P = nb[j]->P;
                const float pz = P[8] * X[0] + P[9] * X[1] + P[10] * X[2] + P[11];
                const float u = (P[0] * X[0] + P[1] * X[1] + P[2] * X[2] + P[3]) / pz;
                const float v = (P[4] * X[0] + P[5] * X[1] + P[6] * X[2] + P[7]) / pz + 0.3f * (float)(cell % 30u);      // up to 8.7 px off the line
                float* wv = &warp[j][cell * C];
                if (C == 4) { wv[0] = xan; wv[1] = yan; }
                wv[C - 2] = u / pc[j].sx / (0.5f * wm1) - 1.0f;
                wv[C - 1] = v / pc[j].sy / (0.5f * hm1) - 1.0f;
                cert[j][cell] = 0.55f + 0.4f * (float)((cell * 7u + (unsigned)j) % 10u) / 10.0f;
            }
        cert[j][1] = nan; cert[j][2] = 0.0f; cert[j][3] = -inf; cert[j][11] = 0.5f; cert[j][12] = inf;
        warp[j][(size_t)4 * C + C - 2] = nan; warp[j][(size_t)5 * C + C - 1] = inf; warp[j][(size_t)6 * C + C - 2] = -3.0f;
        warp[j][(size_t)7 * C + C - 1] = 1.0e30f;
        if (C == 4 && j == 0) { warp[j][(size_t)8 * C] = nan; warp[j][(size_t)9 * C + 1] = inf; warp[j][(size_t)10 * C] = 3.0e38f; }
    }
    LfdSlot slot[K];
    for (int j = 0; j < K; ++j) lfd_slot_fill(slot[j], cert[j].data(), warp[j].data(), masks ? mask[j].data() : nullptr, pc[j]);
    LfdSupportGeom g;
    g.H = H; g.W = W; g.C = C; g.w_match = W_MATCH; g.h_match = H_MATCH; g.wm1 = wm1; g.hm1 = hm1;
    g.mask_sx = (float)W_MATCH / (float)W; g.mask_sy = (float)H_MATCH / (float)H; g.tau = 0.0f; g.reproj_thresh = 0.0f;
    long long n_conf = 0;
    for (size_t step = 0; step < HW; ++step) {
        const int cell = (int)(backwards ? HW - 1 - step : step);
        const int y = cell / W, x = cell - y * W;
        int bst = LFD_AUDIT_NONE;
        const bool ok = !masks || mask_a[(size_t)lfd_nearest_src(y, g.mask_sy, H_MATCH) * W_MATCH + lfd_nearest_src(x, g.mask_sx, W_MATCH)] != 0;
        if (ok) {
            float xan, yan;
            if (C == 4) { xan = slot[0].warp[(size_t)cell * 4]; yan = slot[0].warp[(size_t)cell * 4 + 1]; }
            else { xan = lfd_axis_value(axx, x); yan = lfd_axis_value(axy, y); }
            for (int j = 0; j < K; ++j) {
                const float* wv = slot[j].warp + (size_t)cell * C + (C - 2);
                if (!lfd_far_confident(slot[j], g, 0.5f, slot[j].cert[cell], wv[0], wv[1])) continue;
                ++n_conf;
                const int bin = lfd_audit_bin(pc[j].F, rc.sx, rc.sy, slot[j].sx, slot[j].sy, xan, yan, wv[0], wv[1], wm1, hm1);
                const int want = plain_bin(pc[j].F, (double)(lfd_match_px(xan, wm1) * rc.sx), (double)(lfd_match_px(yan, hm1) * rc.sy),
                                           (double)(lfd_match_px(wv[0], wm1) * slot[j].sx), (double)(lfd_match_px(wv[1], hm1) * slot[j].sy));
                expect(bin == want && bin >= -1 && bin < LFD_AUDIT_BINS, "bin equals the count of thresholds", bin, want);
                uint64_t* row = &table[(size_t)j * LFD_AUDIT_QUANTITIES];
                if (bin < 0) { row[1] += 1; continue; }
                row[0] += 1; row[2 + bin] += 1;
                bst = bin < bst ? bin : bst;
            }
        }
        best[(size_t)cell] = (uint8_t)bst;
    }
    return n_conf;
}

void run(int H, int W, int C, bool masks) {
    const size_t HW = (size_t)H * W;
    std::vector<uint64_t> fwd((size_t)K * LFD_AUDIT_QUANTITIES, 0), bwd((size_t)K * LFD_AUDIT_QUANTITIES, 0);
    std::vector<uint8_t> bf(HW, 7), bb(HW, 9);
    const long long n_f = audit(H, W, C, masks, false, fwd, bf), n_b = audit(H, W, C, masks, true, bwd, bb);
    expect(n_f == n_b && n_f > 0 && n_f < (long long)K * H * W, "confident samples", n_f, n_b);
    expect(std::memcmp(fwd.data(), bwd.data(), fwd.size() * 8) == 0, "order-free table", 0, 0);
    expect(std::memcmp(bf.data(), bb.data(), HW) == 0, "order-free cell map", 0, 0);
    long long total = 0, bins_used = 0;
    for (int j = 0; j < K; ++j) {
        const uint64_t* row = &fwd[(size_t)j * LFD_AUDIT_QUANTITIES];
        long long s = 0;
        for (int b = 0; b < LFD_AUDIT_BINS; ++b) { s += (long long)row[2 + b]; bins_used += row[2 + b] ? 1 : 0; }
        expect(s == (long long)row[0], "bins sum to the usable count", s, (long long)row[0]);
        total += (long long)(row[0] + row[1]);
    }
    expect(total == n_f, "usable + degenerate", total, n_f);
    expect(fwd[2 * LFD_AUDIT_QUANTITIES] == 0 && fwd[2 * LFD_AUDIT_QUANTITIES + 1] > 0, "the pair with the zeroed rows is degenerate", 0, 0);
    expect(bins_used > 40 && fwd[2 + 63] > 0, "the bins are used up to the last", bins_used, (long long)fwd[2 + 63]);
    // the extremes of the arithmetic: products that overflow f64 are degenerate, an exact zero is bin 0, the edges belong to the upper bin
    const double big[9] = {3.0e38, 3.0e38, 3.0e38, 3.0e38, 3.0e38, 3.0e38, 3.0e38, 3.0e38, 3.0e38};
    const double rows[9] = {0.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 1.0, 0.0};        // the line v = va: distance |vb - va|
    expect(lfd_audit_bin(big, 3.0e38f, 3.0e38f, 3.0e38f, 3.0e38f, 1.0f, 1.0f, 1.0f, 1.0f, 3.0e38f, 3.0e38f) == -1, "overflow is degenerate", 0, 0);
    for (int e = 0; e <= 70; ++e) {                                    // vb - va = e / 8 px exactly: bin min(e, 63)
        const float yb = -1.0f + 2.0f * (float)e / 8.0f;               // lfd_match_px(yb, 1) = e / 8
        const int bin = lfd_audit_bin(rows, 1.0f, 1.0f, 1.0f, 1.0f, -1.0f, -1.0f, 0.0f, yb, 1.0f, 1.0f);
        expect(bin == (e < 63 ? e : 63), "an edge belongs to the upper bin", bin, e);
    }
    std::printf("H %d W %d C %d masks %d: %lld confident samples, %lld bins used\n", H, W, C, (int)masks, n_f, bins_used);
}

}  // namespace

int main() {
    run(12, 16, 2, false);
    run(12, 16, 4, true);
    run(7, 9, 4, false);
    run(20, 24, 2, true);
    std::printf("ok (%d mismatches)\n", mismatches);
    return mismatches == 0 ? 0 : 1;
}
