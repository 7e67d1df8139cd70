// Stand-alone host program around the routines of the pose refinement (csrc/lfd_pose.hpp): lfd_pose_make_const, lfd_far_confident,
// lfd_pose_sample and lfd_pose_term exactly as the twin drives them, per cell and slot of a small four-camera scene whose arrays -
// certainties, warps, masks, the table [k][32] - are heap blocks of exactly the documented sizes.  The inputs include what the contract lists:
// NaN certainties, a certainty exactly at the threshold, NaN and infinite observations, observations outside the neighbour's grid, NaN
// A-coordinates (four-channel warps), a pair with coincident centres, values that overflow the f64 products, and residuals on both sides of
// and exactly at pose_inlier_px.  Built with -fsanitize=address,undefined by tests/test_pose_abi.py and run on its own: a read or write
// outside an array, a signed overflow or an out-of-range conversion to an integer ends it with a report and a non-zero status; every table
// is compared with a second accumulation in the opposite order, and every quantised value with the bounds the header derives.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "lfd_pose.hpp"

namespace {

constexpr int W_MATCH = 48, H_MATCH = 40, CAM_W = 640, CAM_H = 400, K = 4;

LfdCam make_cam(float cx, float cy, float cz, float yaw, float pitch) {
    LfdCam c;
    const float f = 500.0f;
    const float Km[9] = {f, 0.0f, CAM_W / 2.0f, 0.0f, f, CAM_H / 2.0f, 0.0f, 0.0f, 1.0f};
    const float cs = std::cos(yaw), sn = std::sin(yaw), cp = std::cos(pitch), sp = std::sin(pitch);
    const float Ry[9] = {cs, 0.0f, -sn, 0.0f, 1.0f, 0.0f, sn, 0.0f, cs}, Rx[9] = {1.0f, 0.0f, 0.0f, 0.0f, cp, -sp, 0.0f, sp, cp};
    float R[9];
    for (int r = 0; r < 3; ++r)
        for (int col = 0; col < 3; ++col) R[3 * r + col] = Rx[3 * r] * Ry[col] + Rx[3 * r + 1] * Ry[3 + col] + Rx[3 * r + 2] * Ry[6 + col];
    const float Cw[3] = {cx, cy, cz};
    float t[3];
    for (int r = 0; r < 3; ++r) t[r] = -(R[3 * r] * Cw[0] + R[3 * r + 1] * Cw[1] + R[3 * r + 2] * Cw[2]);
    for (int i = 0; i < 9; ++i) { c.K[i] = Km[i]; c.R[i] = R[i]; }
    for (int i = 0; i < 3; ++i) { c.t[i] = t[i]; c.C[i] = Cw[i]; }
    for (int r = 0; r < 3; ++r)
        for (int col = 0; col < 4; ++col) {
            float v = 0.0f;
            for (int e = 0; e < 3; ++e) v += Km[3 * r + e] * (col < 3 ? R[3 * e + col] : t[e]);
            c.P[4 * r + col] = v;
        }
    c.w = CAM_W; c.h = CAM_H; c.pad[0] = c.pad[1] = 0;
    return c;
}

int mismatches = 0;

void expect(bool ok, const char* what, long long a, long long b) {
    if (!ok) { ++mismatches; std::printf("MISMATCH %s: %lld / %lld\n", what, a, b); }
}

// one reference's cells into `table` [K][32], visiting them forwards or backwards; returns the confident samples
long long accumulate(int H, int W, int C, bool masks, bool backwards, float inlier_px, std::vector<int64_t>& table) {
    // the reference stands at the origin (t = 0), and so does the last neighbour: a pair with coincident centres
    const LfdCam a = make_cam(0.0f, 0.0f, 0.0f, 0.0f, 0.0f), b0 = make_cam(0.4f, 0.05f, 0.02f, 0.02f, 0.01f),
                 b1 = make_cam(-0.3f, -0.04f, 0.06f, -0.03f, 0.015f), b2 = make_cam(0.8f, 0.1f, -0.05f, 0.0f, -0.02f),
                 b3 = make_cam(0.0f, 0.0f, 0.0f, 0.05f, 0.0f);
    const LfdCam* nb[K] = {&b0, &b1, &b2, &b3};
    LfdPairConst pc[K];
    LfdPoseConst po[K];
    for (int j = 0; j < K; ++j) {
        lfd_make_pair_const(a, *nb[j], j + 1, W_MATCH, H_MATCH, pc[j], nullptr);
        lfd_pose_make_const(a, *nb[j], po[j]);
    }
    expect(po[3].ok == 0.0 && po[3].tn == 0.0 && po[0].ok == 1.0 && po[0].tn > 0.3, "coincident centres are flagged", (long long)po[3].ok, 0);
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
                const float v = (P[4] * X[0] + P[5] * X[1] + P[6] * X[2] + P[7]) / pz + 0.4f * ((float)(cell % 30u) - 15.0f);      // up to 6 px off, either side
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
    const double c2 = (double)inlier_px * (double)inlier_px;
    long long n_conf = 0;
    for (size_t step = 0; step < HW; ++step) {
        const int cell = (int)(backwards ? HW - 1 - step : step);
        const int y = cell / W, x = cell - y * W;
        const bool ok = !masks || mask_a[(size_t)lfd_nearest_src(y, g.mask_sy, H_MATCH) * W_MATCH + lfd_nearest_src(x, g.mask_sx, W_MATCH)] != 0;
        if (!ok) continue;
        float xan, yan;
        if (C == 4) { xan = slot[0].warp[(size_t)cell * 4]; yan = slot[0].warp[(size_t)cell * 4 + 1]; }
        else { xan = lfd_axis_value(axx, x); yan = lfd_axis_value(axy, y); }
        for (int j = 0; j < K; ++j) {
            const float* wv = slot[j].warp + (size_t)cell * C + (C - 2);
            if (!lfd_far_confident(slot[j], g, 0.5f, slot[j].cert[cell], wv[0], wv[1])) continue;
            ++n_conf;
            int32_t q[7];
            const int kind = lfd_pose_sample(po[j], rc.sx, rc.sy, slot[j].sx, slot[j].sy, xan, yan, wv[0], wv[1], wm1, hm1, c2, q);
            expect(kind >= 0 && kind <= 2, "the class", kind, 0);
            int64_t* row = &table[(size_t)j * LFD_POSE_QUANTITIES];
            row[kind] += 1;
            for (int e = 0; e < 7; ++e) {
                const long long bound = e < 6 ? (1LL << 19) : (1LL << 16);
                expect(q[e] >= -bound && q[e] <= bound && (kind == LFD_POSE_INLIER || q[e] == 0), "the quantised values' bounds", q[e], bound);
            }
            if (kind != LFD_POSE_INLIER) continue;
            for (int e = 0; e < LFD_POSE_SUMS; ++e) row[3 + e] += lfd_pose_term(q, e);
        }
    }
    return n_conf;
}

void run(int H, int W, int C, bool masks, float inlier_px) {
    std::vector<int64_t> fwd((size_t)K * LFD_POSE_QUANTITIES, 0), bwd((size_t)K * LFD_POSE_QUANTITIES, 0);
    const long long n_f = accumulate(H, W, C, masks, false, inlier_px, fwd), n_b = accumulate(H, W, C, masks, true, inlier_px, bwd);
    expect(n_f == n_b && n_f > 0 && n_f < (long long)K * H * W, "confident samples", n_f, n_b);
    expect(std::memcmp(fwd.data(), bwd.data(), fwd.size() * 8) == 0, "order-free table", 0, 0);
    long long total = 0, inliers = 0, outliers = 0;
    for (int j = 0; j < K; ++j) {
        const int64_t* row = &fwd[(size_t)j * LFD_POSE_QUANTITIES];
        total += row[0] + row[1] + row[2];
        inliers += row[0]; outliers += row[1];
        expect(row[31] == 0, "column 31 is untouched", row[31], 0);
        expect(row[3] >= 0 && row[10] >= 0 && row[16] >= 0 && row[30] >= 0, "squares are not negative", row[3], row[10]);
        // the 21 products are the upper triangle of a Gram matrix: |H_ab| <= sqrt(H_aa H_bb)
        const int diag[6] = {10, 16, 21, 25, 28, 30};
        int col = 10;
        for (int p = 0; p < 6; ++p)
            for (int q = p; q < 6; ++q, ++col)
                expect((double)row[col] * (double)row[col] <= (double)row[diag[p]] * (double)row[diag[q]] * (1.0 + 1e-12) + 1.0, "Cauchy-Schwarz", col, j);
    }
    expect(total == n_f, "inliers + outliers + degenerate", total, n_f);
    expect(inliers > 0 && outliers > 0, "both classes occur", inliers, outliers);
    const int64_t* last = &fwd[(size_t)(K - 1) * LFD_POSE_QUANTITIES];
    expect(last[0] == 0 && last[1] == 0 && last[2] > 0, "the pair with coincident centres is degenerate", last[0], last[2]);
    for (int e = 3; e < LFD_POSE_QUANTITIES; ++e) expect(last[e] == 0, "... and sums nothing", last[e], e);
    std::printf("H %d W %d C %d masks %d inlier_px %g: %lld confident samples, %lld inliers, %lld outliers\n", H, W, C, (int)masks, (double)inlier_px, n_f,
                inliers, outliers);
}

// the extremes of the arithmetic, on a pair whose arithmetic is exact: K = [[64, 0, 32], [0, 64, 32]], R = I, centres 0 and (1, 0, 0): the line
// of (ua, va) is the row va, r = vb - va
void extremes() {
    LfdCam a, b;
    std::memset(&a, 0, sizeof(a));
    const float Km[9] = {64.0f, 0.0f, 32.0f, 0.0f, 64.0f, 32.0f, 0.0f, 0.0f, 1.0f}, I[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    for (int i = 0; i < 9; ++i) { a.K[i] = Km[i]; a.R[i] = I[i]; }
    a.w = a.h = 65;
    b = a;
    b.t[0] = -1.0f;
    LfdPoseConst pc;
    lfd_pose_make_const(a, b, pc);
    expect(pc.tn == 1.0 && pc.th[0] == -1.0 && pc.ok == 1.0, "the exact pair", (long long)pc.tn, 1);
    int32_t q[7];
    const auto at = [&](float va_px, float vb_px, double c) {
        return lfd_pose_sample(pc, 1.0f, 1.0f, 1.0f, 1.0f, 0.0f, va_px / 32.0f - 1.0f, -0.125f, vb_px / 32.0f - 1.0f, 64.0f, 64.0f, c * c, q);
    };
    expect(at(20.0f, 22.0f, 2.0) == LFD_POSE_OUTLIER && q[6] == 0, "a residual exactly at pose_inlier_px is an outlier", q[6], 0);
    expect(at(20.0f, 18.0f, 2.0) == LFD_POSE_OUTLIER, "... on either side", 0, 0);
    expect(at(20.0f, 21.75f, 2.0) == LFD_POSE_INLIER && q[6] == 1792, "rq = rint(1024 r)", q[6], 1792);
    expect(at(20.0f, 18.25f, 2.0) == LFD_POSE_INLIER && q[6] == -1792, "... signed", q[6], -1792);
    expect(at(0.0f, 64.0f, 64.0) == LFD_POSE_OUTLIER, "64 px at the largest pose_inlier_px", 0, 0);
    expect(at(0.5f, 64.0f, 64.0) == LFD_POSE_INLIER && q[6] == 65024, "the largest rq stays within 2^16", q[6], 65024);
    LfdPoseConst big = pc;
    for (int i = 0; i < 9; ++i) { big.KAi[i] = 3.0e300; big.KBi[i] = 3.0e300; }
    expect(lfd_pose_sample(big, 3.0e38f, 3.0e38f, 3.0e38f, 3.0e38f, 1.0f, 1.0f, 1.0f, 1.0f, 3.0e38f, 3.0e38f, 64.0, q) == LFD_POSE_DEGENERATE,
           "overflow is degenerate", 0, 0);
    LfdPoseConst steep = pc;
    for (int i = 0; i < 9; ++i) steep.KBi[i] = pc.KBi[i] * 1.0e-9;     // |J| far above 2^16: refused before any conversion to an integer
    steep.KBi[8] = 1.0;
    expect(lfd_pose_sample(steep, 1.0f, 1.0f, 1.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 64.0f, 64.0f, 4096.0, q) == LFD_POSE_DEGENERATE && q[0] == 0,
           "a derivative of 2^16 or more is degenerate", q[0], 0);
    b.t[0] = 0.0f;
    lfd_pose_make_const(a, b, pc);
    expect(pc.ok == 0.0 && at(20.0f, 20.0f, 2.0) == LFD_POSE_DEGENERATE, "coincident centres", 0, 0);
    b.t[0] = std::numeric_limits<float>::infinity();
    lfd_pose_make_const(a, b, pc);
    expect(pc.ok == 0.0 && pc.th[0] == 0.0 && at(20.0f, 20.0f, 2.0) == LFD_POSE_DEGENERATE, "a baseline that is not finite", 0, 0);
    // the column order of the sums
    const int32_t v[7] = {2, 3, 5, 7, 11, 13, 17};
    expect(lfd_pose_term(v, 0) == 289 && lfd_pose_term(v, 1) == 34 && lfd_pose_term(v, 6) == 221 && lfd_pose_term(v, 7) == 4 && lfd_pose_term(v, 8) == 6 &&
           lfd_pose_term(v, 12) == 26 && lfd_pose_term(v, 13) == 9 && lfd_pose_term(v, 26) == 143 && lfd_pose_term(v, 27) == 169, "column order", 0, 0);
}

}  // namespace

int main() {
    run(12, 16, 2, false, 5.0f);
    run(12, 16, 4, true, 2.0f);
    run(7, 9, 4, false, 1.0f);
    run(20, 24, 2, true, 4.0f);
    extremes();
    std::printf("ok (%d mismatches)\n", mismatches);
    return mismatches == 0 ? 0 : 1;
}
