// Stand-alone host program around the routines of the far-field shell (csrc/lfd_far.hpp): lfd_far_dir_matrix, lfd_far_direction,
// lfd_far_slot, lfd_far_verdict, lfd_far_key, lfd_far_kept and lfd_far_record exactly as the twins drive them, per cell of a small
// three-camera scene whose arrays - certainties, warps, masks, the image, the table, the emitted records - are heap blocks of exactly the
// documented sizes.  The inputs include what the contract lists: NaN certainties, NaN and infinite observations, observations outside the
// neighbour's grid, NaN A-coordinates (four-channel warps), a zero direction, the smallest and the largest shell, an emit into exactly
// n_out records.  Built with -fsanitize=address,undefined by tests/test_far_sanitized.py and run on its own: a read or write outside an array,
// a signed overflow or an out-of-range float-to-integer conversion ends it with a report and a non-zero status; every table is compared with
// a second accumulation in another order, and every record with the table it came from.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "lfd_far.hpp"

namespace {

constexpr int W_MATCH = 48, H_MATCH = 40, CAM_W = 640, CAM_H = 400, K = 2;

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

// one reference's cells into `table`, visiting them forwards or backwards; returns the far cells
long long accumulate(int H, int W, int C, bool masks, int S, bool backwards, std::vector<uint64_t>& table) {
    const LfdCam a = make_cam(0.0f, 0.0f), b0 = make_cam(0.4f, 0.02f), b1 = make_cam(-0.3f, -0.03f);
    const LfdCam* nb[K] = {&b0, &b1};
    LfdPairConst pc[K];
    lfd_make_pair_const(a, b0, 1, W_MATCH, H_MATCH, pc[0], nullptr);
    lfd_make_pair_const(a, b1, 2, W_MATCH, H_MATCH, pc[1], nullptr);
    LfdRefConst rc;
    lfd_make_ref_const(a, W_MATCH, H_MATCH, rc);
    float M[9];
    lfd_far_dir_matrix(a, M);
    const LfdAxis axx = lfd_make_axis(W), axy = lfd_make_axis(H);
    const size_t HW = (size_t)H * W;
    std::vector<float> cert[K], warp[K];
    std::vector<uint8_t> mask[K], mask_a((size_t)W_MATCH * H_MATCH, 1), image((size_t)W_MATCH * H_MATCH * 3);
    for (size_t i = 0; i < image.size(); ++i) image[i] = (uint8_t)((i * 37u + 11u) & 0xffu);
    for (int x = 0; x < W_MATCH; ++x) mask_a[(size_t)3 * W_MATCH + x] = 0;
    const float wm1 = (float)(W_MATCH - 1), hm1 = (float)(H_MATCH - 1);
    for (int j = 0; j < K; ++j) {
        cert[j].resize(HW); warp[j].resize(HW * C);
        mask[j].assign((size_t)W_MATCH * H_MATCH, 1);
        for (int y = 0; y < H_MATCH; ++y) mask[j][(size_t)y * W_MATCH + 5 + j] = 0;
        float Mb[9];
        lfd_far_dir_matrix(*nb[j], Mb);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const size_t cell = (size_t)y * W + x;
                const float xan = lfd_axis_value(axx, x), yan = lfd_axis_value(axy, y);
                float d[3];
                lfd_far_direction(M, rc.sx, rc.sy, xan, yan, wm1, hm1, d);
                // the rotation-only transfer of the cell (upper half) or a point 2 units along the ray (lower half)
                const float s = y < H / 2 ? 1.0e6f : 2.0f;
                const float X[3] = {a.C[0] + s * d[0], a.C[1] + s * d[1], a.C[2] + s * d[2]};
                const float* P = nb[j]->P;
                const float pz = P[8] * X[0] + P[9] * X[1] + P[10] * X[2] + P[11];
                const float u = (P[0] * X[0] + P[1] * X[1] + P[2] * X[2] + P[3]) / pz, v = (P[4] * X[0] + P[5] * X[1] + P[6] * X[2] + P[7]) / pz;
                float* wv = &warp[j][cell * C];
                if (C == 4) { wv[0] = xan; wv[1] = yan; }
                wv[C - 2] = u / pc[j].sx / (0.5f * wm1) - 1.0f;
                wv[C - 1] = v / pc[j].sy / (0.5f * hm1) - 1.0f;
                cert[j][cell] = 0.55f + 0.4f * (float)((cell * 7u + (unsigned)j) % 10u) / 10.0f;
            }
        const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
        cert[j][1] = nan; cert[j][2] = 0.0f; cert[j][3] = -inf;
        warp[j][(size_t)4 * C + C - 2] = nan; warp[j][(size_t)5 * C + C - 1] = inf; warp[j][(size_t)6 * C + C - 2] = -3.0f;
        warp[j][(size_t)7 * C + C - 1] = 1.0e30f;
        if (C == 4 && j == 0) { warp[j][(size_t)8 * C] = nan; warp[j][(size_t)9 * C + 1] = inf; warp[j][(size_t)10 * C] = 1.0e38f; }
    }
    LfdSlot slot[K];
    for (int j = 0; j < K; ++j) lfd_slot_fill(slot[j], cert[j].data(), warp[j].data(), masks ? mask[j].data() : nullptr, pc[j]);
    LfdSupportGeom g;
    g.H = H; g.W = W; g.C = C; g.w_match = W_MATCH; g.h_match = H_MATCH; g.wm1 = wm1; g.hm1 = hm1;
    g.mask_sx = (float)W_MATCH / (float)W; g.mask_sy = (float)H_MATCH / (float)H; g.tau = 0.8f; g.reproj_thresh = 0.0f;
    long long n_far = 0;
    for (size_t step = 0; step < HW; ++step) {
        const int cell = (int)(backwards ? HW - 1 - step : step);
        const int y = cell / W, x = cell - y * W;
        if (masks && mask_a[(size_t)lfd_nearest_src(y, g.mask_sy, H_MATCH) * W_MATCH + lfd_nearest_src(x, g.mask_sx, W_MATCH)] == 0) continue;
        float xan, yan, d[3];
        if (C == 4) { xan = slot[0].warp[(size_t)cell * 4]; yan = slot[0].warp[(size_t)cell * 4 + 1]; }
        else { xan = lfd_axis_value(axx, x); yan = lfd_axis_value(axy, y); }
        lfd_far_direction(M, rc.sx, rc.sy, xan, yan, wm1, hm1, d);
        int n_conf = 0, n_agree = 0;
        for (int j = 0; j < K; ++j) {
            const float* wv = slot[j].warp + (size_t)cell * C + (C - 2);
            const int v = lfd_far_slot(slot[j], g, 0.5f, slot[j].cert[cell], wv[0], wv[1], d[0], d[1], d[2]);
            n_conf += v & 1; n_agree += v >> 1;
        }
        if (!lfd_far_verdict(n_conf, n_agree, 2, K)) continue;
        long long key, q[3];
        if (!lfd_far_key(d[0], d[1], d[2], S, &key, q)) continue;
        expect(key >= 0 && key < 6LL * S * S, "key in range", key, 6LL * S * S);
        float rgb[3];
        lfd_bilinear_rgb_f32(image.data(), W_MATCH, H_MATCH, lfd_match_px(xan, wm1), lfd_match_px(yan, hm1), rgb);
        uint64_t* row = &table[(size_t)key * LFD_FAR_QUANTITIES];
        for (int e = 0; e < 3; ++e) { row[e] += (uint64_t)q[e]; row[3 + e] += (uint64_t)lfd_quantise_u8(rgb[e]); }
        row[6] += 1;
        ++n_far;
    }
    return n_far;
}

void run(int H, int W, int C, bool masks, int S) {
    const size_t rows = (size_t)6 * S * S;
    std::vector<uint64_t> fwd(rows * LFD_FAR_QUANTITIES, 0), bwd(rows * LFD_FAR_QUANTITIES, 0);
    const long long n_f = accumulate(H, W, C, masks, S, false, fwd), n_b = accumulate(H, W, C, masks, S, true, bwd);
    expect(n_f == n_b && n_f > 0 && n_f < (long long)H * W, "far cells", n_f, n_b);
    expect(std::memcmp(fwd.data(), bwd.data(), fwd.size() * 8) == 0, "order-free table", 0, 0);
    long long total = 0, kept = 0;
    for (size_t i = 0; i < rows; ++i) { total += (long long)fwd[i * 7 + 6]; kept += lfd_far_kept(&fwd[i * 7], 1) ? 1 : 0; }
    expect(total == n_f, "sum of the counts", total, n_f);
    // emit into exactly `kept` records
    std::vector<float> xyz((size_t)kept * 3), rgb((size_t)kept * 3), nrm((size_t)kept * 3);
    std::vector<int32_t> smp((size_t)kept);
    const double centre[3] = {0.5, -0.25, 2.0}, radius = 40.0;
    long long o = 0;
    for (size_t i = 0; i < rows; ++i) {
        if (!lfd_far_kept(&fwd[i * 7], 1)) continue;
        lfd_far_record(&fwd[i * 7], centre, radius, &xyz[3 * o], &rgb[3 * o], &nrm[3 * o], &smp[o]);
        double r2 = 0.0, n2 = 0.0;
        for (int e = 0; e < 3; ++e) { const double dx = (double)xyz[3 * o + e] - centre[e]; r2 += dx * dx; n2 += (double)nrm[3 * o + e] * nrm[3 * o + e]; }
        expect(std::fabs(std::sqrt(r2) - radius) < 1e-4 && std::fabs(n2 - 1.0) < 1e-5, "record on the sphere", (long long)i, o);
        expect(smp[o] == (int32_t)fwd[i * 7 + 6] && rgb[3 * o] >= 0.0f && rgb[3 * o] <= 1.0f, "samples / colour", smp[o], (long long)fwd[i * 7 + 6]);
        ++o;
    }
    expect(o == kept, "records", o, kept);
    // a saturated count and a row whose direction sums cancel
    uint64_t big[7] = {1, 0, 0, 255, 0, 0, 0x100000000ull}, zero[7] = {0, 0, 0, 9, 9, 9, 5};
    float a3[3], b3[3];
    int32_t s1 = 0;
    lfd_far_record(big, centre, radius, a3, b3, nullptr, &s1);
    expect(s1 == 0x7fffffff && lfd_far_kept(big, 1) && !lfd_far_kept(zero, 1), "saturation / empty direction", s1, 0);
    // directions that have no cell
    long long key = 0, q[3];
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    expect(!lfd_far_key(0.0f, -0.0f, 0.0f, S, &key, q) && !lfd_far_key(nan, 1.0f, 0.0f, S, &key, q) && !lfd_far_key(1.0f, inf, 0.0f, S, &key, q),
           "zero / non-finite direction", 0, 0);
    expect(lfd_far_key(3.0e38f, -3.0e38f, 3.0e38f, S, &key, q) && lfd_far_key(1.0e-45f, 0.0f, 0.0f, S, &key, q), "extreme directions", 0, 0);
    std::printf("H %d W %d C %d masks %d S %d: %lld far cells, %lld direction cells\n", H, W, C, (int)masks, S, n_f, kept);
}

}  // namespace

int main() {
    run(12, 16, 2, false, 8);
    run(12, 16, 4, true, 8);
    run(7, 9, 4, false, 512);
    run(20, 24, 2, true, 32);
    std::printf("ok (%d mismatches)\n", mismatches);
    return mismatches == 0 ? 0 : 1;
}
