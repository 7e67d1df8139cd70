// Stand-alone host program around the per-point routine of the surface normals (csrc/lfd_normals.hpp): lfd_normal_point exactly as the twin
// drives it, over a small two-camera scene whose arrays are heap blocks of exactly the grid's size, for every cell of the grid (windows clipped
// at all four edges and in the corners) and for the degenerate inputs of the contract - a cell of -1 or beyond the grid, a slot the reference
// does not have, a NaN position, a NaN warp inside the window, a single live row, a mask that leaves one row, no live cell at all.  Built with
// -fsanitize=address,undefined by tests/test_normals_sanitized.py and run on its own: a read outside an array, a signed overflow or an
// out-of-range conversion ends it with a report and a non-zero status; every status is compared with the count the contract gives.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "lfd_normals.hpp"

namespace {

constexpr int W_MATCH = 96, H_MATCH = 80, CAM_W = 1297, CAM_H = 840;

LfdCam make_cam(float cx_world, int w_match, int h_match) {
    LfdCam c;
    const float f = 960.0f;
    const float K[9] = {f, 0.0f, CAM_W / 2.0f, 0.0f, f, CAM_H / 2.0f, 0.0f, 0.0f, 1.0f};
    const float R[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    const float t[3] = {-cx_world, 0.0f, 0.0f};
    for (int i = 0; i < 9; ++i) { c.K[i] = K[i]; c.R[i] = R[i]; }
    for (int i = 0; i < 3; ++i) { c.t[i] = t[i]; }
    for (int r = 0; r < 3; ++r)
        for (int col = 0; col < 4; ++col) {
            float v = 0.0f;
            for (int e = 0; e < 3; ++e) v += K[3 * r + e] * (col < 3 ? R[3 * e + col] : t[e]);
            c.P[4 * r + col] = v;
        }
    c.C[0] = cx_world; c.C[1] = 0.0f; c.C[2] = 0.0f;
    c.w = CAM_W; c.h = CAM_H; c.pad[0] = c.pad[1] = 0;
    (void)w_match; (void)h_match;
    return c;
}

struct Scene {
    int H, W, C;
    LfdRefConst rc;
    LfdPairConst pc[2];
    std::vector<float> cert[2], warp[2], ax, ay, xyz;      // xyz: the surface point of every cell (a tilted plane)
    LfdSupportGeom g;
    LfdKernelParams kp;
};

Scene make_scene(int H, int W, int C) {
    Scene s;
    s.H = H; s.W = W; s.C = C;
    const LfdCam a = make_cam(0.0f, W_MATCH, H_MATCH), b0 = make_cam(0.6f, W_MATCH, H_MATCH), b1 = make_cam(-0.5f, W_MATCH, H_MATCH);
    lfd_make_ref_const(a, W_MATCH, H_MATCH, s.rc);
    lfd_make_pair_const(a, b0, 1, W_MATCH, H_MATCH, s.pc[0], nullptr);
    lfd_make_pair_const(a, b1, 2, W_MATCH, H_MATCH, s.pc[1], nullptr);
    const LfdAxis axx = lfd_make_axis(W), axy = lfd_make_axis(H);
    s.ax.resize((size_t)W); s.ay.resize((size_t)H);
    for (int x = 0; x < W; ++x) s.ax[(size_t)x] = lfd_axis_value(axx, x);
    for (int y = 0; y < H; ++y) s.ay[(size_t)y] = lfd_axis_value(axy, y);
    s.xyz.resize((size_t)H * W * 3);
    const LfdCam* nb[2] = {&b0, &b1};
    for (int j = 0; j < 2; ++j) { s.cert[j].assign((size_t)H * W, 0.6f); s.warp[j].resize((size_t)H * W * C); }
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const double ua = ((double)s.ax[(size_t)x] + 1.0) * 0.5 * (W_MATCH - 1) * ((double)CAM_W / W_MATCH);
            const double va = ((double)s.ay[(size_t)y] + 1.0) * 0.5 * (H_MATCH - 1) * ((double)CAM_H / H_MATCH);
            const double dx = (ua - a.K[2]) / a.K[0], dy = (va - a.K[5]) / a.K[4];
            const double z = 4.0 / (1.0 - 0.5 * dy);                  // a plane tilted about the image's x axis
            const double X[3] = {dx * z, dy * z, z};
            const size_t q = (size_t)y * W + x;
            for (int e = 0; e < 3; ++e) s.xyz[3 * q + e] = (float)X[e];
            for (int j = 0; j < 2; ++j) {
                const double xc = X[0] - nb[j]->C[0];
                const double ub = nb[j]->K[0] * xc / z + nb[j]->K[2], vb = nb[j]->K[4] * X[1] / z + nb[j]->K[5];
                float* w = &s.warp[j][q * C];
                if (C == 4) { w[0] = s.ax[(size_t)x]; w[1] = s.ay[(size_t)y]; }
                w[C - 2] = (float)(2.0 * (ub / ((double)CAM_W / W_MATCH)) / (W_MATCH - 1) - 1.0);
                w[C - 1] = (float)(2.0 * (vb / ((double)CAM_H / H_MATCH)) / (H_MATCH - 1) - 1.0);
            }
        }
    s.g.H = H; s.g.W = W; s.g.C = C; s.g.w_match = W_MATCH; s.g.h_match = H_MATCH;
    s.g.wm1 = (float)(W_MATCH - 1); s.g.hm1 = (float)(H_MATCH - 1);
    s.g.mask_sx = (float)W_MATCH / (float)W; s.g.mask_sy = (float)H_MATCH / (float)H;
    s.g.tau = 0.0f; s.g.reproj_thresh = 0.8f;
    s.kp = lfd_normal_params(s.g);
    return s;
}

int window(int H, int W, int R, int cell, int row_only = -1, int skip = -1) {
    const int y = cell / W, x = cell % W;
    int n = 0;
    for (int dy = -R; dy <= R; ++dy)
        for (int dx = -R; dx <= R; ++dx) {
            const int qy = y + dy, qx = x + dx;
            if (qy < 0 || qy >= H || qx < 0 || qx >= W) continue;
            if (row_only >= 0 && qy != row_only) continue;
            if (qy * W + qx == skip) continue;
            ++n;
        }
    return n;
}

int mismatches = 0;

void expect(bool ok, const char* what, int a, int b) {
    if (!ok) { ++mismatches; std::printf("MISMATCH %s: %d / %d\n", what, a, b); }
}

unsigned point(const Scene& s, const uint8_t* mask_a, const uint8_t* const* mask_b, int ns, int R, int cell, int slot, const float* X, float* nrm) {
    LfdNormalSlot sl[2];
    for (int j = 0; j < 2; ++j) sl[j] = {s.cert[j].data(), s.warp[j].data(), mask_b ? mask_b[j] : nullptr};
    return lfd_normal_point(s.rc, s.pc, sl, ns, mask_a, s.ax.data(), s.ay.data(), s.g, s.kp, R, 0.5f, cell, slot, X[0], X[1], X[2], nrm);
}

void run_grid(int H, int W, int C) {
    Scene s = make_scene(H, W, C);
    const int HW = H * W;
    float nrm[3];
    std::vector<uint8_t> ones((size_t)W_MATCH * H_MATCH, 1);
    const uint8_t* mb[2] = {ones.data(), ones.data()};
    for (int R = 1; R <= 4; ++R)
        for (int cell = 0; cell < HW; ++cell) {
            const float* X = &s.xyz[3 * (size_t)cell];
            const int slot = cell & 1;
            const unsigned st = point(s, nullptr, nullptr, 2, R, cell, slot, X, nrm);
            const int want = window(H, W, R, cell);
            expect((int)(st & 0x7f) == want && ((st & 0x80) != 0) == (H > 1 && W > 1), "plain", (int)st, want);
            const double len = std::sqrt((double)nrm[0] * nrm[0] + (double)nrm[1] * nrm[1] + (double)nrm[2] * nrm[2]);
            expect(std::fabs(len - 1.0) < 1e-6 && nrm[2] < 0.0f, "unit, towards the camera", (int)(len * 1e6), cell);
            // masks of ones: only a cell whose warp leaves the neighbour's image drops out
            const unsigned sm = point(s, ones.data(), mb, 2, R, cell, slot, X, nrm);
            expect((sm & 0x7f) <= (st & 0x7f), "masks of ones", (int)sm, (int)st);
        }
    const int R = 4, mid = (H / 2) * W + W / 2;
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const float* Xm = &s.xyz[3 * (size_t)mid];
    // the guard: nothing is read through the cell or the slot
    for (int cell : {-1, HW, HW + 7, std::numeric_limits<int>::max(), std::numeric_limits<int>::min()})
        expect(point(s, nullptr, nullptr, 2, R, cell, 0, Xm, nrm) == 0u && std::fabs(nrm[2] + 1.0f) < 0.2f, "cell outside the grid", cell, 0);
    for (int slot : {2, 3, 255}) expect(point(s, nullptr, nullptr, 2, R, mid, slot, Xm, nrm) == 0u, "slot the reference does not have", slot, 0);
    expect(point(s, nullptr, nullptr, 1, R, mid, 1, Xm, nrm) == 0u, "slot beyond n_slots", 1, 0);
    const float bad[4][3] = {{nan, Xm[1], Xm[2]}, {Xm[0], inf, Xm[2]}, {Xm[0], Xm[1], -Xm[2]}, {0.0f, 0.0f, 0.0f}};
    for (int b = 0; b < 4; ++b) {
        const unsigned st = point(s, nullptr, nullptr, 2, R, mid, 0, bad[b], nrm);
        expect(st == 0u, "position the guard stops", b, (int)st);
        if (b != 2) expect(nrm[0] == 0.0f && nrm[1] == 0.0f && nrm[2] == 0.0f, "no view vector", b, 0);
    }
    // a NaN warp in one window cell: that cell is skipped, the rest fit
    const int hole = mid + 1;
    const float kept = s.warp[0][(size_t)hole * C + C - 1];
    s.warp[0][(size_t)hole * C + C - 1] = nan;
    unsigned st = point(s, nullptr, nullptr, 2, R, mid, 0, Xm, nrm);
    expect((int)(st & 0x7f) == window(H, W, R, mid, -1, hole) && (st & 0x80) != 0, "NaN warp", (int)st, window(H, W, R, mid, -1, hole));
    s.warp[0][(size_t)hole * C + C - 1] = kept;
    // a single live row, left by zero certainties and by mask_a: counted, collinear, the view vector
    const int y0 = H / 2;
    std::vector<float> full = s.cert[0];
    for (int q = 0; q < HW; ++q) if (q / W != y0) s.cert[0][(size_t)q] = (q & 1) ? 0.0f : nan;
    st = point(s, nullptr, nullptr, 2, R, mid, 0, Xm, nrm);
    expect((int)st == window(H, W, R, mid, y0), "one live row (certainty)", (int)st, window(H, W, R, mid, y0));
    s.cert[0] = full;
    std::vector<uint8_t> row((size_t)W_MATCH * H_MATCH, 0);
    for (int my = 0; my < H_MATCH; ++my)
        for (int gy = 0; gy < H; ++gy)
            if (gy == y0 && lfd_nearest_src(gy, s.g.mask_sy, H_MATCH) == my)
                for (int mx = 0; mx < W_MATCH; ++mx) row[(size_t)my * W_MATCH + mx] = 1;
    st = point(s, row.data(), nullptr, 2, R, mid, 0, Xm, nrm);
    expect((int)st == window(H, W, R, mid, y0), "one live row (mask_a)", (int)st, window(H, W, R, mid, y0));
    // nothing live at all: mask_b of zeros, warps that leave the image
    std::vector<uint8_t> zeros((size_t)W_MATCH * H_MATCH, 0);
    const uint8_t* mz[2] = {zeros.data(), zeros.data()};
    expect(point(s, nullptr, mz, 2, R, mid, 0, Xm, nrm) == 0u, "mask_b of zeros", 0, 0);
    std::vector<float> wkeep = s.warp[1];
    for (int q = 0; q < HW; ++q) { s.warp[1][(size_t)q * C + C - 2] = (q % 3 == 0) ? 1e30f : ((q % 3 == 1) ? -inf : 5.0f); }
    expect(point(s, nullptr, mb, 2, R, mid, 1, Xm, nrm) == 0u, "warps outside the mask", 0, 0);
    st = point(s, nullptr, nullptr, 2, R, mid, 1, Xm, nrm);
    expect((st & 0x80) == 0u, "warps outside the image", (int)st, 0);
    s.warp[1] = wkeep;
}

}  // namespace

int main() {
    run_grid(20, 24, 2);
    run_grid(20, 24, 4);
    run_grid(6, 8, 2);
    run_grid(6, 8, 4);
    run_grid(3, 2, 2);
    std::printf("ok (%d mismatches)\n", mismatches);
    return mismatches ? 1 : 0;
}
