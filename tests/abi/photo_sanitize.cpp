// Stand-alone host program around the twin of the photo-consistency gate (csrc/lfd_photo.hpp): lfd_photo_check, lfd_photo_thresholds and
// lfd_photo_point - the very routine lfd_photo_gate_host runs per point behind its context checks - driven over heap arrays of exactly the
// documented sizes (certainty [H * W], warp [H * W * C], images [h_match * w_match * 3], masks [h_match * w_match], axes [W] and [H]) on the
// edge cases of the rule: a 6 x 8 grid whose R = 3 window crosses every border at once, 2- and 4-channel warps, masks, observations that are
// NaN, infinite, exactly on and just beyond the border, certainties of exactly 0 and NaN, reference positions of a 4-channel warp that are NaN
// or far outside the image, cells outside the grid, slots the reference does not have, constant images, a texture floor of 0 and one beyond
// every variance.  Every status and ncc is compared with a plain loop written from the rule.  Built with -fsanitize=address,undefined by
// tests/test_photo_sanitized.py and run on its own: a read outside an array, an overflow of the integer sums or an out-of-range conversion ends it
// with a report and a non-zero status.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "lfd_photo.hpp"

struct Case {
    int H, W, C, wm, hm, ns;
    std::vector<float*> cert, warp;
    std::vector<uint8_t*> mask_b, img;
    uint8_t* img_a;
    uint8_t* mask_a;
    float *ax, *ay;
};

// the four-tap blend as the rule words it, on its own: taps floor / floor + 1 clamped, a clamped column folds its weights, fused chain, / 255
static void tap_blend(const uint8_t* img, int w, int h, float x, float y, float* rgb) {
    float fx0 = std::floor(x), fy0 = std::floor(y);
    if (!(fx0 > 0.0f)) fx0 = 0.0f;
    if (fx0 > (float)(w - 1)) fx0 = (float)(w - 1);
    if (!(fy0 > 0.0f)) fy0 = 0.0f;
    if (fy0 > (float)(h - 1)) fy0 = (float)(h - 1);
    const float fx1 = fx0 + 1.0f > (float)(w - 1) ? (float)(w - 1) : fx0 + 1.0f, fy1 = fy0 + 1.0f > (float)(h - 1) ? (float)(h - 1) : fy0 + 1.0f;
    const int x0 = (int)fx0, y0 = (int)fy0, x1 = (int)fx1, y1 = (int)fy1;
    const float ax = fx1 - x, bx = x - fx0, ay = fy1 - y, by = y - fy0;
    float wa = ax * ay, wb = bx * ay, wc = ax * by, wd = bx * by;
    if (fx1 == fx0) { wa = wa + wb; wb = 0.0f; wc = wc + wd; wd = 0.0f; }
    for (int ch = 0; ch < 3; ++ch) {
        const float a = (float)img[((size_t)y0 * w + x0) * 3 + ch], b = (float)img[((size_t)y0 * w + x1) * 3 + ch];
        const float c = (float)img[((size_t)y1 * w + x0) * 3 + ch], d = (float)img[((size_t)y1 * w + x1) * 3 + ch];
        rgb[ch] = std::fmaf(d, wd, std::fmaf(c, wc, std::fmaf(b, wb, a * wa))) * 0.00392156862745098f;
    }
}

static long long grey_of(const float* rgb) {
    long long s = 0;
    for (int ch = 0; ch < 3; ++ch) {
        float c = rgb[ch];
        if (!(c >= 0.0f)) c = 0.0f;
        if (c > 1.0f) c = 1.0f;
        s += (long long)std::floor(c * 4096.0f);
    }
    return s;
}

static int nearest(int dst, float scale, int size) {
    const int s = (int)std::floor((float)dst * scale);
    return s < size - 1 ? s : size - 1;
}

static unsigned brute(const Case& c, int R, float min_ncc, float min_texture, int cell, int s, float* ncc) {
    *ncc = std::numeric_limits<float>::quiet_NaN();
    if (cell < 0 || cell >= c.H * c.W || s >= c.ns) return 0u;
    const float msx = (float)c.wm / (float)c.W, msy = (float)c.hm / (float)c.H;
    const int y = cell / c.W, x = cell % c.W;
    long long n = 0, Sa = 0, Sb = 0, Saa = 0, Sbb = 0, Sab = 0;
    for (int qy = y - R; qy <= y + R; ++qy)
        for (int qx = x - R; qx <= x + R; ++qx) {
            if (qy < 0 || qy >= c.H || qx < 0 || qx >= c.W) continue;
            const size_t q = (size_t)qy * c.W + qx;
            const float* wp = c.warp[s] + q * c.C;
            const float xb = wp[c.C - 2], yb = wp[c.C - 1];
            if (!(c.cert[s][q] > 0.0f) || !(xb >= -1.0f && xb <= 1.0f && yb >= -1.0f && yb <= 1.0f)) continue;
            if (c.mask_b[s]) {
                const float gx = std::nearbyint(((xb + 1.0f) * (float)c.W - 1.0f) / 2.0f), gy = std::nearbyint(((yb + 1.0f) * (float)c.H - 1.0f) / 2.0f);
                if (!(gx >= 0.0f && gx <= (float)(c.W - 1) && gy >= 0.0f && gy <= (float)(c.H - 1))) continue;
                if (!c.mask_b[s][(size_t)nearest((int)gy, msy, c.hm) * c.wm + nearest((int)gx, msx, c.wm)]) continue;
            }
            if (c.mask_a && !c.mask_a[(size_t)nearest(qy, msy, c.hm) * c.wm + nearest(qx, msx, c.wm)]) continue;
            const float xa = c.C == 4 ? wp[0] : c.ax[qx], ya = c.C == 4 ? wp[1] : c.ay[qy];
            float va[3], vb[3];
            tap_blend(c.img_a, c.wm, c.hm, ((xa + 1.0f) * 0.5f) * (float)(c.wm - 1), ((ya + 1.0f) * 0.5f) * (float)(c.hm - 1), va);
            tap_blend(c.img[s], c.wm, c.hm, ((xb + 1.0f) * 0.5f) * (float)(c.wm - 1), ((yb + 1.0f) * 0.5f) * (float)(c.hm - 1), vb);
            const long long a = grey_of(va), b = grey_of(vb);
            n += 1; Sa += a; Sb += b; Saa += a * a; Sbb += b * b; Sab += a * b;
        }
    const long long side = 2 * R + 1;
    if (2 * n < side * side + 1) return 1u;
    const long long va = n * Saa - Sa * Sa, vb = n * Sbb - Sb * Sb, cov = n * Sab - Sa * Sb;
    const double sd = (double)min_texture * 12288.0 / 255.0;
    const double T = std::ceil(sd * sd);
    if ((double)va < (double)(n * n) * T || (double)vb < (double)(n * n) * T) return 2u;      // (va, n n and T's products: exact in f64 below 2^53, or huge)
    const double fc = (double)cov, fv = (double)va * (double)vb, t2 = (double)min_ncc * (double)min_ncc;
    if (fv > 0.0) *ncc = (float)(fc / std::sqrt(fv));
    return (cov > 0 && fc * fc >= t2 * fv) ? 3u : 4u;
}

static long long run(const char* name, const Case& c, int R, float min_ncc, float min_texture, const std::vector<int>& cells, const std::vector<int>& slots) {
    std::vector<LfdPhotoSlot> sl((size_t)c.ns);
    for (int j = 0; j < c.ns; ++j) sl[(size_t)j] = {c.cert[(size_t)j], c.warp[(size_t)j], c.mask_b[(size_t)j], c.img[(size_t)j]};
    LfdSupportGeom g;
    g.H = c.H; g.W = c.W; g.C = c.C; g.w_match = c.wm; g.h_match = c.hm;
    g.wm1 = (float)(c.wm - 1); g.hm1 = (float)(c.hm - 1); g.mask_sx = (float)c.wm / (float)c.W; g.mask_sy = (float)c.hm / (float)c.H;
    g.tau = 0.0f; g.reproj_thresh = 0.0f;
    const LfdPhotoThresh th = lfd_photo_thresholds(min_ncc, min_texture);
    long long bad = 0, count[LFD_PHOTO_STATUSES] = {0, 0, 0, 0, 0};
    const size_t n = cells.size();
    uint8_t* status = new uint8_t[n];                                         // exactly one entry per input point, on the heap
    float* ncc = new float[n];
    for (size_t i = 0; i < n; ++i) {
        status[i] = (uint8_t)lfd_photo_point(sl.data(), c.ns, c.img_a, c.mask_a, c.ax, c.ay, g, R, th, cells[i], slots[i], &ncc[i]);
        float want_ncc;
        const unsigned want = brute(c, R, min_ncc, min_texture, cells[i], slots[i], &want_ncc);
        bad += status[i] == want ? 0 : 1;
        bad += (std::isnan(ncc[i]) && std::isnan(want_ncc)) || ncc[i] == want_ncc ? 0 : 1;
        ++count[status[i] < LFD_PHOTO_STATUSES ? status[i] : 0];
    }
    std::printf("%-22s %2d x %2d C %d R %d ncc %-4g tex %-8g points %4zu statuses %lld %lld %lld %lld %lld  %s\n", name, c.H, c.W, c.C, R, min_ncc,
                min_texture, n, count[0], count[1], count[2], count[3], count[4], bad ? "MISMATCH" : "ok");
    delete[] status;
    delete[] ncc;
    return bad;
}

int main() {
    std::mt19937 gen(5);
    std::uniform_real_distribution<float> uni(0.0f, 1.0f);
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    long long bad = 0;
    for (int C : {2, 4})
        for (int masks = 0; masks < 2; ++masks) {
            Case c;
            c.H = 6; c.W = 8; c.C = C; c.wm = 40; c.hm = 32; c.ns = 3;
            const size_t HW = (size_t)c.H * c.W, px = (size_t)c.wm * c.hm;
            c.ax = new float[(size_t)c.W]; c.ay = new float[(size_t)c.H];
            for (int x = 0; x < c.W; ++x) c.ax[x] = -1.0f + (2.0f * (float)x + 1.0f) / (float)c.W;
            for (int y = 0; y < c.H; ++y) c.ay[y] = -1.0f + (2.0f * (float)y + 1.0f) / (float)c.H;
            c.img_a = new uint8_t[px * 3];
            for (size_t e = 0; e < px * 3; ++e) c.img_a[e] = (uint8_t)(255.0f * uni(gen));
            c.mask_a = nullptr;
            if (masks) {
                c.mask_a = new uint8_t[px];
                for (size_t e = 0; e < px; ++e) c.mask_a[e] = uni(gen) < 0.85f ? 1 : 0;
            }
            for (int j = 0; j < c.ns; ++j) {
                float* cert = new float[HW];
                float* warp = new float[HW * (size_t)C];
                uint8_t* img = new uint8_t[px * 3];
                // slot 0: the reference's image under a gain and an offset at (nearly) the same place - consistent; slot 1: another image - refuted
                for (size_t e = 0; e < px * 3; ++e) img[e] = j == 0 ? (uint8_t)(0.7f * (float)c.img_a[e] + 20.0f) : (uint8_t)(255.0f * uni(gen));
                for (size_t q = 0; q < HW; ++q) {
                    cert[q] = 0.1f + 0.8f * uni(gen);
                    float* wp = warp + q * (size_t)C;
                    const float xa = c.ax[q % (size_t)c.W], ya = c.ay[q / (size_t)c.W];
                    if (C == 4) { wp[0] = xa; wp[1] = ya; }
                    wp[C - 2] = j == 2 ? 2.4f * uni(gen) - 1.2f : xa;            // slot 2: anywhere, a good part outside [-1, 1]
                    wp[C - 1] = j == 2 ? 2.4f * uni(gen) - 1.2f : ya;
                }
                // the special values, inside windows of the points below
                cert[9] = 0.0f; cert[10] = nan; cert[11] = -0.5f;
                warp[17 * (size_t)C + (size_t)C - 2] = nan; warp[18 * (size_t)C + (size_t)C - 1] = inf; warp[19 * (size_t)C + (size_t)C - 2] = -inf;
                warp[20 * (size_t)C + (size_t)C - 2] = 1.0f; warp[21 * (size_t)C + (size_t)C - 1] = -1.0f;
                warp[22 * (size_t)C + (size_t)C - 2] = std::nextafter(1.0f, 2.0f); warp[23 * (size_t)C + (size_t)C - 1] = std::nextafter(-1.0f, -2.0f);
                if (C == 4) {                                                  // the reference position is the warp's: anything may stand there
                    warp[25 * 4] = nan; warp[26 * 4 + 1] = inf; warp[27 * 4] = 3.0e38f; warp[28 * 4 + 1] = -3.0e38f; warp[29 * 4] = -7.0f; warp[30 * 4] = 1.5f;
                }
                uint8_t* mb = nullptr;
                if (masks) {
                    mb = new uint8_t[px];
                    for (size_t e = 0; e < px; ++e) mb[e] = uni(gen) < 0.85f ? 1 : 0;
                }
                c.cert.push_back(cert); c.warp.push_back(warp); c.img.push_back(img); c.mask_b.push_back(mb);
            }
            std::vector<int> cells, slots;
            for (int s = 0; s < c.ns; ++s)
                for (int q = 0; q < (int)HW; ++q) { cells.push_back(q); slots.push_back(s); }
            for (int q : {-1, (int)HW, std::numeric_limits<int>::max(), std::numeric_limits<int>::min()}) { cells.push_back(q); slots.push_back(0); }
            for (int s : {3, 16, 255}) { cells.push_back(5); slots.push_back(s); }
            for (int R = 1; R <= 3; ++R) {
                bad += run(masks ? "noise, masks" : "noise", c, R, 0.8f, 2.0f, cells, slots);
                bad += run("texture floor 0", c, R, 1.0f, 0.0f, cells, slots);
                bad += run("texture floor huge", c, R, 0.5f, 3.0e38f, cells, slots);
                bad += run("texture floor 48.2", c, R, 1e-30f, 48.2f, cells, slots);
            }
            // constant images: va = vb = cov = 0
            std::memset(c.img_a, 131, px * 3);
            for (int j = 0; j < c.ns; ++j) std::memset(c.img[(size_t)j], 90 + 40 * j, px * 3);
            bad += run("constant", c, 2, 0.8f, 2.0f, cells, slots);
            bad += run("constant, floor 0", c, 2, 0.8f, 0.0f, cells, slots);
            // white and black: the largest sums the rule allows (a, b = 12 288 over 49 cells)
            for (size_t e = 0; e < px * 3; ++e) { c.img_a[e] = (e / 3) % 2 ? 255 : 0; c.img[0][e] = (e / 3) % 2 ? 255 : 0; }
            bad += run("black and white", c, 3, 0.8f, 2.0f, cells, slots);
            for (int j = 0; j < c.ns; ++j) { delete[] c.cert[(size_t)j]; delete[] c.warp[(size_t)j]; delete[] c.img[(size_t)j]; delete[] c.mask_b[(size_t)j]; }
            delete[] c.img_a; delete[] c.mask_a; delete[] c.ax; delete[] c.ay;
        }

    // the argument check: what it refuses and what it lets through, over arrays of the documented sizes
    {
        const long long cap = 5;
        float* f = new float[7 * cap * 2];
        int32_t* cell = new int32_t[cap * 2];
        uint8_t* slot = new uint8_t[cap * 2];
        uint8_t* status = new uint8_t[cap];
        float* ncc = new float[cap];
        int64_t* counters = new int64_t[LFD_PHOTO_STATUSES];
        int64_t offs[2] = {0, 5}, offs_out[2];
        const uint8_t* images[1] = {status};
        lfd_points in = {f, f + 3 * cap, f + 6 * cap, cell, slot, cap}, out = {f + 7 * cap, f + 10 * cap, f + 13 * cap, cell + cap, slot + cap, cap};
        int code = 0;
        auto chk = [&](int R, float ncc_min, float tex, const lfd_points* o, uint8_t* st, float* nc, int64_t* cnt) {
            return lfd_photo_check(&in, offs, images, R, ncc_min, tex, o, offs_out, st, nc, cnt, &code);
        };
        bad += chk(2, 0.8f, 2.0f, &out, status, ncc, counters) == nullptr ? 0 : 1;
        bad += chk(2, 1.0f, 0.0f, &out, nullptr, nullptr, nullptr) == nullptr ? 0 : 1;
        for (int R : {0, 4, -1}) bad += (chk(R, 0.8f, 2.0f, &out, status, ncc, counters) && code == LFD_ERR_INVALID) ? 0 : 1;
        for (float v : {0.0f, -0.5f, 1.0001f, nan, inf}) bad += (chk(2, v, 2.0f, &out, status, ncc, counters) && code == LFD_ERR_INVALID) ? 0 : 1;
        for (float v : {-1.0f, nan, inf}) bad += (chk(2, 0.8f, v, &out, status, ncc, counters) && code == LFD_ERR_INVALID) ? 0 : 1;
        bad += (chk(2, 0.8f, 2.0f, &out, slot, ncc, counters) && code == LFD_ERR_INVALID) ? 0 : 1;
        bad += (chk(2, 0.8f, 2.0f, &out, status, f + 8 * cap, counters) && code == LFD_ERR_INVALID) ? 0 : 1;
        bad += (chk(2, 0.8f, 2.0f, &out, status, reinterpret_cast<float*>(counters), counters) && code == LFD_ERR_INVALID) ? 0 : 1;
        lfd_points small = out;
        small.capacity = cap - 1;
        bad += (chk(2, 0.8f, 2.0f, &small, status, ncc, counters) && code == LFD_ERR_CAPACITY) ? 0 : 1;
        std::printf("%-22s %s\n", "argument check", bad ? "MISMATCH" : "ok");
        delete[] f; delete[] cell; delete[] slot; delete[] status; delete[] ncc; delete[] counters;
    }
    std::printf("%s (%lld mismatches)\n", bad ? "FAILED" : "ok", bad);
    return bad ? 1 : 0;
}
