// Photo-consistency gate on triangulated points (lfd_photo_gate): the per-point routine, compiled for the device (lfd_photo.hip)
// and for the host (lfd_host.hip's twin).  Every other gate is geometric; this one looks at the pixels.  A match that slid along its epipolar
// line has Sampson distance 0, triangulates cleanly and reprojects exactly: only the images can refute it.  The test is the zero-mean
// normalised cross-correlation (ZNCC) of the two patches the MATCH joins - the reference's around the point's cell, the winning neighbour's
// where the dense warp sends every cell of that window.  The warp is the patch-to-patch mapping: no homography, no normal.  xyz is carried
// along and never read, so the gate commutes with the re-triangulation.
//
// The rule, for input point i of reference r, made by winning slot s on cell c = (y, x) of the H x W grid:
//
//   guard     cell outside [0, H * W) or s >= n_slots[r]: kept with status 0, no address is formed from the cell or the slot.
//   window    the cells (y + dy, x + dx), |dy|, |dx| <= R (1 .. 3), inside the grid.  A window cell c' PARTICIPATES iff
//               - lfd_support_live(cert[r, s][c']);
//               - its observation (xb, yb), the last two warp channels of slot s at c', is finite and -1 <= xb, yb <= 1 (f32 compares);
//               - with mask_b[r, s]: the mask pixel the warp points at (lfd_support_mask_index) is non-zero;
//               - with mask_a[r]: the cell's own mask pixel (the certainty prologue's lookup) is non-zero.
//   samples   reference: lfd_bilinear_rgb_f32 of image[r] at the match pixel (lfd_match_px) of the cell's reference position - warp channels
//             0 and 1 of a 4-channel warp, else axis_x / axis_y; neighbour: lfd_colour_sample of nbr_image[r * k + s] at (xb, yb).  Each
//             channel c is quantised as (uint32_t)(c * 4096.0f) - a power of two and a truncation - after a clamp to [0, 1] that changes
//             nothing for a position inside the image and makes the conversion defined for a 4-channel warp whose reference position is
//             far outside or NaN (NaN -> 0).  a, b: the sums of the three quantised channels, at most 12 288.
//   sums      exact integers: n, Sa, Sb, Saa, Sbb, Sab over the participating cells; va = n Saa - Sa Sa, vb = n Sbb - Sb Sb, cov = n Sab - Sa Sb
//             (every term below 3.7e11).  Nothing depends on summation order, launch geometry or thread count.
//   verdict   in this order -
//               1  2 n < (2R + 1)^2 + 1 (under half the window participates)                           status 1, kept
//               2  va < n n T or vb < n n T (untextured: no evidence)                                  status 2, kept
//               3  cov > 0 and (double)cov * (double)cov >= t2 * ((double)va * (double)vb)             status 3, kept
//               4  otherwise                                                                            status 4, DROPPED
//             T = ceil((min_texture * 12288 / 255)^2), an integer computed once in f64 by lfd_photo_texture_floor (min_texture: a standard
//             deviation in 8-bit grey levels); t2 = (double)min_ncc * (double)min_ncc.  Each f64 product is rounded once (the build uses
//             -ffp-contract=off); no division and no root takes part in the decision.
//   ncc       optional, per INPUT point: (float)(cov / sqrt(va vb)) for status 3 or 4, NaN otherwise.  IEEE divide and root on the host,
//             lfd_sqrt_rare / lfd_recip_refined on the device: within one f32 ulp (the precedent of sigma_rel).  The decision never reads it.
//
// The gate drops only on evidence against a match.  ZNCC is invariant to gain and offset: differently exposed views need no gain_compensation.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/lfd_densify.h"
#include "lfd_colour.hpp"
#include "lfd_geometry.hpp"
#include "lfd_support.hpp"

#define LFD_PHOTO_MAX_RADIUS 3
#define LFD_PHOTO_GUARDED 0
#define LFD_PHOTO_SPARSE 1
#define LFD_PHOTO_UNTEXTURED 2
#define LFD_PHOTO_CONSISTENT 3
#define LFD_PHOTO_REFUTED 4
#define LFD_PHOTO_STATUSES 5

struct LfdPhotoSlot {            // one neighbour of the reference at work (LDS on the device, a table on the host)
    const float* cert;
    const float* warp;
    const uint8_t* mask_b;
    const uint8_t* img;          // its match-size image
};

struct LfdPhotoAcc {             // what lives across the window loop: six exact integers
    uint32_t n, Sa, Sb;
    uint64_t Saa, Sbb, Sab;
};

struct LfdPhotoThresh {          // the thresholds of a call, made once by lfd_photo_thresholds on the host for both entry points
    long long T;                 // the texture floor (a variance of the quantised sums, per n^2)
    double t2;                   // min_ncc^2
};

// T = ceil((min_texture * 12288 / 255)^2) in f64.  va <= n n 12288^2 < n n 2^40, so a floor at or above 2^40 keeps every point as untextured:
// the cap changes no verdict and keeps n n T inside i64.
inline long long lfd_photo_texture_floor(float min_texture) {
    const double s = (double)min_texture * 12288.0 / 255.0;
    const double t = ceil(s * s);
    return t >= 1099511627776.0 ? 1099511627776LL : (long long)t;
}

inline LfdPhotoThresh lfd_photo_thresholds(float min_ncc, float min_texture) {
    LfdPhotoThresh t;
    t.T = lfd_photo_texture_floor(min_texture);
    t.t2 = (double)min_ncc * (double)min_ncc;
    return t;
}

LFD_HD bool lfd_photo_guarded(int cell, long long HW, int s, int ns) { return cell < 0 || (long long)cell >= HW || s >= ns; }

// one channel, quantised (see `samples` above)
LFD_HD uint32_t lfd_photo_quantise(float c) { return (uint32_t)(fminf(fmaxf(c, 0.0f), 1.0f) * 4096.0f); }

LFD_HD uint32_t lfd_photo_grey(const float* rgb) { return lfd_photo_quantise(rgb[0]) + lfd_photo_quantise(rgb[1]) + lfd_photo_quantise(rgb[2]); }

LFD_HD void lfd_photo_clear(LfdPhotoAcc& a) { a.n = 0u; a.Sa = 0u; a.Sb = 0u; a.Saa = 0ull; a.Sbb = 0ull; a.Sab = 0ull; }

// Does window cell q = (qx, qy), inside the grid, participate?  cert, (xbn, ybn): the winning slot's raw certainty and observation at q.
LFD_HD bool lfd_photo_participates(const uint8_t* mask_a, const uint8_t* mask_b, const LfdSupportGeom& g, int qx, int qy, float cert, float xbn,
                                   float ybn) {
    bool part = lfd_support_live(cert) && xbn >= -1.0f && xbn <= 1.0f && ybn >= -1.0f && ybn <= 1.0f;       // (a NaN or an inf fails a compare)
    if (part && mask_b) {
        const long long m = lfd_support_mask_index(xbn, ybn, g.W, g.H, g.mask_sx, g.mask_sy, g.w_match, g.h_match);
        part = m >= 0 && mask_b[m] != 0;
    }
    if (part && mask_a)
        part = mask_a[(size_t)lfd_nearest_src(qy, g.mask_sy, g.h_match) * g.w_match + lfd_nearest_src(qx, g.mask_sx, g.w_match)] != 0;
    return part;
}

// One participating window cell.  (xan, yan): the cell's reference position, (xbn, ybn): its observation; img_a / img_b: the reference's and the
// winning neighbour's image.
LFD_HD void lfd_photo_sample(LfdPhotoAcc& acc, const uint8_t* img_a, const uint8_t* img_b, const LfdSupportGeom& g, float xan, float yan, float xbn,
                             float ybn) {
    float va[3], vb[3];
#if defined(__HIP_DEVICE_COMPILE__)
    // the dense kernel's form of the same blend (lfd_geometry.hpp): a row's two taps in ONE unaligned 8-byte load, four loads per cell instead
    // of 24 byte loads, all four issued before the first is used; bit-identical to lfd_bilinear_rgb_f32
    const float xa = lfd_match_px(xan, g.wm1), ya = lfd_match_px(yan, g.hm1), xb = lfd_match_px(xbn, g.wm1), yb = lfd_match_px(ybn, g.hm1);
    unsigned sa0, sa1, sb0, sb1;
    const LfdTapRows ta = lfd_bilinear_fetch(img_a, g.w_match, g.h_match, xa, ya, sa0, sa1);
    const LfdTapRows tb = lfd_bilinear_fetch(img_b, g.w_match, g.h_match, xb, yb, sb0, sb1);
    lfd_bilinear_eval_f32(ta, sa0, sa1, g.w_match, g.h_match, xa, ya, va);
    lfd_bilinear_eval_f32(tb, sb0, sb1, g.w_match, g.h_match, xb, yb, vb);
#else
    lfd_bilinear_rgb_f32(img_a, g.w_match, g.h_match, lfd_match_px(xan, g.wm1), lfd_match_px(yan, g.hm1), va);
    lfd_colour_sample(img_b, g, xbn, ybn, vb);
#endif
    const uint32_t a = lfd_photo_grey(va), b = lfd_photo_grey(vb);
    acc.n += 1u; acc.Sa += a; acc.Sb += b;
    acc.Saa += (uint64_t)(a * a); acc.Sbb += (uint64_t)(b * b); acc.Sab += (uint64_t)(a * b);     // (a, b <= 12 288: the products fit 32 bits)
}

// The verdict of a point that passed the guard; *ncc receives the optional value (NaN unless the status is 3 or 4).
LFD_HD unsigned lfd_photo_verdict(const LfdPhotoAcc& acc, int R, const LfdPhotoThresh& th, float* ncc) {
    *ncc = __builtin_nanf("");
    const long long n = (long long)acc.n, Sa = (long long)acc.Sa, Sb = (long long)acc.Sb, side = 2 * R + 1;
    if (2 * n < side * side + 1) return LFD_PHOTO_SPARSE;
    const long long va = n * (long long)acc.Saa - Sa * Sa, vb = n * (long long)acc.Sbb - Sb * Sb, cov = n * (long long)acc.Sab - Sa * Sb;
    const long long floor_ = n * n * th.T;
    if (va < floor_ || vb < floor_) return LFD_PHOTO_UNTEXTURED;
    const double fc = (double)cov, fv = (double)va * (double)vb;
    const double lhs = fc * fc, rhs = th.t2 * fv;
    if (fv > 0.0) {
#if defined(__HIP_DEVICE_COMPILE__)
        *ncc = (float)(fc * lfd_recip_refined(lfd_sqrt_rare(fv)));
#else
        *ncc = (float)(fc / sqrt(fv));
#endif
    }
    return (cov > 0 && lhs >= rhs) ? LFD_PHOTO_CONSISTENT : LFD_PHOTO_REFUTED;
}

// One point over plain pointers, every value read where it is needed: the twin's form of the routine (the kernel issues a window row's certainty and
// observation loads before its arithmetic and calls the same functions).  sl [ns]: the reference's neighbours; img_a / mask_a: the reference's image and mask;
// ax / ay: the A-grid axes (two-channel warps).  Returns the status.
inline unsigned lfd_photo_point(const LfdPhotoSlot* sl, int ns, const uint8_t* img_a, const uint8_t* mask_a, const float* ax, const float* ay,
                                const LfdSupportGeom& g, int R, const LfdPhotoThresh& th, int cell, int s, float* ncc) {
    *ncc = __builtin_nanf("");
    if (lfd_photo_guarded(cell, (long long)g.H * g.W, s, ns)) return LFD_PHOTO_GUARDED;
    const LfdPhotoSlot& w = sl[s];
    const int y = cell / g.W, x = cell - y * g.W;
    LfdPhotoAcc acc;
    lfd_photo_clear(acc);
    for (int dy = -R; dy <= R; ++dy) {
        const int qy = y + dy;
        if (qy < 0 || qy >= g.H) continue;
        for (int dx = -R; dx <= R; ++dx) {
            const int qx = x + dx;
            if (qx < 0 || qx >= g.W) continue;
            const size_t q = (size_t)qy * g.W + qx;
            const float* wp = w.warp + q * g.C;
            if (!lfd_photo_participates(mask_a, w.mask_b, g, qx, qy, w.cert[q], wp[g.C - 2], wp[g.C - 1])) continue;
            const float xan = g.C == 4 ? wp[0] : ax[qx], yan = g.C == 4 ? wp[1] : ay[qy];
            lfd_photo_sample(acc, img_a, w.img, g, xan, yan, wp[g.C - 2], wp[g.C - 1]);
        }
    }
    return lfd_photo_verdict(acc, R, th, ncc);
}

// What the gate's own launch works on (device), by value in the kernel arguments.
struct LfdPhotoArgs {
    LfdPointStage st;                  // (g.tau, g.reproj_thresh unused)
    const uint8_t* const* img;         // [n_refs * k] the neighbours' match-size images (device table)
    int32_t* seg_counts;               // [n_refs * k] or null (zeroed before the launch)
    uint8_t* status;                   // [capacity] or null
    float* ncc;                        // [capacity] or null
    unsigned long long* counters;      // [5] or null: points per status; added to
    uint8_t* keep;                     // workspace [n_wg * 256]: 1 kept, 0 dropped
    unsigned* wg_kept;                 // workspace [n_wg + 1]: kept points per workgroup
    int32_t radius;
    LfdPhotoThresh th;
};

// Arguments of lfd_photo_gate / lfd_photo_gate_host that do not depend on the batch; what is wrong with them (and the status), or null.
inline const char* lfd_photo_check(const lfd_points* in, const int64_t* ref_offsets_in, const uint8_t* const* nbr_image, int32_t window_cells,
                                   float min_ncc, float min_texture, const lfd_points* out, const int64_t* ref_offsets_out,
                                   const uint8_t* status, const float* ncc, const int64_t* counters, int* code) {
    *code = LFD_ERR_INVALID;
    if (!nbr_image) return "null nbr_image";
    if (window_cells < 1 || window_cells > LFD_PHOTO_MAX_RADIUS) return "window_cells must be in [1, 3]";
    if (!(min_ncc > 0.0f) || !(min_ncc <= 1.0f)) return "min_ncc must be in (0, 1]";
    if (!(min_texture >= 0.0f) || !(min_texture <= 3.4028234e38f)) return "min_texture must be finite and >= 0";
    int sup_code = LFD_ERR_INVALID;
    const char* why = lfd_support_check(in, ref_offsets_in, 1, 1.0f, out, ref_offsets_out, &sup_code);
    if (why && sup_code != LFD_ERR_CAPACITY) return why;
    const long long cap = in->capacity;
    const struct { const void* p; long long bytes; } a[10] = {{in->xyz, 12 * cap}, {in->rgb, 12 * cap}, {in->err, 4 * cap}, {in->cell, 4 * cap},
                                                             {in->slot, cap}, {out->xyz, 12 * out->capacity}, {out->rgb, 12 * out->capacity},
                                                             {out->err, 4 * out->capacity}, {out->cell, 4 * out->capacity},
                                                             {out->slot, out->capacity}},
                                                      b[3] = {{status, cap}, {ncc, 4 * cap}, {counters, 8 * LFD_PHOTO_STATUSES}};
    for (int j = 0; j < 3; ++j) {
        if (!b[j].p) continue;
        const uintptr_t b0 = reinterpret_cast<uintptr_t>(b[j].p), b1 = b0 + (uintptr_t)(b[j].bytes > 0 ? b[j].bytes : 1);
        for (int i = 0; i < 10; ++i) {
            if (!a[i].p) continue;
            const uintptr_t a0 = reinterpret_cast<uintptr_t>(a[i].p), a1 = a0 + (uintptr_t)a[i].bytes;
            if (a0 < b1 && b0 < a1) return "status / ncc / counters must overlap nothing of in or out";
        }
        for (int i = 0; i < j; ++i) {
            if (!b[i].p) continue;
            const uintptr_t a0 = reinterpret_cast<uintptr_t>(b[i].p), a1 = a0 + (uintptr_t)(b[i].bytes > 0 ? b[i].bytes : 1);
            if (a0 < b1 && b0 < a1) return "status, ncc and counters overlap each other";
        }
    }
    if (why) { *code = LFD_ERR_CAPACITY; return why; }
    return nullptr;
}
