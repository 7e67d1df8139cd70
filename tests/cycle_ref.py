"""The yardstick of the forward-backward gate's tests (lfd_cycle_gate): an f64 evaluation, from the f32 inputs, of

    c        = certainty floored at the threshold
    (xb, yb) = the forward warp of the cell; outside [-1, 1]^2 or NaN: rejected, error +inf
    ix, iy   = ((xb + 1) Wb - 1) / 2, ((yb + 1) Hb - 1) / 2
    (xa', ya') = bilinear blend of warp_BA at (ix, iy), taps clamped to the grid (grid_sample: border, align_corners=False)
    e        = hypot((xa' - xa) 0.5 (w_match - 1), (ya' - ya) 0.5 (h_match - 1))        [px of the match image]
    kept iff e <= tau;  cert_out = kept ? c : 0

and the derived bound B on |e_f32 - e| every implementation has to stay under.  With u = 2^-24:

  position   the f32 un-normalisation of xb rounds three times - (xb + 1) <= 2, its product with Wb <= 2 Wb, the subtraction of 1 - each by at
             most u 2 Wb before the exact halving: the tap position is off by at most delta = 3 u (max(Wb, Hb) + 1) cells per axis.  Inside a
             cell the blend f is bilinear, so f(x + a, y + b) - f(x, y) = a f_x + b f_y + a b f_xy EXACTLY, with the slopes
             f_x = (1 - wy)(v01 - v00) + wy (v11 - v10), f_y = (1 - wx)(v10 - v00) + wx (v11 - v01) at the f64 position and the twist
             f_xy = v11 - v10 - v01 + v00: the blend moves by at most delta (|f_x| + |f_y|) + delta^2 |f_xy|.  A position within delta of a
             cell boundary may be rounded across it; f is continuous there and within half a cell of texel (round ix, round iy) it stays inside
             the 3 x 3 texels round that one (indices clamped, as the taps are), where its slope along x (y) is a convex combination of
             differences of horizontally (vertically) adjacent texels: for those few cells the bound is delta (Gh + Gv) with Gh, Gv the
             largest such differences inside the window.
  blend      the two weights of an axis are exact for ix >= 1 and off by at most u / 2 below; their four products round once each (the weights'
             absolute errors add up to at most 3 u), the four products with the texels once each, and so do the three sums: at most 6 u V,
             V = max |texel| of the channel over the taps (over the window next to a cell boundary).
  pixels     the subtraction xa' - xa, the product with (w_match - 1) (the factor 0.5 is exact), the two squares, their sum and the square root
             (1 ulp on the device) round once each, all relative to the value: at most 8 u e.

    B = 0.5 (w_match - 1) (P_x + 6 u V_x) + 0.5 (h_match - 1) (P_y + 6 u V_y) + 8 u e,    P = the position term of the channel

The decision compares d2 with the f32 square of tau, which is tau^2 (1 + u) at worst: tau itself moves by at most u tau.  A cell is IN BAND when
|e - tau| <= B + u tau; outside the band every implementation must take the reference's decision, inside it may take either.  A cell whose
forward coordinate is outside has no band: it is rejected, its error is +inf.  A NaN (from warp_BA) rejects too.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24


def delta(Hb: int, Wb: int) -> float:
    return 3.0 * U * (max(Hb, Wb) + 1)


def identity_axis(n: int) -> np.ndarray:
    """torch.linspace(-1 + 1/n, 1 - 1/n, n) element by element, as lfd_identity_axis documents it (f32)."""
    start, end = np.float32(-1.0 + 1.0 / n), np.float32(1.0 - 1.0 / n)
    step = np.float32((end - start) / np.float32(n - 1)) if n > 1 else np.float32(0.0)
    j = np.arange(n)
    lo = (start + (step * j.astype(np.float32)).astype(np.float32)).astype(np.float32)
    hi = (end - (step * (n - 1 - j).astype(np.float32)).astype(np.float32)).astype(np.float32)
    return np.where(j < n // 2, lo, hi).astype(np.float32) if n > 1 else np.array([start], np.float32)


def reference(cert, warp_ab, warp_ba, w_match: int, h_match: int, certainty_thresh: float, tau: float, axis_x=None, axis_y=None):
    """One pair.  cert (H, W), warp_ab (H, W, 2 | 4), warp_ba (Hb, Wb, 2): f32 arrays.  Returns a dict of (H, W) arrays:
    ``c`` f32 floored certainty, ``e`` f64 error in px (+inf outside), ``bound`` f64 B, ``keep`` the reference's decision, ``band`` cells where an
    implementation may decide either way, ``cert_out`` f32 what the reference emits."""
    cert, warp_ab, warp_ba = np.asarray(cert, np.float32), np.asarray(warp_ab, np.float32), np.asarray(warp_ba, np.float32)
    H, W = cert.shape
    Hb, Wb = warp_ba.shape[:2]
    C = warp_ab.shape[-1]
    th = np.float32(certainty_thresh)
    c = np.where(cert < th, th, cert).astype(np.float32)
    if C == 4:
        xa, ya = warp_ab[..., 0].astype(np.float64), warp_ab[..., 1].astype(np.float64)
    else:
        ax = identity_axis(W) if axis_x is None else np.asarray(axis_x, np.float32)
        ay = identity_axis(H) if axis_y is None else np.asarray(axis_y, np.float32)
        xa = np.broadcast_to(ax.astype(np.float64).reshape(1, W), (H, W))
        ya = np.broadcast_to(ay.astype(np.float64).reshape(H, 1), (H, W))
    xb, yb = warp_ab[..., C - 2].astype(np.float64), warp_ab[..., C - 1].astype(np.float64)
    with np.errstate(invalid="ignore"):
        inside = (xb >= -1.0) & (xb <= 1.0) & (yb >= -1.0) & (yb <= 1.0)
    sx, sy = np.where(inside, xb, 0.0), np.where(inside, yb, 0.0)
    ix, iy = ((sx + 1.0) * Wb - 1.0) / 2.0, ((sy + 1.0) * Hb - 1.0) / 2.0
    x0, y0 = np.floor(ix), np.floor(iy)
    wx1, wy1 = ix - x0, iy - y0
    cx = lambda i: np.clip(i.astype(np.int64), 0, Wb - 1)
    cy = lambda i: np.clip(i.astype(np.int64), 0, Hb - 1)
    ba = warp_ba.astype(np.float64)
    v00, v01 = ba[cy(y0), cx(x0)], ba[cy(y0), cx(x0 + 1)]
    v10, v11 = ba[cy(y0 + 1), cx(x0)], ba[cy(y0 + 1), cx(x0 + 1)]
    w = lambda a: a[..., None]
    back = w((1 - wy1) * (1 - wx1)) * v00 + w((1 - wy1) * wx1) * v01 + w(wy1 * (1 - wx1)) * v10 + w(wy1 * wx1) * v11
    sxp, syp = 0.5 * (w_match - 1), 0.5 * (h_match - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy = (back[..., 0] - xa) * sxp, (back[..., 1] - ya) * syp
        e = np.where(inside, np.hypot(dx, dy), np.inf)
    d = delta(Hb, Wb)
    with np.errstate(invalid="ignore", over="ignore"):
        # inside the cell: the exact expansion of the bilinear blend
        f_x = w(1 - wy1) * (v01 - v00) + w(wy1) * (v11 - v10)
        f_y = w(1 - wx1) * (v10 - v00) + w(wx1) * (v11 - v01)
        f_xy = v11 - v10 - v01 + v00
        pos = d * (np.abs(f_x) + np.abs(f_y)) + d * d * np.abs(f_xy)
        vmax = np.maximum(np.maximum(np.abs(v00), np.abs(v01)), np.maximum(np.abs(v10), np.abs(v11)))
        # within delta of a cell boundary: the 3 x 3 window round the nearest texel, indices clamped
        near = (wx1 < d) | (wx1 > 1.0 - d) | (wy1 < d) | (wy1 > 1.0 - d)
        if near.any():
            rx, ry = np.floor(ix[near] + 0.5), np.floor(iy[near] + 0.5)
            win = np.stack([np.stack([ba[cy(ry + j), cx(rx + i)] for i in (-1, 0, 1)], 0) for j in (-1, 0, 1)], 0)      # (3, 3, n, 2): [row, column]
            pos[near] = d * (np.abs(win[:, 1:] - win[:, :-1]).max(axis=(0, 1)) + np.abs(win[1:] - win[:-1]).max(axis=(0, 1)))
            vmax[near] = np.abs(win).max(axis=(0, 1))
        bound = sxp * (pos[..., 0] + 6 * U * vmax[..., 0]) + syp * (pos[..., 1] + 6 * U * vmax[..., 1])
        bound = bound + 8 * U * np.where(np.isfinite(e), e, 0.0)
        tau32 = float(np.float32(tau))
        keep = inside & (e <= tau32)
        band = inside & np.isfinite(e) & (np.abs(e - tau32) <= bound + U * tau32)
    cert_out = np.where(keep, c, np.float32(0.0)).astype(np.float32)
    return dict(c=c, e=e, bound=bound, keep=keep, band=band, inside=inside, cert_out=cert_out)


def check_against_reference(ref: dict, cert_out, err=None):
    """(cells out of band whose output differs from the reference's, cells in band whose output is neither c nor 0, cells whose error is outside
    the bound, share of the cells in band).  Outputs are compared as bits (a NaN certainty equals itself)."""
    out = np.asarray(cert_out, np.float32)
    same = lambda a, b: a.view(np.uint32) == b.view(np.uint32)
    zero = np.zeros_like(out)
    wrong = int((~ref["band"] & ~same(out, ref["cert_out"])).sum())
    neither = int((ref["band"] & ~same(out, ref["c"]) & ~same(out, zero)).sum())
    bad_err = 0
    if err is not None:
        err = np.asarray(err, np.float64)
        e = ref["e"]
        with np.errstate(invalid="ignore"):
            fin = np.isfinite(e)
            bad_err = int((fin & ~(np.abs(err - e) <= ref["bound"])).sum())
            bad_err += int((~ref["inside"] & ~(np.isinf(err) & (err > 0))).sum())            # outside: exactly +inf
            bad_err += int((ref["inside"] & np.isnan(e) & ~np.isnan(err)).sum())             # a NaN from warp_BA stays one
            bad_err += int((ref["inside"] & np.isinf(e) & ~(np.isinf(err) | (err > 1e30))).sum())
    return wrong, neither, bad_err, float(ref["band"].mean())


def probe_inputs(cams, ref_index, nbr_indices, H, W, w_match, h_match, device="cpu", channels=2, **kw):
    """The issue's probe: forward fields of ``synth_reference`` (0.5 px noise, 5 % outliers unless ``kw`` says otherwise) and, as the backward
    warp of every pair, the neighbour's own field towards the reference.  (cert [k], warp_ab [k], warp_ba [k]) as contiguous f32 torch tensors."""
    from lichtfeld_densification_plugin_amd import synthetic as syn
    kw = {"noise_px": 0.5, "outlier_frac": 0.05, **kw}
    s = syn.synth_reference(cams, ref_index, list(nbr_indices), H, W, w_match, h_match, device=device, channels=channels, **kw)
    back = [syn.synth_reference(cams, n, [ref_index], H, W, w_match, h_match, device=device, **kw).warp[0][..., -2:].contiguous() for n in nbr_indices]
    k = len(nbr_indices)
    return [s.cert[j].contiguous() for j in range(k)], [s.warp[j].contiguous() for j in range(k)], back
