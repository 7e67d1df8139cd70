"""The yardstick of the multi-view support filter's tests (lfd_support_filter): an f64 evaluation, from the f32 inputs, of one
(point, other neighbour) test

    live     = the neighbour's raw certainty at the point's cell is > 0 and, with a mask, the mask pixel its warp points at is set
    (ub, vb) = ((xb + 1) 0.5 (w_match - 1) sx, (yb + 1) 0.5 (h_match - 1) sy)        the neighbour's own observation of the cell [camera px]
    (px, py, pz) = P (X, 1)                                                          the triangulated point in the neighbour
    e        = hypot(px / pz - ub, py / pz - vb)                                     [camera px of the neighbour]
    agree    = pz > 0 and e <= tau

and the derived first-order bound B on what the library's f32 evaluation can move e by.  The library never divides: it compares
d2 = du du + dv dv, du = px - ub pz, dv = py - vb pz, with the square of t = tau pz.  For pz > 0 this is D = hypot(du, dv) = e pz against tau pz,
so an error dD of D and dT of t move the quantity compared with tau by (dD + dT) / pz.  With u = 2^-24 (every f32 operation is correctly
rounded: relative error at most u):

  projection  a row is fmaf(1, P3, fmaf(X2, P2, fmaf(X1, P1, X0 P0))): FOUR roundings, each of a partial sum s1 = X0 P0, s2 = s1 + X1 P1,
              s3 = s2 + X2 P2, s4 = s3 + P3, each by at most u |s_i|:   E(row) = u (|s1| + |s2| + |s3| + |s4|)
  pixels      xb + 1, the product with (w_match - 1) (the factor 0.5 is exact) and the product with sx round once each, all relative to the
              value:   |d ub| <= 3 u |ub|, |d vb| <= 3 u |vb|
  cross       ub pz rounds once and inherits both operands' errors:   |d (ub pz)| <= |ub| E(z) + 3 u |ub| pz + u |ub| pz;  the subtraction
              rounds once:   |d du| <= E(x) + |ub| E(z) + 4 u |ub| pz + u |du|, likewise dv with E(y), vb
  norm        the two squares and their sum round once each, relative to d2; the root halves that:   dD <= |d du| + |d dv| + 2 u D
  threshold   t = tau pz rounds once and inherits E(z), its square rounds once (half of it on t):   dT <= tau E(z) + 2 u tau pz

    B = (E(x) + E(y) + (|ub| + |vb| + tau) E(z) + 4 u pz (|ub| + |vb|) + u (|du| + |dv|) + 2 u D + 2 u tau pz) / pz

A test is IN BAND when |e - tau| <= B, or when |pz| <= E(z) (the sign of the depth itself is within rounding); outside the band every
implementation must take the reference's decision, inside it may take either.  A test with a non-finite observation or projection has no band:
it does not agree.  Whether a neighbour is live involves no rounding that could differ (a comparison with 0, index arithmetic written out in f32
and repeated here operation by operation).
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
f32 = np.float32


def pixel_scale(cam_size: int, match_size: int) -> np.float32:
    """Camera px per match px as the library forms it: (float) (w_cam / (double) w_match)."""
    return f32(float(cam_size) / float(match_size))


def grid_nearest(g, size: int):
    """F.grid_sample(mode='nearest', align_corners=False) index in f32 (lfd_grid_nearest), -1 = outside (NaN and inf included)."""
    g = np.asarray(g, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        f = ((g + f32(1.0)) * f32(size) - f32(1.0)) / f32(2.0)
        r = np.rint(f)
        ok = (r >= 0) & (r <= size - 1)
    return np.where(ok, np.where(ok, r, 0).astype(np.int64), -1)


def nearest_src(dst, scale: np.float32, in_size: int):
    """F.interpolate(mode='nearest') source index (lfd_nearest_src)."""
    s = np.floor(np.asarray(dst).astype(f32) * f32(scale)).astype(np.int64)
    return np.minimum(s, in_size - 1)


def mask_lookup(mask, xb, yb, H: int, W: int, w_match: int, h_match: int):
    """The pixel of ``mask`` (h_match, w_match) the normalised coordinate points at, as the kernels' certainty prologue finds it; False outside."""
    ix, iy = grid_nearest(xb, W), grid_nearest(yb, H)
    ok = (ix >= 0) & (iy >= 0)
    sx, sy = f32(w_match) / f32(W), f32(h_match) / f32(H)
    mx, my = nearest_src(np.where(ok, ix, 0), sx, w_match), nearest_src(np.where(ok, iy, 0), sy, h_match)
    return ok & (np.asarray(mask)[my, mx] != 0)


def pair_test(P, sx, sy, xyz, xb, yb, w_match: int, h_match: int, tau: float):
    """One other neighbour over n points.  P (3, 4) f32, sx / sy f32 scalars, xyz (n, 3) f32, xb / yb (n,) f32 normalised.  dict of (n,) arrays:
    ``e`` f64 residual in px (NaN / inf where undefined), ``pz`` f64, ``bound`` f64 B, ``agree`` the reference's decision, ``band``."""
    P = np.asarray(P, f32).astype(np.float64).reshape(3, 4)
    X = np.asarray(xyz, f32).astype(np.float64).reshape(-1, 3)
    xb, yb = np.asarray(xb, f32).astype(np.float64), np.asarray(yb, f32).astype(np.float64)
    sx, sy, tau = float(f32(sx)), float(f32(sy)), float(f32(tau))
    with np.errstate(all="ignore"):
        ub = (xb + 1.0) * 0.5 * (w_match - 1) * sx
        vb = (yb + 1.0) * 0.5 * (h_match - 1) * sy
        rows, errs = [], []
        for i in range(3):
            s1 = X[:, 0] * P[i, 0]
            s2 = s1 + X[:, 1] * P[i, 1]
            s3 = s2 + X[:, 2] * P[i, 2]
            s4 = s3 + P[i, 3]
            rows.append(s4)
            errs.append(U * (np.abs(s1) + np.abs(s2) + np.abs(s3) + np.abs(s4)))
        px, py, pz = rows
        Ex, Ey, Ez = errs
        e = np.hypot(px / pz - ub, py / pz - vb)
        du, dv = px - ub * pz, py - vb * pz
        D = np.hypot(du, dv)
        a = np.abs(ub) + np.abs(vb)
        bound = (Ex + Ey + (a + tau) * Ez + 4 * U * np.abs(pz) * a + U * (np.abs(du) + np.abs(dv)) + 2 * U * D + 2 * U * tau * np.abs(pz)) / np.abs(pz)
        finite = np.isfinite(ub) & np.isfinite(vb) & np.isfinite(px) & np.isfinite(py) & np.isfinite(pz)
        agree = finite & (pz > 0) & (e <= tau)
        band = finite & ((np.abs(pz) <= Ez) | ((pz > 0) & (np.abs(e - tau) <= bound)))
    return dict(e=e, pz=pz, bound=bound, agree=agree, band=band)


def reference(cams, ref_cam: int, nbr_cams, cert, warp, masks_b, w_match: int, h_match: int, cell, slot, xyz, tau: float):
    """All tests of one reference's points.  cams: the run's camera records; cert [k] (H, W) f32, warp [k] (H, W, 2 | 4) f32, masks_b None or
    [k] of None / (h_match, w_match) u8; cell (n,) i32, slot (n,) u8, xyz (n, 3) f32.  dict of (n, k) arrays ``tested`` (j != slot), ``live``,
    ``e``, ``bound``, ``agree``, ``band`` and of (n,) arrays ``support`` (live and agree, the reference's count), ``clean`` (no live test of the
    point is in band: its count must be the reference's)."""
    k = len(nbr_cams)
    cell, slot = np.asarray(cell).astype(np.int64), np.asarray(slot).astype(np.int64)
    n = cell.size
    H, W = np.asarray(cert[0]).shape
    out = {name: np.zeros((n, k), dt) for name, dt in (("tested", bool), ("live", bool), ("agree", bool), ("band", bool))}
    out["e"], out["bound"] = np.full((n, k), np.nan), np.full((n, k), np.nan)
    for j in range(k):
        cam = cams[int(nbr_cams[j])]
        wj = np.asarray(warp[j], f32).reshape(H * W, -1)[cell]
        xb, yb = wj[:, -2], wj[:, -1]
        with np.errstate(invalid="ignore"):
            live = np.asarray(cert[j], f32).reshape(-1)[cell] > 0
        if masks_b is not None and masks_b[j] is not None:
            live &= mask_lookup(np.asarray(masks_b[j]), xb, yb, H, W, w_match, h_match)
        t = pair_test(np.asarray(cam.P, f32), pixel_scale(cam.width, w_match), pixel_scale(cam.height, h_match), xyz, xb, yb, w_match, h_match, tau)
        out["tested"][:, j] = slot != j
        out["live"][:, j] = live
        for name in ("e", "bound", "agree", "band"):
            out[name][:, j] = t[name]
    counted = out["tested"] & out["live"]
    out["support"] = (counted & out["agree"]).sum(axis=1)
    out["clean"] = ~(counted & out["band"]).any(axis=1)
    return out
