"""The yardstick of the multi-view colour's tests (lfd_colour_multiview): a NumPy evaluation of the rule as the header states
it, operation by operation in f32, so that it can be compared with the library bit for bit.

Per point X of a reference, made by winning slot s on cell c:

    guard    X or its colour not finite, c outside the grid, s >= number of slots: the colour stays, status 0
    views    the reference (the colour the point has); slot s unless its observation is not finite; every slot j != s, ascending, that is live
             (raw certainty > 0, mask pixel set: tests/support_ref.py's lookup) and agrees with X within tau - the support filter's test
    colour   of a neighbour: the four-tap f32 blend of its match-size image at ((xb + 1) 0.5) (w_match - 1), ((yb + 1) 0.5) (h_match - 1)
    mean     sum = c_ref; sum += c_s; sum += c_j ...; sum * RN_f32(1 / n)
    median   per channel the middle value of the n in ascending order; (lo + hi) * 0.5 of the two middle ones for even n

A fused multiply-add is a * b + c in f64 rounded to f32: the product of two f32 is exact in f64, so only the sum rounds before the final
rounding (a double rounding that could differ from one f32 rounding needs the f64 sum to land on an f32 midpoint - 29 zero bits in a row).
"""
from __future__ import annotations

import numpy as np

import support_ref

f32 = np.float32
RECIP = np.array([0.0] + [1.0 / n for n in range(1, 18)], np.float64).astype(f32)        # RN_f32(1 / n), n = 1 .. 17
INV255 = f32(1.0 / 255.0)


def fma(a, b, c):
    return (np.asarray(a, f32).astype(np.float64) * np.asarray(b, f32).astype(np.float64) + np.asarray(c, f32).astype(np.float64)).astype(f32)


def match_px(n, size_m1):
    return ((np.asarray(n, f32) + f32(1.0)) * f32(0.5)) * f32(size_m1)


def bilinear(img, x, y):
    """img (h, w, 3) u8, x / y (n,) f32 match px -> (n, 3) f32 in [0, 1]: taps floor / floor + 1 clamped to the image, weights (x1 - x)(y1 - y) ...,
    blended d wd + (c wc + (b wb + a wa)) with fused multiply-adds, times RN_f32(1 / 255); a clamped column folds its two weights."""
    h, w = img.shape[:2]
    x, y = np.asarray(x, f32), np.asarray(y, f32)
    x0 = np.minimum(np.maximum(np.floor(x), f32(0.0)), f32(w - 1))
    y0 = np.minimum(np.maximum(np.floor(y), f32(0.0)), f32(h - 1))
    x1 = np.minimum(x0 + f32(1.0), f32(w - 1))
    y1 = np.minimum(y0 + f32(1.0), f32(h - 1))
    ax, bx, ay, by = x1 - x, x - x0, y1 - y, y - y0
    wa, wb, wc, wd = ax * ay, bx * ay, ax * by, bx * by
    clamped = x1 == x0
    wa, wc = np.where(clamped, wa + wb, wa), np.where(clamped, wc + wd, wc)
    wb, wd = np.where(clamped, f32(0.0), wb), np.where(clamped, f32(0.0), wd)
    ix0, iy0, ix1, iy1 = x0.astype(np.int64), y0.astype(np.int64), x1.astype(np.int64), y1.astype(np.int64)
    a, b, c, d = (img[iy, ix].astype(f32) for iy, ix in ((iy0, ix0), (iy0, ix1), (iy1, ix0), (iy1, ix1)))
    out = np.empty((x.size, 3), f32)
    for ch in range(3):
        s = fma(d[:, ch], wd, fma(c[:, ch], wc, fma(b[:, ch], wb, a[:, ch] * wa)))
        out[:, ch] = s * INV255
    return out


def agree(P, sx, sy, xyz, xb, yb, w_match, h_match, tau):
    """The support filter's comparison in f32: rows of P as forward fused chains, cross-multiplied by the depth, nothing divided."""
    P = np.asarray(P, f32).reshape(3, 4)
    X = np.asarray(xyz, f32)
    ub = match_px(xb, w_match - 1) * f32(sx)
    vb = match_px(yb, h_match - 1) * f32(sy)
    row = lambda i: fma(f32(1.0), P[i, 3], fma(X[:, 2], P[i, 2], fma(X[:, 1], P[i, 1], X[:, 0] * P[i, 0])))
    px, py, pz = row(0), row(1), row(2)
    du, dv = px - ub * pz, py - vb * pz
    d2 = du * du + dv * dv
    t = f32(tau) * pz
    return (pz > 0) & (d2 <= t * t)


def reference(cams, ref_cam, nbr_cams, cert, warp, masks_b, nbr_images, w_match, h_match, cell, slot, xyz, rgb, tau, mode):
    """One reference's points.  cert [k] (H, W) f32, warp [k] (H, W, 2 | 4) f32, masks_b None or [k] of None / (h_match, w_match) u8, nbr_images
    [k] (h_match, w_match, 3) u8; cell (n,) i32, slot (n,) u8, xyz / rgb (n, 3) f32; mode "mean" | "median".  Returns (rgb (n, 3) f32, status (n,) u8)."""
    k = len(nbr_cams)
    cell, slot = np.asarray(cell).astype(np.int64), np.asarray(slot).astype(np.int64)
    xyz, rgb = np.asarray(xyz, f32).reshape(-1, 3), np.asarray(rgb, f32).reshape(-1, 3)
    n = cell.size
    H, W = np.asarray(cert[0]).shape
    guard = ~(np.isfinite(xyz).all(axis=1) & np.isfinite(rgb).all(axis=1)) | (cell < 0) | (cell >= H * W) | (slot >= k)
    cs, ss = np.where(guard, 0, cell), np.where(guard, 0, slot)
    with np.errstate(all="ignore"):
        part = np.zeros((n, k), bool)
        col = np.zeros((n, k, 3), f32)
        for j in range(k):
            cam = cams[int(nbr_cams[j])]
            wj = np.asarray(warp[j], f32).reshape(H * W, -1)[cs]
            xb, yb = wj[:, -2], wj[:, -1]
            live = np.asarray(cert[j], f32).reshape(-1)[cs] > 0
            if masks_b is not None and masks_b[j] is not None:
                live &= support_ref.mask_lookup(np.asarray(masks_b[j]), xb, yb, H, W, w_match, h_match)
            ok = live & agree(cam.P, support_ref.pixel_scale(cam.width, w_match), support_ref.pixel_scale(cam.height, h_match), xyz, xb, yb,
                              w_match, h_match, tau)
            part[:, j] = np.where(ss == j, np.isfinite(xb) & np.isfinite(yb), ok) & ~guard
            idx = np.nonzero(part[:, j])[0]
            col[idx, j] = bilinear(np.asarray(nbr_images[j]), match_px(xb[idx], w_match - 1), match_px(yb[idx], h_match - 1))
        count = 1 + part.sum(axis=1)
        rows = np.arange(n)
        if mode == "mean":
            total = rgb.copy()
            win = part[rows, ss]
            total = np.where(win[:, None], total + col[rows, ss], total)
            for j in range(k):
                take = part[:, j] & (ss != j)
                total = np.where(take[:, None], total + col[:, j], total)
            out = total * RECIP[count][:, None]
        elif mode == "median":
            vals = np.concatenate([rgb[:, None, :], np.where(part[:, :, None], col, f32(np.inf))], axis=1)
            vals = np.sort(vals, axis=1)
            lo, hi = vals[rows, (count - 1) // 2], vals[rows, count // 2]
            out = np.where((count % 2 == 1)[:, None], lo, (lo + hi) * f32(0.5))
        else:
            raise ValueError(mode)
    out = out.astype(f32)
    out.view(np.uint32)[guard] = np.ascontiguousarray(rgb).view(np.uint32)[guard]
    return out, np.where(guard, 0, count).astype(np.uint8)


def batch_reference(cams, refs, nbr_images, w_match, h_match, res, tau, mode):
    """Every reference of a collected result ``res`` for the ReferenceInputs ``refs`` (CPU tensors); nbr_images [r][j] arrays."""
    off = np.asarray(res.ref_offsets)
    cell, slot, xyz, rgb = res.cell.cpu().numpy(), res.slot.cpu().numpy(), res.xyz.cpu().numpy(), res.rgb.cpu().numpy()
    out, status = np.empty_like(rgb), np.empty(cell.shape, np.uint8)
    for r, ri in enumerate(refs):
        a, b = int(off[r]), int(off[r + 1])
        out[a:b], status[a:b] = reference(cams, ri.ref_cam, ri.nbr_cams, [c.cpu().numpy() for c in ri.cert], [w.cpu().numpy() for w in ri.warp],
                                          [m.cpu().numpy() if m is not None else None for m in ri.mask_b] if ri.mask_b is not None else None,
                                          [np.asarray(im) for im in nbr_images[r]], w_match, h_match, cell[a:b], slot[a:b], xyz[a:b], rgb[a:b],
                                          tau, mode)
    return out, status
