"""The yardstick of the tests of lfd_estimate_normals: an f64 NumPy restatement of the contract in include/lfd_densify.h with its
own two-view DLT (np.linalg.svd in f64), its own window rules and its own sums - nothing of the library runs here.

Per input point it gives the normal, the status the contract asks for, whether any decision about one of its window cells is IN BAND, and a
bound on the angle between this normal and an implementation's.

    delta     the library's per-cell point Y_q is within delta = 1e-5 |Y| + 1e-6 per coordinate of the f64 one: the tolerance
              tests/test_host_twin.py grants the per-cell routine
    in band   the two-view test of q: support_ref.pair_test's rule for either view (|e - thresh| <= B, or the sign of a depth within rounding) with
              B widened by what delta moves a projection by, sqrt(3) delta (|P0| + |P1| + (|u| + |v|) |P2|) / pz (rows of P without the last
              column, Euclidean norms).  The depth step of q: the same rule applied to |pz_q - pz_X| against depth_step_rel pz_X - the two depths'
              f32 evaluation errors E(z) (four roundings of a partial sum each, as in support_ref), one rounding of the difference and one of the
              product, and sqrt(3) delta |P2| for Y_q.  Whether q is live involves no rounding.
              Outside the band every implementation must take this decision; a point none of whose live in-grid cells is in band must come out
              with this status.
    angle     U = n sum dx D - sum dx sum D moves by at most sqrt(3) delta_max sum_q |n dx_q - sx| when every Y_q moves by delta (delta_max: the
              largest over the window), V likewise; to first order the direction of N = U x V turns by (|dU| |V| + |U| |dV|) / |U x V|.  Added
              to it: sqrt(3) 2^-24 for the rounding of the result's components to f32.
"""
from __future__ import annotations

import numpy as np

import support_ref
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

f32 = np.float32
U24 = 2.0 ** -24
FITTED = 0x80


def _px(n, size: int, scale) -> np.ndarray:
    """Normalised f32 coordinate -> camera px, f64 from the f32 inputs."""
    return (np.asarray(n, f32).astype(np.float64) + 1.0) * 0.5 * (size - 1) * float(f32(scale))


def two_view_svd(Pa, Pb, ua, va, ub, vb):
    """DLT of n correspondences: the right singular vector of the smallest singular value of the four rows u P2 - P0, v P2 - P1 of both
    views, dehomogenised.  (n, 3) f64; NaN where an input is not finite."""
    n = ua.shape[0]
    A = np.empty((n, 4, 4))
    A[:, 0] = ua[:, None] * Pa[2] - Pa[0]
    A[:, 1] = va[:, None] * Pa[2] - Pa[1]
    A[:, 2] = ub[:, None] * Pb[2] - Pb[0]
    A[:, 3] = vb[:, None] * Pb[2] - Pb[1]
    ok = np.isfinite(A).all(axis=(1, 2))
    Y = np.full((n, 3), np.nan)
    if ok.any():
        v = np.linalg.svd(A[ok])[2][:, 3, :]
        with np.errstate(all="ignore"):
            Y[ok] = v[:, :3] / v[:, 3:4]
    return Y


def _depth(P, X):
    """Row 2 of P applied to (X, 1) in f64 and the f32 evaluation error of the library's fma chain (support_ref's E)."""
    s1 = X[:, 0] * P[2, 0]
    s2 = s1 + X[:, 1] * P[2, 1]
    s3 = s2 + X[:, 2] * P[2, 2]
    s4 = s3 + P[2, 3]
    return s4, U24 * (np.abs(s1) + np.abs(s2) + np.abs(s3) + np.abs(s4))


def cell_points(cams, ri, w_match: int, h_match: int, reproj_thresh: float):
    """Every cell of every slot of one reference through the two-view routine.  List over slots of dicts of (H*W, ...) arrays: ``Y`` f64,
    ``keep`` the reference's decision, ``band`` whether it is in band, ``delta`` the per-coordinate tolerance of Y."""
    ca = cams[ri.ref_cam]
    Pa = np.asarray(ca.P, f32).astype(np.float64)
    H, W = ri.cert[0].shape
    out = []
    for j, nb in enumerate(ri.nbr_cams):
        cb = cams[nb]
        Pb = np.asarray(cb.P, f32).astype(np.float64)
        w = ri.warp[j].cpu().numpy().reshape(H * W, -1)
        if w.shape[1] == 4:
            xa, ya = w[:, 0], w[:, 1]
        else:
            xa = np.tile(hb.identity_axis(W), H)
            ya = np.repeat(hb.identity_axis(H), W)
        xb, yb = w[:, -2], w[:, -1]
        sa = (support_ref.pixel_scale(ca.width, w_match), support_ref.pixel_scale(ca.height, h_match))
        sb = (support_ref.pixel_scale(cb.width, w_match), support_ref.pixel_scale(cb.height, h_match))
        with np.errstate(all="ignore"):
            ua, va = _px(xa, w_match, sa[0]), _px(ya, h_match, sa[1])
            ub, vb = _px(xb, w_match, sb[0]), _px(yb, h_match, sb[1])
            Y = two_view_svd(Pa, Pb, ua, va, ub, vb)
            delta = 1e-5 * np.abs(Y).max(axis=1) + 1e-6
            keep = np.ones(H * W, bool)
            band = np.zeros(H * W, bool)
            for P, cam_sc, xn, yn, u, v in ((Pa, sa, xa, ya, ua, va), (Pb, sb, xb, yb, ub, vb)):
                t = support_ref.pair_test(P.astype(f32), cam_sc[0], cam_sc[1], Y.astype(f32), xn, yn, w_match, h_match, reproj_thresh)
                dE = np.sqrt(3.0) * delta * (np.linalg.norm(P[0, :3]) + np.linalg.norm(P[1, :3]) + (np.abs(u) + np.abs(v)) * np.linalg.norm(P[2, :3])) / np.abs(t["pz"])
                keep &= t["agree"]
                band |= t["band"] | (np.isfinite(t["e"]) & (np.abs(t["e"] - float(f32(reproj_thresh))) <= t["bound"] + dE))
            keep &= np.isfinite(Y).all(axis=1)
        out.append(dict(Y=Y, keep=keep, band=band & np.isfinite(Y).all(axis=1), delta=delta))
    return out


def reference(cams, ri, w_match: int, h_match: int, cell, slot, xyz, radius: int, depth_step_rel: float, reproj_thresh: float, cells=None):
    """One reference's points.  ri: its ReferenceInputs (CPU or device tensors); cell (n,) i32, slot (n,) u8, xyz (n, 3) f32.  dict of (n,)
    arrays ``normal`` (n, 3) f64, ``status`` (the contract's byte), ``count`` (cells that took part), ``flagged`` (some decision of a live
    in-grid window cell is in band), ``bound`` (rad; inf where the fit is degenerate).  ``cells``: a cached ``cell_points`` result."""
    ca = cams[ri.ref_cam]
    Pa = np.asarray(ca.P, f32).astype(np.float64)
    Ca = np.asarray(ca.C, f32).astype(np.float64)
    H, W = ri.cert[0].shape
    k = len(ri.nbr_cams)
    if cells is None:
        cells = cell_points(cams, ri, w_match, h_match, reproj_thresh)
    cell, slot = np.asarray(cell).astype(np.int64), np.asarray(slot).astype(np.int64)
    X = np.asarray(xyz, f32).astype(np.float64).reshape(-1, 3)
    n = cell.size
    step = float(f32(depth_step_rel))
    with np.errstate(all="ignore"):
        Vw = Ca[None, :] - X
        vn = np.linalg.norm(Vw, axis=1)
        fallback = np.where((np.isfinite(vn) & (vn > 0))[:, None], Vw / vn[:, None], 0.0)
        pzX, EzX = _depth(Pa, X)
        ok = np.isfinite(X).all(axis=1) & (cell >= 0) & (cell < H * W) & (slot < k) & (pzX > 0)
    fallback[~np.isfinite(fallback).all(axis=1)] = 0.0
    y, x = np.where(ok, cell, 0) // W, np.where(ok, cell, 0) % W
    sj = np.where(ok, slot, 0)
    cert = np.stack([c.cpu().numpy().reshape(-1) for c in ri.cert])
    Yall = np.stack([c["Y"] for c in cells])
    keep_all, band_all, delta_all = (np.stack([c[name] for c in cells]) for name in ("keep", "band", "delta"))
    warp_b = np.stack([w.cpu().numpy().reshape(H * W, -1)[:, -2:] for w in ri.warp])
    mask_a = ri.mask_a.cpu().numpy() if ri.mask_a is not None else None
    cnt = np.zeros(n, np.int64)
    sx, sy, sxx, sxy, syy = (np.zeros(n, np.int64) for _ in range(5))
    A0, Ax, Ay = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
    flagged = np.zeros(n, bool)
    dmax = np.zeros(n)
    offs = []
    norm_p2 = np.linalg.norm(Pa[2, :3])
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            qy, qx = y + dy, x + dx
            inside = ok & (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
            q = np.where(inside, qy * W + qx, 0)
            with np.errstate(all="ignore"):
                live = inside & (cert[sj, q] > 0)
                if ri.mask_b is not None:
                    for j in range(k):
                        if ri.mask_b[j] is not None:
                            mine = live & (sj == j)
                            wb = warp_b[j][q]
                            live &= ~mine | support_ref.mask_lookup(ri.mask_b[j].cpu().numpy(), wb[:, 0], wb[:, 1], H, W, w_match, h_match)
                if mask_a is not None:
                    mx = support_ref.nearest_src(np.where(inside, qx, 0), f32(w_match) / f32(W), w_match)
                    my = support_ref.nearest_src(np.where(inside, qy, 0), f32(h_match) / f32(H), h_match)
                    live &= mask_a[my, mx] != 0
                Y = Yall[sj, q]
                keep = keep_all[sj, q]
                delta = delta_all[sj, q]
                pzq, Ezq = _depth(Pa, np.where(np.isfinite(Y), Y, 0.0))
                d, t = pzq - pzX, step * pzX
                near = np.abs(d) <= t
                Bd = Ezq + (1.0 + step) * EzX + np.sqrt(3.0) * delta * norm_p2 + U24 * (np.abs(d) + 2.0 * np.abs(t))
                band = band_all[sj, q] | (keep & (np.abs(np.abs(d) - t) <= Bd))
            flagged |= live & band
            take = live & keep & near
            D = np.where(take[:, None], Y - X, 0.0)
            A0 += D
            Ax += dx * D
            Ay += dy * D
            cnt += take
            sx += dx * take
            sy += dy * take
            sxx += dx * dx * take
            sxy += dx * dy * take
            syy += dy * dy * take
            dmax = np.maximum(dmax, np.where(take, delta, 0.0))
            offs.append((dx, dy, take))
    a, b, c = cnt * sxx - sx * sx, cnt * sxy - sx * sy, cnt * syy - sy * sy
    fit = ok & (a * c - b * b > 0)
    with np.errstate(all="ignore"):
        Uv = cnt[:, None] * Ax - sx[:, None] * A0
        Vv = cnt[:, None] * Ay - sy[:, None] * A0
        N = np.cross(Uv, Vv)
        nn = (N * N).sum(axis=1)
        fit &= np.isfinite(nn) & (nn > 0)
        N = np.where(((N * Vw).sum(axis=1) < 0)[:, None], -N, N)
        unit = N / np.sqrt(nn)[:, None]
        lever_x, lever_y = np.zeros(n), np.zeros(n)
        for dx, dy, take in offs:
            lever_x += take * np.abs(cnt * dx - sx)
            lever_y += take * np.abs(cnt * dy - sy)
        dU, dV = np.sqrt(3.0) * dmax * lever_x, np.sqrt(3.0) * dmax * lever_y
        bound = (dU * np.linalg.norm(Vv, axis=1) + np.linalg.norm(Uv, axis=1) * dV) / np.sqrt(nn) + np.sqrt(3.0) * U24
    normal = np.where(fit[:, None], unit, fallback)
    status = np.where(ok, cnt, 0) | np.where(fit, FITTED, 0)
    return dict(normal=normal, status=status.astype(np.int64), count=np.where(ok, cnt, 0), flagged=flagged, bound=np.where(fit, bound, np.inf),
                fitted=fit, fallback=fallback)


def over_references(cams, refs, src, w_match: int, h_match: int, radius: int, depth_step_rel: float, reproj_thresh: float, cache=None):
    """``reference`` over every reference of a collected result, concatenated in the points' order.  ``cache``: a dict that keeps the per-cell
    points of every reference between calls (they do not depend on the radius or the depth step)."""
    off = np.asarray(src.ref_offsets)
    cell, slot, xyz = src.cell.cpu().numpy(), src.slot.cpu().numpy(), src.xyz.cpu().numpy()
    parts = []
    for r, ri in enumerate(refs):
        a, b = int(off[r]), int(off[r + 1])
        cells = None
        if cache is not None:
            key = (r, float(reproj_thresh))
            if key not in cache:
                cache[key] = cell_points(cams, ri, w_match, h_match, reproj_thresh)
            cells = cache[key]
        parts.append(reference(cams, ri, w_match, h_match, cell[a:b], slot[a:b], xyz[a:b], radius, depth_step_rel, reproj_thresh, cells))
    return {name: np.concatenate([p[name] for p in parts]) for name in parts[0]}
