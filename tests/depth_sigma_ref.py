"""The yardstick of the depth-uncertainty gate's tests (lfd_depth_sigma_filter): sigma_rel in f64 NumPy from the f32 inputs.

    X(l) = C_A + l D, D = X - C_A                      the point along the reference's ray, l = 1 at the point
    (px, py, pz) = P_j (X, 1),  h = P_j[:, :3] D       view j
    g  = (hx / pz - px hz / pz^2, hy / pz - py hz / pz^2)                 image motion per unit l [camera px]
    I_j = p00 gx^2 + 2 p01 gx gy + p11 gy^2            p: the view's precision [camera px^-2]
    sigma_rel = 1 / sqrt(sum_j I_j)                    +inf where the sum is not finite or <= 0

The participating views are the winning slot and - where ``accepted`` - the candidates of tests/support_ref.py (live and agree at tau).  A view
with pz <= 0, a non-finite contribution or an invalid precision is skipped.  A point one of whose candidate tests lies in support_ref's rounding
band is reported in ``band``: its participating set may legitimately differ between implementations.
"""
from __future__ import annotations

import numpy as np

import support_ref

f32 = np.float32


def plane_valid(q):
    """lfd_refine_prec_valid: finite, q00 > 0, q11 > 0, det > 0 (f64 from the f32 entries).  q (n, 3) f32."""
    q = np.asarray(q, f32).astype(np.float64)
    with np.errstate(all="ignore"):
        return np.isfinite(q).all(axis=1) & (q[:, 0] > 0) & (q[:, 2] > 0) & (q[:, 0] * q[:, 2] - q[:, 1] * q[:, 1] > 0)


def view_information(P, C_A, xyz, p00, p01, p11):
    """I_j over n points (NaN / inf where undefined) and pz.  P (3, 4) f32, C_A (3,) f32, xyz (n, 3) f32, p (n,) f64."""
    P = np.asarray(P, f32).astype(np.float64).reshape(3, 4)
    X = np.asarray(xyz, f32).astype(np.float64).reshape(-1, 3)
    D = X - np.asarray(C_A, f32).astype(np.float64).reshape(1, 3)
    with np.errstate(all="ignore"):
        p = X @ P[:, :3].T + P[:, 3]
        h = D @ P[:, :3].T
        pz = p[:, 2]
        gx = h[:, 0] / pz - p[:, 0] * h[:, 2] / (pz * pz)
        gy = h[:, 1] / pz - p[:, 1] * h[:, 2] / (pz * pz)
        info = p00 * gx * gx + 2.0 * p01 * gx * gy + p11 * gy * gy
    return info, pz


def reference(cams, ri, cell, slot, xyz, w_match: int, h_match: int, accepted=None, tau: float = 0.0, iso_sigma_px: float = 0.0):
    """One reference's points.  ri: its ReferenceInputs (CPU tensors); cell (n,) i32, slot (n,) u8, xyz (n, 3) f32; accepted: None (winner only)
    or (n,) bool; iso_sigma_px > 0: the isotropic form, else ri.precision.  dict of (n,) arrays ``sigma`` f64, ``n_views`` (views that
    contributed), ``band``."""
    k = len(ri.nbr_cams)
    cell, slot = np.asarray(cell).astype(np.int64), np.asarray(slot).astype(np.int64)
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    n = cell.size
    H, W = ri.cert[0].shape
    ok = (cell >= 0) & (cell < H * W) & (slot < k)
    csafe = np.where(ok, cell, 0)
    part = np.zeros((n, k), bool)
    part[np.arange(n), np.where(ok, slot, 0)] = ok
    band = np.zeros(n, bool)
    if accepted is not None and n:
        sup = support_ref.reference(cams, ri.ref_cam, ri.nbr_cams, [c.numpy() for c in ri.cert], [w.numpy() for w in ri.warp],
                                    [m.numpy() if m is not None else None for m in ri.mask_b] if ri.mask_b is not None else None,
                                    w_match, h_match, csafe, np.where(ok, slot, 0), xyz, tau)
        acc = np.asarray(accepted, bool) & ok
        part |= sup["tested"] & sup["live"] & sup["agree"] & acc[:, None]
        band = acc & ~sup["clean"]
    total = np.zeros(n)
    n_views = np.zeros(n, np.int64)
    C_A = np.asarray(cams[ri.ref_cam].C, f32).reshape(3)
    finite_x = np.isfinite(xyz.astype(np.float64)).all(axis=1)
    for j in range(k):
        cam = cams[int(ri.nbr_cams[j])]
        if iso_sigma_px > 0.0:
            inv = 1.0 / (float(f32(iso_sigma_px)) ** 2)
            p00, p01, p11, valid = np.full(n, inv), np.zeros(n), np.full(n, inv), np.ones(n, bool)
        else:
            q = ri.precision[j].numpy().reshape(H * W, 3)[csafe]
            sx = float(support_ref.pixel_scale(cam.width, w_match))
            sy = float(support_ref.pixel_scale(cam.height, h_match))
            qd = q.astype(np.float64)
            with np.errstate(all="ignore"):
                p00, p01, p11 = qd[:, 0] / (sx * sx), qd[:, 1] / (sx * sy), qd[:, 2] / (sy * sy)
            valid = plane_valid(q)
        info, pz = view_information(np.asarray(cam.P, f32), C_A, xyz, p00, p01, p11)
        with np.errstate(invalid="ignore"):
            use = part[:, j] & valid & finite_x & (pz > 0) & np.isfinite(info)
        total += np.where(use, info, 0.0)
        n_views += use
    with np.errstate(all="ignore"):
        sigma = np.where(np.isfinite(total) & (total > 0), 1.0 / np.sqrt(total), np.inf)
    return dict(sigma=sigma, n_views=n_views, band=band)


def over_references(cams, refs, src, w_match: int, h_match: int, status=None, tau: float = 0.0, iso_sigma_px: float = 0.0):
    """``reference`` over every reference of a collected result ``src`` for the ReferenceInputs ``refs``; status: None or the refinement's u8
    status of the points (0x80 = accepted).  The dicts' arrays concatenated in the result's order."""
    off = np.asarray(src.ref_offsets)
    cell, slot, xyz = src.cell.cpu().numpy(), src.slot.cpu().numpy(), src.xyz.cpu().numpy()
    acc = None if status is None else (np.asarray(status.cpu().numpy() if hasattr(status, "cpu") else status) & 0x80) != 0
    parts = []
    for r, ri in enumerate(refs):
        a, b = int(off[r]), int(off[r + 1])
        parts.append(reference(cams, ri, cell[a:b], slot[a:b], xyz[a:b], w_match, h_match, None if acc is None else acc[a:b], tau, iso_sigma_px))
    return {name: np.concatenate([p[name] for p in parts]) if parts else np.zeros(0) for name in ("sigma", "n_views", "band")}


def depth_z(xyz, truth, C_A, sigma):
    """z = ((X - X_true) . D / |D|^2) / sigma_rel, D = X - C_A: the depth error along the ray in units of the predicted sigma."""
    X = np.asarray(xyz, np.float64)
    D = X - np.asarray(C_A, f32).astype(np.float64).reshape(1, 3)
    with np.errstate(all="ignore"):
        return ((X - np.asarray(truth, np.float64)) * D).sum(axis=1) / (D * D).sum(axis=1) / np.asarray(sigma, np.float64)
