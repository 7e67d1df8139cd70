"""The yardstick of the far-field shell's tests (lfd_far_accumulate / lfd_far_emit): a NumPy evaluation of the rule as the header
states it - the decision operation by operation in f32 (a fused multiply-add is tests/colour_ref.py's: the product exact in f64, one sum, one
rounding), the direction cell and the records in f64 - so that tables and records can be compared with the library element for element.

Per grid cell of a reference:

    d         M (u, v, 1), M = R^T K^-1 as forward fused chains, (u, v) the cell's A-coordinate in camera px
    confident raw certainty >= far_certainty (NaN: no), observation inside the neighbour's grid, mask_b (if any) set where it points
    agrees    the support filter's cross-multiplied comparison for the homogeneous point (d, 0)
    far       mask_a (if any) set at the cell, n_conf >= min(far_min_views, n_slots), n_agree == n_conf, d finite and not zero
    key       cube map of d in f64: face 2 m + (d_m < 0), the other two components over |d_m| to floor((u + 1) / 2 S), clamped
    sample    rint(d / |d| 2^30) [3], the reference image's u8 colour at the cell [3], 1
"""
from __future__ import annotations

import numpy as np

import colour_ref
import support_ref

f32 = np.float32
fma = colour_ref.fma
QUANTITIES = 7


def axis(n: int) -> np.ndarray:
    """The matcher's A-grid axis as the library forms it (lfd_make_axis / lfd_axis_value), f32."""
    start, end = f32(-1.0 + 1.0 / n), f32(1.0 - 1.0 / n)
    if n == 1:
        return np.array([start], f32)
    step = (end - start) / f32(n - 1)
    j = np.arange(n)
    lo = start + step * j.astype(f32)
    hi = end - step * (n - 1 - j).astype(f32)
    return np.where(j < n // 2, lo, hi).astype(f32)


def dir_matrix(cam) -> np.ndarray:
    """(9,) f32: R^T K^-1 of a pinhole K = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]] (lfd_far_dir_matrix)."""
    K, R = np.asarray(cam.K, f32).reshape(9), np.asarray(cam.R, f32).reshape(9)
    assert K[1] == 0 and K[3] == 0 and K[6] == 0 and K[7] == 0 and K[8] == 1
    z, one = f32(0.0), f32(1.0)
    Ki = np.array([one / K[0], z, -K[2] / K[0], z, one / K[4], -K[5] / K[4], z, z, one], f32)
    Ki[Ki == 0] = z                                                    # (-0 -> +0 like the library)
    M = np.empty(9, f32)
    for i in range(3):
        for j in range(3):
            M[3 * i + j] = fma(R[6 + i], Ki[6 + j], fma(R[3 + i], Ki[3 + j], R[i] * Ki[j]))
    return M


def direction(cam, xan, yan, w_match: int, h_match: int) -> np.ndarray:
    """(n, 3) f32 world directions of the normalised A-coordinates (n,) f32."""
    M = dir_matrix(cam)
    sx, sy = support_ref.pixel_scale(cam.width, w_match), support_ref.pixel_scale(cam.height, h_match)
    ua = colour_ref.match_px(xan, w_match - 1) * sx
    va = colour_ref.match_px(yan, h_match - 1) * sy
    return np.stack([fma(M[3 * i + 1], va, fma(M[3 * i], ua, M[3 * i + 2])) for i in range(3)], axis=-1).astype(f32)


def agree(P, sx, sy, d, xb, yb, w_match, h_match, tau):
    P = np.asarray(P, f32).reshape(3, 4)
    ub = colour_ref.match_px(xb, w_match - 1) * f32(sx)
    vb = colour_ref.match_px(yb, h_match - 1) * f32(sy)
    row = lambda i: fma(f32(0.0), P[i, 3], fma(d[:, 2], P[i, 2], fma(d[:, 1], P[i, 1], d[:, 0] * P[i, 0])))
    px, py, pz = row(0), row(1), row(2)
    du, dv = px - ub * pz, py - vb * pz
    d2 = du * du + dv * dv
    t = f32(tau) * pz
    return (pz > 0) & (d2 <= t * t)


def keys(d, S: int):
    """d (n, 3) f32 -> (valid (n,) bool, key (n,) i64, q (n, 3) i64); rows that are not valid hold key -1, q 0."""
    d = np.asarray(d, f32)
    n = d.shape[0]
    valid = np.isfinite(d).all(axis=1)
    dd = np.where(valid[:, None], d, f32(1.0)).astype(np.float64)
    a = np.abs(dd)
    m = np.zeros(n, np.int64)
    m = np.where(a[:, 1] > a[np.arange(n), m], 1, m)
    m = np.where(a[:, 2] > a[np.arange(n), m], 2, m)
    am = a[np.arange(n), m]
    valid &= am > 0
    am = np.where(valid, am, 1.0)
    ia, ib = np.where(m == 0, 1, 0), np.where(m == 2, 1, 2)
    u, v = dd[np.arange(n), ia] / am, dd[np.arange(n), ib] / am
    iu = np.clip(np.floor(((u + 1.0) * 0.5) * float(S)).astype(np.int64), 0, S - 1)
    iv = np.clip(np.floor(((v + 1.0) * 0.5) * float(S)).astype(np.int64), 0, S - 1)
    face = 2 * m + (dd[np.arange(n), m] < 0)
    key = (face * S + iv) * S + iu
    nrm = np.sqrt((dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2])
    nrm = np.where(valid, nrm, 1.0)
    q = np.rint((dd / nrm[:, None]) * 1073741824.0).astype(np.int64)
    return valid, np.where(valid, key, -1), np.where(valid[:, None], q, 0)


def quantise_u8(c):
    with np.errstate(invalid="ignore"):
        v = np.rint(np.asarray(c, f32) * f32(255.0))
        return np.where(np.isnan(v), 0, np.clip(v, 0, 255)).astype(np.int64)


def cells(cams, ri, w_match: int, h_match: int, tau, far_certainty, far_min_views: int, S: int) -> dict:
    """One reference (a ReferenceInputs of CPU tensors).  dict of (H W,) arrays: ``d`` (n, 3) f32, ``conf`` / ``agree`` (n, k) bool (agree only
    where confident), ``n_conf``, ``far``, ``key``, ``q`` (n, 3), ``rgb`` (n, 3) i64 (0 where not far)."""
    k = len(ri.nbr_cams)
    H, W = tuple(ri.cert[0].shape)
    n = H * W
    cam = cams[int(ri.ref_cam)]
    warp = [np.asarray(w.numpy(), f32).reshape(n, -1) for w in ri.warp]
    C = warp[0].shape[1]
    yy, xx = np.divmod(np.arange(n), W)
    if C == 4:
        xan, yan = warp[0][:, 0], warp[0][:, 1]
    else:
        xan, yan = axis(W)[xx], axis(H)[yy]
    with np.errstate(all="ignore"):
        d = direction(cam, xan, yan, w_match, h_match)
        conf, agr = np.zeros((n, k), bool), np.zeros((n, k), bool)
        for j in range(k):
            nb = cams[int(ri.nbr_cams[j])]
            xb, yb = warp[j][:, -2], warp[j][:, -1]
            c = np.asarray(ri.cert[j].numpy(), f32).reshape(n) >= f32(far_certainty)
            c &= (support_ref.grid_nearest(xb, W) >= 0) & (support_ref.grid_nearest(yb, H) >= 0)
            if ri.mask_b is not None and ri.mask_b[j] is not None:
                c &= support_ref.mask_lookup(ri.mask_b[j].numpy(), xb, yb, H, W, w_match, h_match)
            conf[:, j] = c
            agr[:, j] = c & agree(nb.P, support_ref.pixel_scale(nb.width, w_match), support_ref.pixel_scale(nb.height, h_match), d, xb, yb,
                                  w_match, h_match, tau)
        ok = np.ones(n, bool)
        if ri.mask_a is not None:
            sx, sy = f32(w_match) / f32(W), f32(h_match) / f32(H)
            ok = ri.mask_a.numpy()[support_ref.nearest_src(yy, sy, h_match), support_ref.nearest_src(xx, sx, w_match)] != 0
        n_conf, n_agree = conf.sum(axis=1), agr.sum(axis=1)
        valid, key, q = keys(d, S)
        far = ok & (n_conf >= min(int(far_min_views), k)) & (n_agree == n_conf) & valid
        rgb = np.zeros((n, 3), np.int64)
        idx = np.nonzero(far)[0]
        if idx.size:
            col = colour_ref.bilinear(ri.image.numpy(), colour_ref.match_px(xan[idx], w_match - 1), colour_ref.match_px(yan[idx], h_match - 1))
            rgb[idx] = quantise_u8(col)
    return dict(d=d, conf=conf, agree=agr, n_conf=n_conf, far=far, key=np.where(far, key, -1), q=np.where(far[:, None], q, 0), rgb=rgb,
                shape=(H, W))


def accumulate(cams, refs, w_match: int, h_match: int, tau, far_certainty, far_min_views: int, S: int):
    """Every reference of a batch.  Returns (table (6 S S, 7) uint64, counters (n_refs,) int64, [cells(...) per reference])."""
    table = np.zeros((6 * S * S, QUANTITIES), np.int64)
    counters = np.zeros(len(refs), np.int64)
    per = []
    for r, ri in enumerate(refs):
        c = cells(cams, ri, w_match, h_match, tau, far_certainty, far_min_views, S)
        idx = np.nonzero(c["far"])[0]
        for e in range(3):
            np.add.at(table[:, e], c["key"][idx], c["q"][idx, e])
            np.add.at(table[:, 3 + e], c["key"][idx], c["rgb"][idx, e])
        np.add.at(table[:, 6], c["key"][idx], 1)
        counters[r] = idx.size
        per.append(c)
    return table.view(np.uint64), counters, per


def emit(table, S: int, min_samples: int, centre, radius: float):
    """table (6 S S, 7) uint64 -> (keys (m,) i64, xyz, rgb, normal (m, 3) f32, samples (m,) i32), in key order."""
    t = np.asarray(table).view(np.int64)
    s = t[:, :3]
    keep = (t[:, 6] >= int(min_samples)) & (s != 0).any(axis=1)
    idx = np.nonzero(keep)[0]
    sd = s[idx].astype(np.float64)
    nrm = np.sqrt((sd[:, 0] * sd[:, 0] + sd[:, 1] * sd[:, 1]) + sd[:, 2] * sd[:, 2])
    h = sd / nrm[:, None]
    cnt = t[idx, 6].astype(np.float64)
    xyz = (np.asarray(centre, np.float64).reshape(1, 3) + float(radius) * h).astype(f32)
    rgb = (t[idx, 3:6].astype(np.float64) / (255.0 * cnt)[:, None]).astype(f32)
    return idx, xyz, rgb, (-h).astype(f32), np.minimum(t[idx, 6], 2 ** 31 - 1).astype(np.int32)


def cell_directions(key, S: int, n: int = 4) -> np.ndarray:
    """(len(key), n * n, 3) f64: an n x n lattice of directions inside each direction cell (the inverse of ``keys``' cube map)."""
    key = np.asarray(key, np.int64)
    face, rest = np.divmod(key, S * S)
    iv, iu = np.divmod(rest, S)
    m, neg = face // 2, face % 2
    t = (np.arange(n) + 0.5) / n
    uu = ((iu[:, None, None] + t[None, None, :]) / S) * 2.0 - 1.0
    vv = ((iv[:, None, None] + t[None, :, None]) / S) * 2.0 - 1.0
    uu, vv = np.broadcast_arrays(uu, vv)
    out = np.empty(key.shape + (n, n, 3))
    rows = np.arange(key.size)
    ia, ib = np.where(m == 0, 1, 0), np.where(m == 2, 1, 2)
    out[rows, :, :, m] = np.where(neg == 1, -1.0, 1.0)[:, None, None]
    out[rows, :, :, ia] = uu
    out[rows, :, :, ib] = vv
    return out.reshape(key.size, n * n, 3)
