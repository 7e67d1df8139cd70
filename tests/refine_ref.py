"""The yardstick of the multi-view re-triangulation's tests (lfd_refine_multiview): the same candidates, the same f32 rows, M and its
smallest eigenvector in f64 through numpy.linalg.eigh, the same acceptance - and, per point, the margin of every test to its threshold.

    candidates   every other neighbour that is live and agrees with the two-view point within tau (tests/support_ref.py, evaluated in f64)
    rows         u p2 - p0, v p2 - p1 per view with f32 entries, formed operation by operation as the library forms them (pixel conversion, multiply,
                 subtract: NumPy's f32 operations are the same IEEE operations); views: reference, winning slot, candidates
    X'           eigenvector of the smallest eigenvalue of M = sum row row^T (f64), divided by its last component, rounded to f32
    accepted     X' finite; in the reference and in the winning view depth > 0 and reprojection error <= reproj_thresh; every candidate agrees with
                 X' within tau.  err' = the larger of the two reprojection errors.

A point is IN BAND when any acceptance test - the two reprojection tests and the candidate tests at X' - comes closer to its threshold than
BAND_PX = 1e-3 px (the project's ERR_ATOL), when support_ref's own derived rounding bound says a candidate test at X or X' may go either way, or when
a depth is within rounding of 0.  Outside the band an implementation must report the reference's status; inside it may take either decision.
"""
from __future__ import annotations

import numpy as np

import support_ref

f32 = np.float32
BAND_PX = 1e-3
ACCEPTED = 0x80


def identity_axis(n: int) -> np.ndarray:
    """torch.linspace(-1 + 1/n, 1 - 1/n, n) in f32 as the library computes it (lfd_make_axis / lfd_axis_value)."""
    start, end = f32(-1.0 + 1.0 / n), f32(1.0 - 1.0 / n)
    step = (end - start) / f32(n - 1) if n > 1 else f32(0.0)
    j = np.arange(n)
    lo = start + step * j.astype(f32)
    hi = end - step * (n - 1 - j).astype(f32)
    return np.where(j < n // 2, lo, hi).astype(f32) if n > 1 else np.array([start], f32)


def match_px(nrm, size_m1: int, scale) -> np.ndarray:
    """lfd_match_px times the pair's pixel scale, f32 operation by operation."""
    nrm = np.asarray(nrm, f32)
    with np.errstate(all="ignore"):
        return (((nrm + f32(1.0)) * f32(0.5)) * f32(size_m1)) * f32(scale)


def rows_f32(P, u, v) -> np.ndarray:
    """(n, 2, 4) f32: u p2 - p0 and v p2 - p1, multiply then subtract."""
    P = np.asarray(P, f32).reshape(3, 4)
    with np.errstate(all="ignore"):
        ru = u[:, None].astype(f32) * P[2][None, :] - P[0][None, :]
        rv = v[:, None].astype(f32) * P[2][None, :] - P[1][None, :]
    return np.stack([ru, rv], axis=1).astype(f32)


def smallest_eigenvector(M: np.ndarray) -> np.ndarray:
    """(n, 4) f64 of (n, 4, 4) symmetric matrices; rows with a non-finite entry give NaN."""
    ok = np.isfinite(M).all(axis=(1, 2))
    out = np.full((M.shape[0], 4), np.nan)
    if ok.any():
        _w, v = np.linalg.eigh(M[ok])
        out[ok] = v[:, :, 0]
    return out


def observations(ref_cam, nbr_cams, warp, H, W, cell, axes=None):
    """Normalised observations of the cells: the reference's per slot (n, k, 2) - channels 0, 1 of that slot's warp, or the A-grid axes - and every
    neighbour's own (n, k, 2)."""
    k = len(nbr_cams)
    n = cell.size
    ax, ay = (np.asarray(axes[0], f32), np.asarray(axes[1], f32)) if axes is not None else (identity_axis(W), identity_axis(H))
    a, b = np.zeros((n, k, 2), f32), np.zeros((n, k, 2), f32)
    for j in range(k):
        wj = np.asarray(warp[j], f32).reshape(H * W, -1)[cell]
        b[:, j] = wj[:, -2:]
        if wj.shape[1] == 4:
            a[:, j] = wj[:, :2]
        else:
            a[:, j, 0], a[:, j, 1] = ax[cell % W], ay[cell // W]
    return a, b


def reference(cams, ref_cam: int, nbr_cams, cert, warp, masks_b, w_match: int, h_match: int, cell, slot, xyz, err, tau: float, reproj_thresh: float,
              axes=None):
    """One reference's points.  Arguments as tests/support_ref.py::reference, plus the points' ``err`` and the two thresholds.  dict of (n,) arrays:
    ``n_extra``, ``accepted``, ``status`` (n_extra | 0x80), ``xyz`` (n, 3) f32 and ``err`` f32 as emitted, ``band`` (some test within BAND_PX or
    within rounding of its threshold), ``margin`` f64 (the smallest distance of a test to its threshold, inf where nothing was tested)."""
    k = len(nbr_cams)
    cell, slot = np.asarray(cell).astype(np.int64), np.asarray(slot).astype(np.int64)
    xyz, err = np.asarray(xyz, f32).reshape(-1, 3), np.asarray(err, f32).reshape(-1)
    n = cell.size
    H, W = np.asarray(cert[0]).shape
    inside = (cell >= 0) & (cell < H * W) & (slot < k)
    cell_s, slot_s = np.where(inside, cell, 0), np.where(inside, slot, 0)
    sup = support_ref.reference(cams, ref_cam, nbr_cams, cert, warp, masks_b, w_match, h_match, cell_s, slot_s, xyz, tau)
    counted = sup["tested"] & sup["live"] & inside[:, None]
    cand = counted & sup["agree"]
    margin = np.where(counted, np.abs(sup["e"] - tau), np.inf)
    margin = np.where(np.isnan(margin), np.inf, margin).min(axis=1, initial=np.inf)
    band = (counted & sup["band"]).any(axis=1)         # who is a candidate: support_ref's own derived rounding bound
    n_extra = cand.sum(axis=1)

    obs_a, obs_b = observations(ref_cam, nbr_cams, warp, H, W, cell_s, axes)
    rc = cams[int(ref_cam)]
    idx = np.arange(n)
    ua = match_px(obs_a[idx, slot_s, 0], w_match - 1, support_ref.pixel_scale(rc.width, w_match))
    va = match_px(obs_a[idx, slot_s, 1], h_match - 1, support_ref.pixel_scale(rc.height, h_match))
    M = np.einsum("nri,nrj->nij", *(2 * [rows_f32(rc.P, ua, va).astype(np.float64)]))
    P_win = np.zeros((n, 3, 4), f32)
    ub, vb = np.zeros(n, f32), np.zeros(n, f32)
    for j in range(k):
        cam = cams[int(nbr_cams[j])]
        uj = match_px(obs_b[:, j, 0], w_match - 1, support_ref.pixel_scale(cam.width, w_match))
        vj = match_px(obs_b[:, j, 1], h_match - 1, support_ref.pixel_scale(cam.height, h_match))
        rows = rows_f32(cam.P, uj, vj).astype(np.float64)
        use = (cand[:, j] | (slot_s == j)).astype(np.float64)
        with np.errstate(invalid="ignore"):
            M += np.where(use[:, None, None] > 0, np.einsum("nri,nrj->nij", rows, rows), 0.0)
        win = slot_s == j
        P_win[win] = np.asarray(cam.P, f32).reshape(3, 4)
        ub[win], vb[win] = uj[win], vj[win]
    c = smallest_eigenvector(M)
    with np.errstate(all="ignore"):
        Xn = (c[:, :3] / c[:, 3:4]).astype(f32)
    finite = np.isfinite(Xn).all(axis=1)
    Xs = np.where(finite[:, None], Xn, f32(0.0))

    def reproj(P, u, v):
        """f64 reprojection error and depth of the f32 point in one view per point (P (n, 3, 4) or (3, 4))."""
        P = np.broadcast_to(np.asarray(P, f32).astype(np.float64), (n, 3, 4))
        p = np.einsum("nij,nj->ni", P[:, :, :3], Xs.astype(np.float64)) + P[:, :, 3]
        with np.errstate(all="ignore"):
            e = np.hypot(p[:, 0] / p[:, 2] - u.astype(np.float64), p[:, 1] / p[:, 2] - v.astype(np.float64))
        return e, p[:, 2]

    e_a, z_a = reproj(np.asarray(rc.P, f32).reshape(3, 4), ua, va)
    e_b, z_b = reproj(P_win, ub, vb)
    with np.errstate(invalid="ignore"):
        e_two = np.where(np.isnan(e_a) | np.isnan(e_b), np.nan, np.maximum(e_a, e_b))
        ok = finite & (z_a > 0) & (z_b > 0) & (e_two <= reproj_thresh)
        m_new = np.abs(e_two - reproj_thresh)
        depth_band = (np.abs(z_a) < 1e-6) | (np.abs(z_b) < 1e-6)
    for j in range(k):
        cam = cams[int(nbr_cams[j])]
        t = support_ref.pair_test(np.asarray(cam.P, f32), support_ref.pixel_scale(cam.width, w_match), support_ref.pixel_scale(cam.height, h_match),
                                  Xs, obs_b[:, j, 0], obs_b[:, j, 1], w_match, h_match, tau)
        ok &= ~cand[:, j] | t["agree"]
        with np.errstate(invalid="ignore"):
            mj = np.where(cand[:, j], np.abs(t["e"] - tau), np.inf)
        m_new = np.fmin(m_new, mj)
        depth_band |= cand[:, j] & t["band"]
    has = n_extra > 0
    accepted = has & ok
    m_new = np.where(has & finite, m_new, np.inf)
    with np.errstate(invalid="ignore"):
        band |= has & finite & ((m_new < BAND_PX) | depth_band)
    margin = np.fmin(margin, m_new)
    out_xyz = np.where(accepted[:, None], Xn, xyz).astype(f32)
    out_err = np.where(accepted, e_two.astype(f32), err).astype(f32)
    return dict(n_extra=n_extra, accepted=accepted, status=(n_extra | np.where(accepted, ACCEPTED, 0)).astype(np.uint8), xyz=out_xyz, err=out_err,
                band=band, margin=margin, cand=cand)


def two_view_f64(cams, ref_cam: int, nbr_cams, warp, w_match: int, h_match: int, cell, slot, axes=None) -> np.ndarray:
    """(n, 3) f64: every (cell, slot) triangulated from its two views entirely in f64 (pixel conversion, rows, eigh).  On a noise-free field
    this is the truth the accuracy tests measure against."""
    cell, slot = np.asarray(cell).astype(np.int64), np.asarray(slot).astype(np.int64)
    H, W = np.asarray(warp[0]).shape[:2]
    obs_a, obs_b = observations(ref_cam, nbr_cams, warp, H, W, cell, axes)
    n = cell.size
    idx = np.arange(n)
    rc = cams[int(ref_cam)]

    def px(nrm, size, cam_size):
        return (nrm.astype(np.float64) + 1.0) * 0.5 * (size - 1) * (float(cam_size) / float(size))

    def rows(P, u, v):
        P = np.broadcast_to(np.asarray(P, np.float64), (n, 3, 4))
        return np.stack([u[:, None] * P[:, 2] - P[:, 0], v[:, None] * P[:, 2] - P[:, 1]], axis=1)

    Pb = np.stack([np.asarray(cams[int(nbr_cams[j])].P, np.float64).reshape(3, 4) for j in slot])
    wb = np.array([cams[int(nbr_cams[j])].width for j in slot]), np.array([cams[int(nbr_cams[j])].height for j in slot])
    ra = rows(np.asarray(rc.P, np.float64).reshape(3, 4), px(obs_a[idx, slot, 0], w_match, rc.width), px(obs_a[idx, slot, 1], h_match, rc.height))
    ub = (obs_b[idx, slot, 0].astype(np.float64) + 1.0) * 0.5 * (w_match - 1) * (wb[0] / float(w_match))
    vb = (obs_b[idx, slot, 1].astype(np.float64) + 1.0) * 0.5 * (h_match - 1) * (wb[1] / float(h_match))
    rb = rows(Pb, ub, vb)
    A = np.concatenate([ra, rb], axis=1)
    c = smallest_eigenvector(np.einsum("nri,nrj->nij", A, A))
    return c[:, :3] / c[:, 3:4]


def over_references(cams, refs, src, tau: float, reproj_thresh: float, w_match: int, h_match: int) -> dict:
    """``reference`` over every reference of a collected result ``src`` made for the ReferenceInputs ``refs`` (tensors anywhere), concatenated in
    the result's order."""
    host = lambda t: t.cpu().numpy()
    off = np.asarray(src.ref_offsets)
    cell, slot, xyz, err = host(src.cell), host(src.slot), host(src.xyz), host(src.err)
    parts = []
    for r, ri in enumerate(refs):
        a, b = int(off[r]), int(off[r + 1])
        masks = [host(m) if m is not None else None for m in ri.mask_b] if ri.mask_b is not None else None
        parts.append(reference(cams, ri.ref_cam, ri.nbr_cams, [host(c) for c in ri.cert], [host(w) for w in ri.warp], masks, w_match, h_match,
                               cell[a:b], slot[a:b], xyz[a:b], err[a:b], tau, reproj_thresh))
    return {name: np.concatenate([p[name] for p in parts]) for name in ("n_extra", "accepted", "status", "xyz", "err", "band", "margin")}


def bits(a) -> np.ndarray:
    a = np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def check_against_reference(ref: dict, src, xyz, err, status, reproj_thresh: float, band_cap: float, xyz_rtol=1e-5, xyz_atol=1e-6, err_atol=1e-3):
    """One implementation's output (``xyz``, ``err``, ``status`` for the input points ``src``) against ``over_references``' result: the share of
    points with a candidate that are in band stays under the cap; outside the band the status is the reference's and a refined point agrees
    within the project's tolerances; whatever the band says, a point that was not accepted is its input bit for bit and every accepted point
    passes the two-view threshold.  Returns (points with a candidate, of them in band, accepted, fallen back)."""
    st = np.asarray(status.cpu().numpy() if hasattr(status, "cpu") else status)
    got_xyz, got_err = np.asarray(xyz.cpu().numpy() if hasattr(xyz, "cpu") else xyz), np.asarray(err.cpu().numpy() if hasattr(err, "cpu") else err)
    has = ref["n_extra"] > 0
    in_band = ref["band"]
    n_has, n_band = int(has.sum()), int((has & in_band).sum())
    assert n_band <= band_cap * max(n_has, 1), (n_band, n_has)
    clean = ~in_band
    assert np.array_equal(st[clean], ref["status"][clean]), np.flatnonzero(clean & (st != ref["status"]))[:10]
    acc = (st & ACCEPTED) != 0
    assert np.array_equal(bits(got_xyz)[~acc], bits(src.xyz)[~acc]) and np.array_equal(bits(got_err)[~acc], bits(src.err)[~acc])
    assert not acc[(st & 0x7f) == 0].any()
    assert (got_err[acc] <= np.float32(reproj_thresh)).all() and np.isfinite(got_xyz[acc]).all()
    both = clean & acc
    np.testing.assert_allclose(got_xyz[both], ref["xyz"][both], rtol=xyz_rtol, atol=xyz_atol)
    np.testing.assert_allclose(got_err[both], ref["err"][both], rtol=0, atol=err_atol)
    return n_has, n_band, int(acc.sum()), int((((st & 0x7f) > 0) & ~acc).sum())
