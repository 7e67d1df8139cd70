"""The yardstick of the precision-weighted re-triangulation's tests (lfd_refine_multiview_weighted): tests/refine_ref.py with the
weights of the contract, everything behind the f32 rows in f64.

    candidates   as tests/refine_ref.py (tests/support_ref.py, evaluated in f64)
    rows         the same f32 rows
    valid(j)     the three plane values of view j at the cell finite, q00 > 0, q11 > 0, q00 q11 - q01 q01 > 0 in f64 (exact products of f32 values)
    weights      p = (q00 / sx^2, q01 / (sx sy), q11 / sy^2) with the pair's f32 pixel scales, w2 = 1 / pz^2 at the two-view X; per neighbour view
                 M += w2 (p00 ru ru^T + p01 (ru rv^T + rv ru^T) + p11 rv rv^T); the reference M += lamA w2_A (ru ru^T + rv rv^T),
                 lamA = sum over the participating neighbour views of (p00 + p11) / 2
    fallback     any participating view (winning slot, candidates) invalid: the unweighted M of tests/refine_ref.py
    X'           numpy.linalg.eigh, divided by its last component, rounded to f32; the same acceptance, the same margins, the same band

Status: n_extra | 0x40 (weighted rows used) | 0x80 (accepted).  The 0x40 bit has no band of its own: validity is decided exactly.
"""
from __future__ import annotations

import numpy as np

import refine_ref as rr
import support_ref

f32 = np.float32
BAND_PX = rr.BAND_PX
ACCEPTED = 0x80
WEIGHTED = 0x40


def plane_valid(q) -> np.ndarray:
    """(n,) bool of (n, 3) f32 plane values."""
    q = np.asarray(q, f32)
    q64 = q.astype(np.float64)
    with np.errstate(all="ignore"):
        det = q64[:, 0] * q64[:, 2] - q64[:, 1] * q64[:, 1]
        return np.isfinite(q).all(axis=1) & (q[:, 0] > 0) & (q[:, 2] > 0) & (det > 0)


def reference(cams, ref_cam: int, nbr_cams, cert, warp, masks_b, prec, w_match: int, h_match: int, cell, slot, xyz, err, tau: float,
              reproj_thresh: float, axes=None):
    """One reference's points; arguments as refine_ref.reference plus ``prec``: per slot an (H, W, 3) f32 plane.  dict of (n,) arrays as
    refine_ref.reference's, plus ``weighted`` (the weighted rows were used) - ``status`` carries it as 0x40."""
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
    band = (counted & sup["band"]).any(axis=1)
    n_extra = cand.sum(axis=1)

    obs_a, obs_b = rr.observations(ref_cam, nbr_cams, warp, H, W, cell_s, axes)
    rc = cams[int(ref_cam)]
    idx = np.arange(n)
    X64 = xyz.astype(np.float64)

    def depth(P):
        P = np.asarray(P, f32).astype(np.float64).reshape(3, 4)
        return X64 @ P[2, :3] + P[2, 3]

    ua = rr.match_px(obs_a[idx, slot_s, 0], w_match - 1, support_ref.pixel_scale(rc.width, w_match))
    va = rr.match_px(obs_a[idx, slot_s, 1], h_match - 1, support_ref.pixel_scale(rc.height, h_match))
    rows_a = rr.rows_f32(rc.P, ua, va).astype(np.float64)
    M_u = np.einsum("nri,nrj->nij", rows_a, rows_a)
    M_w = np.zeros((n, 4, 4))
    lam = np.zeros(n)
    all_valid = np.ones(n, bool)
    P_win = np.zeros((n, 3, 4), f32)
    ub, vb = np.zeros(n, f32), np.zeros(n, f32)
    for j in range(k):
        cam = cams[int(nbr_cams[j])]
        sx, sy = support_ref.pixel_scale(cam.width, w_match), support_ref.pixel_scale(cam.height, h_match)
        uj = rr.match_px(obs_b[:, j, 0], w_match - 1, sx)
        vj = rr.match_px(obs_b[:, j, 1], h_match - 1, sy)
        rows = rr.rows_f32(cam.P, uj, vj).astype(np.float64)
        use = cand[:, j] | (slot_s == j)
        q = np.asarray(prec[j], f32).reshape(H * W, 3)[cell_s]
        valid = plane_valid(q)
        all_valid &= ~use | valid
        q64 = np.where(valid[:, None], q.astype(np.float64), 0.0)
        sx64, sy64 = float(sx), float(sy)
        p00, p01, p11 = q64[:, 0] / (sx64 * sx64), q64[:, 1] / (sx64 * sy64), q64[:, 2] / (sy64 * sy64)
        with np.errstate(all="ignore"):
            w2 = 1.0 / depth(cam.P) ** 2
            ru, rv = rows[:, 0], rows[:, 1]
            outer = lambda a, b: a[:, :, None] * b[:, None, :]
            Mj = (w2 * p00)[:, None, None] * outer(ru, ru) + (w2 * p01)[:, None, None] * (outer(ru, rv) + outer(rv, ru)) \
                + (w2 * p11)[:, None, None] * outer(rv, rv)
            M_w += np.where(use[:, None, None], Mj, 0.0)
            lam += np.where(use, 0.5 * (p00 + p11), 0.0)
            M_u += np.where(use[:, None, None], np.einsum("nri,nrj->nij", rows, rows), 0.0)
        win = slot_s == j
        P_win[win] = np.asarray(cam.P, f32).reshape(3, 4)
        ub[win], vb[win] = uj[win], vj[win]
    with np.errstate(all="ignore"):
        wa = lam / depth(rc.P) ** 2
        M_w += wa[:, None, None] * np.einsum("nri,nrj->nij", rows_a, rows_a)
    has = n_extra > 0
    weighted = has & all_valid
    M = np.where(weighted[:, None, None], M_w, M_u)
    c = rr.smallest_eigenvector(M)
    with np.errstate(all="ignore"):
        Xn = (c[:, :3] / c[:, 3:4]).astype(f32)
    finite = np.isfinite(Xn).all(axis=1)
    Xs = np.where(finite[:, None], Xn, f32(0.0))

    def reproj(P, u, v):
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
    accepted = has & ok
    m_new = np.where(has & finite, m_new, np.inf)
    with np.errstate(invalid="ignore"):
        band |= has & finite & ((m_new < BAND_PX) | depth_band)
    margin = np.fmin(margin, m_new)
    out_xyz = np.where(accepted[:, None], Xn, xyz).astype(f32)
    out_err = np.where(accepted, e_two.astype(f32), err).astype(f32)
    status = (n_extra | np.where(weighted, WEIGHTED, 0) | np.where(accepted, ACCEPTED, 0)).astype(np.uint8)
    return dict(n_extra=n_extra, accepted=accepted, weighted=weighted, status=status, xyz=out_xyz, err=out_err, band=band, margin=margin, cand=cand)


def over_references(cams, refs, src, tau: float, reproj_thresh: float, w_match: int, h_match: int) -> dict:
    """``reference`` over every reference of a collected result ``src`` made for the ReferenceInputs ``refs`` (with precision planes)."""
    host = lambda t: t.cpu().numpy()
    off = np.asarray(src.ref_offsets)
    cell, slot, xyz, err = host(src.cell), host(src.slot), host(src.xyz), host(src.err)
    parts = []
    for r, ri in enumerate(refs):
        a, b = int(off[r]), int(off[r + 1])
        masks = [host(m) if m is not None else None for m in ri.mask_b] if ri.mask_b is not None else None
        parts.append(reference(cams, ri.ref_cam, ri.nbr_cams, [host(c) for c in ri.cert], [host(w) for w in ri.warp], masks,
                               [host(q) for q in ri.precision], w_match, h_match, cell[a:b], slot[a:b], xyz[a:b], err[a:b], tau, reproj_thresh))
    return {name: np.concatenate([p[name] for p in parts]) for name in ("n_extra", "accepted", "weighted", "status", "xyz", "err", "band", "margin")}


def check_against_reference(ref: dict, src, xyz, err, status, reproj_thresh: float, band_cap: float, xyz_rtol=1e-5, xyz_atol=1e-6, err_atol=1e-3):
    """refine_ref.check_against_reference for a status that carries 0x40: outside the band the whole status byte is the reference's; the
    candidates and the weights-used bit are the reference's EVERYWHERE they are decided exactly (0x40 always; the count outside the band).
    Returns (points with a candidate, in band, accepted, fallen back, solved with weights)."""
    st = np.asarray(status.cpu().numpy() if hasattr(status, "cpu") else status)
    got_xyz, got_err = np.asarray(xyz.cpu().numpy() if hasattr(xyz, "cpu") else xyz), np.asarray(err.cpu().numpy() if hasattr(err, "cpu") else err)
    has = ref["n_extra"] > 0
    in_band = ref["band"]
    n_has, n_band = int(has.sum()), int((has & in_band).sum())
    assert n_band <= band_cap * max(n_has, 1), (n_band, n_has)
    clean = ~in_band
    assert np.array_equal(st[clean], ref["status"][clean]), np.flatnonzero(clean & (st != ref["status"]))[:10]
    acc = (st & ACCEPTED) != 0
    assert np.array_equal(rr.bits(got_xyz)[~acc], rr.bits(src.xyz)[~acc]) and np.array_equal(rr.bits(got_err)[~acc], rr.bits(src.err)[~acc])
    assert not acc[(st & 0x3f) == 0].any() and not (st[(st & 0x3f) == 0] & WEIGHTED).any()
    assert (got_err[acc] <= np.float32(reproj_thresh)).all() and np.isfinite(got_xyz[acc]).all()
    both = clean & acc
    np.testing.assert_allclose(got_xyz[both], ref["xyz"][both], rtol=xyz_rtol, atol=xyz_atol)
    np.testing.assert_allclose(got_err[both], ref["err"][both], rtol=0, atol=err_atol)
    return n_has, n_band, int(acc.sum()), int((((st & 0x3f) > 0) & ~acc).sum()), int(((st & WEIGHTED) != 0).sum())
