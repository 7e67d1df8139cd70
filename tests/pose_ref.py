"""The yardstick of the pose refinement's tests (lfd_pose_accumulate): a NumPy evaluation of the rule as the header states it,
one NumPy operation per rounding, so that the integer table can be compared with the library element for element - and an UN-QUANTISED f64
Gauss-Newton step from the same matches (its own assembly and solve, a projector and a pseudo-inverse instead of core/poses.py's QR and
eigen-decomposition), the yardstick of the effect test.

Per pair (A, B), from the records' f32 values in f64:  R = R_B R_A^T,  t = t_B - R t_A,  tn = |t|,  th = t / tn,  K^-1 closed form (f32).
Per confident match:  yA = K_A^-1 (ua, va, 1), p = R yA, n = th x p, l = K_B^-T n, num = (ub l0 + vb l1) + l2, d2 = l0 l0 + l1 l1, d = sqrt(d2),
r = num / d; foot (ub - (r l0) / d, vb - (r l1) / d), yB = K_B^-1 (foot, 1); J = ((n x yB) / d, (p x yB) / d); degenerate / outlier / inlier;
Jq = rint(8 J), rq = rint(1024 r).
"""
from __future__ import annotations

import numpy as np

import audit_ref
import colour_ref
import support_ref

f32, f64 = np.float32, np.float64
QUANTITIES = 32
INLIER, OUTLIER, DEGENERATE = 0, 1, 2


def inv_k(K) -> np.ndarray:
    """(9,) f64 of the f32 closed-form inverse of a plain intrinsic matrix (what the library's own F uses)."""
    K = np.asarray(K, f32).reshape(3, 3)
    assert K[0, 1] == 0 and K[1, 0] == 0 and K[2, 0] == 0 and K[2, 1] == 0 and K[2, 2] == 1
    Ki = np.array([f32(1.0) / K[0, 0], f32(0), -K[0, 2] / K[0, 0], f32(0), f32(1.0) / K[1, 1], -K[1, 2] / K[1, 1], f32(0), f32(0), f32(1)], f32)
    return (Ki + f32(0.0)).astype(f64)                                 # (-0 -> +0)


def pair_const(a, b, dtype=f32) -> dict:
    """The pair's constants from the records' values as ``dtype`` holds them (f32: what the library was given; f64: for the derivative test)."""
    RA, RB = np.asarray(a.R, dtype).astype(f64).reshape(3, 3), np.asarray(b.R, dtype).astype(f64).reshape(3, 3)
    tA, tB = np.asarray(a.t, dtype).astype(f64).reshape(3), np.asarray(b.t, dtype).astype(f64).reshape(3)
    R = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            R[i, j] = (RB[i, 0] * RA[j, 0] + RB[i, 1] * RA[j, 1]) + RB[i, 2] * RA[j, 2]
    t = np.array([tB[i] - ((R[i, 0] * tA[0] + R[i, 1] * tA[1]) + R[i, 2] * tA[2]) for i in range(3)])
    tn = np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
    ok = bool(np.isfinite(tn) and tn > 0.0)
    return dict(KAi=inv_k(a.K), KBi=inv_k(b.K), R=R, th=t / tn if ok else np.zeros(3), tn=float(tn) if ok else 0.0, ok=ok, t=t)


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def samples(pc: dict, ua, va, ub, vb, inlier_px):
    """f32 camera-px coordinates (n,) -> dict(kind (n,), q (n, 7) i64 - zero unless an inlier -, r (n,), J (n, 6)): un-quantised r and J too."""
    ua, va, ub, vb = (np.asarray(a, f32).astype(f64) for a in (ua, va, ub, vb))
    KA, KB, R, th = pc["KAi"], pc["KBi"], pc["R"], pc["th"]
    c = f64(f32(inlier_px))
    with np.errstate(all="ignore"):
        yA = [(KA[3 * i] * ua + KA[3 * i + 1] * va) + KA[3 * i + 2] for i in range(3)]
        p = [(R[i, 0] * yA[0] + R[i, 1] * yA[1]) + R[i, 2] * yA[2] for i in range(3)]
        n = cross(th, p)
        l = [(KB[i] * n[0] + KB[3 + i] * n[1]) + KB[6 + i] * n[2] for i in range(3)]
        num = (ub * l[0] + vb * l[1]) + l[2]
        d2 = l[0] * l[0] + l[1] * l[1]
        num2 = num * num
        first = np.isfinite(num) & np.isfinite(d2) & np.isfinite(num2) & (d2 > 0) & pc["ok"]
        d = np.sqrt(d2)
        r = num / d
        uf, vf = ub - (r * l[0]) / d, vb - (r * l[1]) / d
        yB = [(KB[3 * i] * uf + KB[3 * i + 1] * vf) + KB[3 * i + 2] for i in range(3)]
        J = np.stack([v / d for v in cross(n, yB) + cross(p, yB)], axis=1)
        fine = first & np.isfinite(r) & np.isfinite(uf) & np.isfinite(vf) & (np.abs(J) < 65536.0).all(axis=1)
        outlier = fine & (num2 >= (c * c) * d2)
        inlier = fine & ~outlier
        kind = np.where(inlier, INLIER, np.where(outlier, OUTLIER, DEGENERATE))
        q = np.zeros((len(ua), 7), np.int64)
        q[inlier, :6] = np.rint(8.0 * J[inlier]).astype(np.int64)
        q[inlier, 6] = np.rint(1024.0 * r[inlier]).astype(np.int64)
    return dict(kind=kind, q=q, r=r, J=J)


def row_of(q: np.ndarray) -> np.ndarray:
    """The 28 signed sums (columns 3 .. 30) of the inliers' (n, 7) integers, as Python-exact int64."""
    out = [int((q[:, 6] * q[:, 6]).sum())] + [int((q[:, i] * q[:, 6]).sum()) for i in range(6)]
    out += [int((q[:, i] * q[:, j]).sum()) for i in range(6) for j in range(i, 6)]
    return np.asarray(out, np.int64)


def cells(cams, ri, w_match: int, h_match: int, certainty, inlier_px) -> list:
    """One reference (a ReferenceInputs of CPU tensors): per slot dict(conf (H W,), kind, q, r, J) - the confidence test is the audit's."""
    conf = audit_ref.cells(cams, ri, w_match, h_match, certainty)["conf"]
    H, W = tuple(ri.cert[0].shape)
    n = H * W
    cam = cams[int(ri.ref_cam)]
    warp = [np.asarray(w.numpy(), f32).reshape(n, -1) for w in ri.warp]
    yy, xx = np.divmod(np.arange(n), W)
    if warp[0].shape[1] == 4:
        xan, yan = warp[0][:, 0], warp[0][:, 1]
    else:
        xan, yan = audit_ref.far_ref.axis(W)[xx], audit_ref.far_ref.axis(H)[yy]
    out = []
    with np.errstate(all="ignore"):
        ua = colour_ref.match_px(xan, w_match - 1) * support_ref.pixel_scale(cam.width, w_match)
        va = colour_ref.match_px(yan, h_match - 1) * support_ref.pixel_scale(cam.height, h_match)
        for j, nbr in enumerate(ri.nbr_cams):
            nb = cams[int(nbr)]
            ub = colour_ref.match_px(warp[j][:, -2], w_match - 1) * support_ref.pixel_scale(nb.width, w_match)
            vb = colour_ref.match_px(warp[j][:, -1], h_match - 1) * support_ref.pixel_scale(nb.height, h_match)
            s = samples(pair_const(cam, nb), ua, va, ub, vb, inlier_px)
            out.append(dict(conf=conf[:, j], **s))
    return out


def table(cams, refs, k: int, w_match: int, h_match: int, certainty, inlier_px):
    """Every reference of a batch of ``k`` slots.  Returns (table (n_refs k, 32) int64, [cells(...) per reference])."""
    tab = np.zeros((len(refs) * k, QUANTITIES), np.int64)
    per = []
    for r, ri in enumerate(refs):
        cs = cells(cams, ri, w_match, h_match, certainty, inlier_px)
        for j, c in enumerate(cs):
            row = tab[r * k + j]
            for kind in (INLIER, OUTLIER, DEGENERATE):
                row[kind] = int((c["conf"] & (c["kind"] == kind)).sum())
            row[3:31] = row_of(c["q"][c["conf"] & (c["kind"] == INLIER)])
        per.append(cs)
    return tab, per


# ---- the un-quantised step ---------------------------------------------------------------------------------------------------------------------
def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def expm_so3(w):
    th = float(np.linalg.norm(w))
    K = skew(w)
    return np.eye(3) + K if th < 1e-12 else np.eye(3) + np.sin(th) / th * K + (1.0 - np.cos(th)) / th ** 2 * (K @ K)


def pose64(rec):
    return np.asarray(rec.R, f32).astype(f64).reshape(3, 3), np.asarray(rec.t, f32).astype(f64).reshape(3)


def gn_step(cams, refs, w_match: int, h_match: int, certainty=0.5, inlier_px=8.0, min_samples=256, eig_cut=1e-9) -> dict:
    """One un-quantised f64 Gauss-Newton step on the epipolar error of ``refs``' matches against the records ``cams``.  Returns dict(poses
    {camera index: (R, t)} of the cameras in the system, eig_min_rel (the reduced matrix's smallest eigenvalue over its largest), median
    {(a, b): median |r| in px}, step_deg {camera index: rotation step})."""
    pairs, median = [], {}
    for ri in refs:
        for j, c in enumerate(cells(cams, ri, w_match, h_match, certainty, inlier_px)):
            a, b = int(ri.ref_cam), int(ri.nbr_cams[j])
            live = c["conf"] & (c["kind"] != DEGENERATE)
            if live.any():
                median[(a, b)] = float(np.median(np.abs(c["r"][live])))
            m = c["conf"] & (c["kind"] == INLIER)
            if int(m.sum()) >= min_samples:
                pairs.append((a, b, c["J"][m], c["r"][m]))
    idx = sorted({u for a, b, _J, _r in pairs for u in (a, b)})
    at = {u: i for i, u in enumerate(idx)}
    N = len(idx)
    H, g = np.zeros((6 * N, 6 * N)), np.zeros(6 * N)
    for a, b, J, r in pairs:
        pc = pair_const(cams[a], cams[b])
        Js = J.copy()
        Js[:, 3:] /= pc["tn"]
        Ad = np.zeros((6, 6))
        Ad[:3, :3] = pc["R"]
        Ad[3:, :3] = skew(pc["t"]) @ pc["R"]
        Ad[3:, 3:] = pc["R"]
        full = np.zeros((len(r), 6 * N))
        full[:, 6 * at[a]:6 * at[a] + 6] = -Js @ Ad
        full[:, 6 * at[b]:6 * at[b] + 6] += Js
        H += full.T @ full
        g += full.T @ r
    G = np.zeros((6 * N, 7))
    for u in idx:
        R, t = pose64(cams[u])
        i = 6 * at[u]
        for ax in range(3):
            om = -R[:, ax]
            G[i:i + 3, ax], G[i + 3:i + 6, ax], G[i + 3:i + 6, 3 + ax] = om, -np.cross(om, t), -R[:, ax]
        G[i + 3:i + 6, 6] = t
    P = np.eye(6 * N) - G @ np.linalg.pinv(G)
    Hp = P @ H @ P
    lam = np.linalg.eigvalsh(0.5 * (Hp + Hp.T))
    real = lam[7:]                                                     # (the seven projected directions are the zeros)
    delta = -np.linalg.pinv(0.5 * (Hp + Hp.T), rcond=eig_cut, hermitian=True) @ (P @ g)
    poses, step = {}, {}
    for u in idx:
        R, t = pose64(cams[u])
        d = delta[6 * at[u]:6 * at[u] + 6]
        E = expm_so3(d[:3])
        poses[u], step[u] = (E @ R, E @ t + d[3:]), float(np.degrees(np.linalg.norm(d[:3])))
    return dict(poses=poses, eig_min_rel=float(real[0] / lam[-1]), median=median, step_deg=step, delta=delta, index=idx)
