"""The yardstick of the epipolar audit's tests (lfd_epipolar_audit): a NumPy evaluation of the rule as the header states it -
the coordinates in f32, the line and the distance in f64 with one NumPy operation per rounding, the bin as the plain count of thresholds
reached - so that tables and cell maps can be compared with the library element for element.

Per reference r, grid cell c (mask_a, if any, set) and slot j:

    confident raw certainty >= audit_certainty (NaN: no), observation inside the neighbour's grid, mask_b (if any) set where it points
    l         F (ua, va, 1): l_i = (F_3i ua + F_3i+1 va) + F_3i+2
    num, n2   (ub l0 + vb l1) + l2,  l0 l0 + l1 l1
    usable    num^2 and n2 finite, n2 > 0 (else degenerate)
    bin       #{b in 0 .. 62 : num^2 >= ((b + 1)^2 / 64) n2}
"""
from __future__ import annotations

import numpy as np

import colour_ref
import far_ref
import support_ref
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

f32 = np.float32
QUANTITIES = 66
NONE = 255
E2 = (np.arange(1, 64, dtype=np.float64) ** 2) / 64.0                  # exact


def pair_F(cams, ri, j) -> np.ndarray:
    """(9,) f64 of f32 values: the slot's own matrix when the reference carries one, else what PreparedBatch(cameras=...) hands the library."""
    if ri.fundamental is not None:
        return np.asarray(ri.fundamental[j], f32).reshape(9).astype(np.float64)
    a, b = cams[int(ri.ref_cam)], cams[int(ri.nbr_cams[j])]
    return np.asarray(hb.fundamental_from_world2cam(a.K, a.R, a.t, b.K, b.R, b.t), f32).reshape(9).astype(np.float64)


def bins(F, ua, va, ub, vb):
    """f32 camera-px coordinates (n,) -> (usable (n,) bool, bin (n,) i64; 0 where not usable)."""
    ua, va, ub, vb = (np.asarray(a, f32).astype(np.float64) for a in (ua, va, ub, vb))
    with np.errstate(all="ignore"):
        l0 = (F[0] * ua + F[1] * va) + F[2]
        l1 = (F[3] * ua + F[4] * va) + F[5]
        l2 = (F[6] * ua + F[7] * va) + F[8]
        num = (ub * l0 + vb * l1) + l2
        n2 = l0 * l0 + l1 * l1
        num2 = num * num
        usable = np.isfinite(num2) & np.isfinite(n2) & (n2 > 0)
        b = (num2[:, None] >= E2[None, :] * n2[:, None]).sum(axis=1)
    return usable, np.where(usable, b, 0)


def cells(cams, ri, w_match: int, h_match: int, audit_certainty) -> dict:
    """One reference (a ReferenceInputs of CPU tensors).  dict of (H W, k) arrays ``conf``, ``usable``, ``bin`` and (H W,) ``best``."""
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
        xan, yan = far_ref.axis(W)[xx], far_ref.axis(H)[yy]
    ok = np.ones(n, bool)
    if ri.mask_a is not None:
        sx, sy = f32(w_match) / f32(W), f32(h_match) / f32(H)
        ok = ri.mask_a.numpy()[support_ref.nearest_src(yy, sy, h_match), support_ref.nearest_src(xx, sx, w_match)] != 0
    conf, usable, bn = np.zeros((n, k), bool), np.zeros((n, k), bool), np.zeros((n, k), np.int64)
    with np.errstate(all="ignore"):
        ua = colour_ref.match_px(xan, w_match - 1) * support_ref.pixel_scale(cam.width, w_match)
        va = colour_ref.match_px(yan, h_match - 1) * support_ref.pixel_scale(cam.height, h_match)
        for j in range(k):
            nb = cams[int(ri.nbr_cams[j])]
            xb, yb = warp[j][:, -2], warp[j][:, -1]
            c = ok & (np.asarray(ri.cert[j].numpy(), f32).reshape(n) >= f32(audit_certainty))
            c &= (support_ref.grid_nearest(xb, W) >= 0) & (support_ref.grid_nearest(yb, H) >= 0)
            if ri.mask_b is not None and ri.mask_b[j] is not None:
                c &= support_ref.mask_lookup(ri.mask_b[j].numpy(), xb, yb, H, W, w_match, h_match)
            ub = colour_ref.match_px(xb, w_match - 1) * support_ref.pixel_scale(nb.width, w_match)
            vb = colour_ref.match_px(yb, h_match - 1) * support_ref.pixel_scale(nb.height, h_match)
            u, b = bins(pair_F(cams, ri, j), ua, va, ub, vb)
            conf[:, j], usable[:, j], bn[:, j] = c, c & u, b
    best = np.where(usable, bn, NONE).min(axis=1) if k else np.full(n, NONE)
    return dict(conf=conf, usable=usable, bin=bn, best=best.astype(np.uint8), shape=(H, W))


def audit(cams, refs, k: int, w_match: int, h_match: int, audit_certainty):
    """Every reference of a batch of ``k`` slots.  Returns (table (n_refs k, 66) uint64, best (n_refs, H W) uint8, [cells(...) per reference])."""
    table = np.zeros((len(refs) * k, QUANTITIES), np.int64)
    best, per = [], []
    for r, ri in enumerate(refs):
        c = cells(cams, ri, w_match, h_match, audit_certainty)
        for j in range(len(ri.nbr_cams)):
            row = table[r * k + j]
            row[0] = c["usable"][:, j].sum()
            row[1] = (c["conf"][:, j] & ~c["usable"][:, j]).sum()
            row[2:] = np.bincount(c["bin"][c["usable"][:, j], j], minlength=64)
        best.append(c["best"])
        per.append(c)
    return table.view(np.uint64), np.stack(best), per
