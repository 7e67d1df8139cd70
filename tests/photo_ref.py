"""The yardstick of the photo-consistency gate's tests (lfd_photo_gate): a brute-force evaluation of the rule as the header
states it - the samples in NumPy f32, operation by operation (tests/colour_ref.py's blend, tests/support_ref.py's mask lookup), the sums in
int64, the verdict per point in Python integers and Python floats (IEEE f64, one rounding per product).  It shares no code with
csrc/lfd_photo.hpp.

Per input point of a reference, made by winning slot s on cell (y, x) of the H x W grid:

    guard     cell outside [0, H W) or s >= number of slots: kept, status 0
    window    cells (y + dy, x + dx), |dy|, |dx| <= R, inside the grid; one takes part iff the slot's raw certainty there is > 0, its
              observation (xb, yb) is finite and -1 <= xb, yb <= 1, the mask_b pixel the observation points at is set, the cell's own mask_a
              pixel is set
    samples   reference image at the match pixel of the cell's reference position (warp channels 0, 1, else the axes), neighbour image at
              the match pixel of (xb, yb): the four-tap f32 blend; each channel clamped to [0, 1] (NaN -> 0), times 4096, truncated; a, b
              their sums over the three channels
    sums      n, Sa, Sb, Saa, Sbb, Sab; va = n Saa - Sa^2, vb = n Sbb - Sb^2, cov = n Sab - Sa Sb
    verdict   1 kept: 2 n < (2R + 1)^2 + 1;  2 kept: va < n^2 T or vb < n^2 T, T = ceil((min_texture * 12288 / 255)^2);
              3 kept: cov > 0 and float(cov) * float(cov) >= (min_ncc * min_ncc) * (float(va) * float(vb));  4 dropped: otherwise
    ncc       f32(cov / sqrt(va vb)) for status 3 and 4 (NaN where va vb = 0), NaN otherwise
"""
from __future__ import annotations

import math

import numpy as np

import colour_ref
import support_ref
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

f32 = np.float32


def texture_floor(min_texture) -> int:
    s = float(f32(min_texture)) * 12288.0 / 255.0
    return int(math.ceil(s * s))


def grey(img, x, y):
    """(n,) int64: the three quantised channels of the blend of ``img`` at match px (x, y), summed."""
    with np.errstate(all="ignore"):
        c = colour_ref.bilinear(img, x, y)
        c = np.where(c >= 0, c, f32(0.0)).astype(f32)              # (a NaN is not >= 0)
        c = np.minimum(c, f32(1.0))
        return np.floor(c * f32(4096.0)).astype(np.int64).sum(axis=1)


def verdict(n, Sa, Sb, Saa, Sbb, Sab, R, T, min_ncc):
    """One point, Python integers.  (status, ncc)"""
    nan = f32(np.nan)
    side = 2 * R + 1
    if 2 * n < side * side + 1:
        return 1, nan
    va, vb, cov = n * Saa - Sa * Sa, n * Sbb - Sb * Sb, n * Sab - Sa * Sb
    assert max(abs(va), abs(vb), abs(cov), n * Saa, n * Sbb, n * Sab) < 3.7e11
    if va < n * n * T or vb < n * n * T:
        return 2, nan
    t2 = float(f32(min_ncc)) * float(f32(min_ncc))
    fc, fv = float(cov), float(va) * float(vb)
    ncc = f32(fc / math.sqrt(fv)) if fv > 0.0 else nan
    return (3 if (cov > 0 and fc * fc >= t2 * fv) else 4), ncc


def reference(cert, warp, image, mask_a, masks_b, nbr_images, w_match, h_match, cell, slot, R, min_ncc, min_texture, sums=None, axes=None):
    """One reference's points.  cert [k] (H, W) f32, warp [k] (H, W, 2 | 4) f32, image (h_match, w_match, 3) u8, mask_a None or (h_match,
    w_match) u8, masks_b None or [k] of None / such masks, nbr_images [k] images; cell (n,) i32, slot (n,) u8.  Returns (status (n,) u8, kept
    (n,) bool, ncc (n,) f32); ``sums``: a list that receives the (n, 6) int64 sums; ``axes``: the batch's (axis_x, axis_y), None: the library's own."""
    k = len(cert)
    cell, slot = np.asarray(cell).astype(np.int64), np.asarray(slot).astype(np.int64)
    npts = cell.size
    H, W = np.asarray(cert[0]).shape
    if axes is not None:
        ax, ay = np.asarray(axes[0], f32), np.asarray(axes[1], f32)
    else:
        ax, ay = np.asarray(hb.identity_axis(W), f32), np.asarray(hb.identity_axis(H), f32)  # the A-grid axes as the library forms them
    sx, sy = f32(w_match) / f32(W), f32(h_match) / f32(H)
    guard = (cell < 0) | (cell >= H * W) | (slot >= k)
    acc = np.zeros((npts, 6), np.int64)
    for j in range(k):
        idx = np.nonzero(~guard & (slot == j))[0]
        if idx.size == 0:
            continue
        cj = np.asarray(cert[j], f32)
        wj = np.asarray(warp[j], f32)
        y, x = cell[idx] // W, cell[idx] % W
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                qy, qx = y + dy, x + dx
                inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                qy, qx, at = qy[inside], qx[inside], idx[inside]
                obs = wj[qy, qx]
                xb, yb = obs[:, -2], obs[:, -1]
                with np.errstate(invalid="ignore"):
                    part = (cj[qy, qx] > 0) & (xb >= f32(-1)) & (xb <= f32(1)) & (yb >= f32(-1)) & (yb <= f32(1))
                if masks_b is not None and masks_b[j] is not None:
                    part &= support_ref.mask_lookup(np.asarray(masks_b[j]), xb, yb, H, W, w_match, h_match)
                if mask_a is not None:
                    part &= np.asarray(mask_a)[support_ref.nearest_src(qy, sy, h_match), support_ref.nearest_src(qx, sx, w_match)] != 0
                qy, qx, at, obs = qy[part], qx[part], at[part], obs[part]
                if at.size == 0:
                    continue
                xa, ya = (obs[:, 0], obs[:, 1]) if obs.shape[1] == 4 else (ax[qx], ay[qy])
                with np.errstate(all="ignore"):
                    a = grey(np.asarray(image), colour_ref.match_px(xa, w_match - 1), colour_ref.match_px(ya, h_match - 1))
                    b = grey(np.asarray(nbr_images[j]), colour_ref.match_px(obs[:, -2], w_match - 1), colour_ref.match_px(obs[:, -1], h_match - 1))
                np.add.at(acc, at, np.stack([np.ones_like(a), a, b, a * a, b * b, a * b], axis=1))
    T = texture_floor(min_texture)
    status, ncc = np.zeros(npts, np.uint8), np.full(npts, np.nan, f32)
    for i in range(npts):
        if not guard[i]:
            status[i], ncc[i] = verdict(*(int(v) for v in acc[i]), R, T, min_ncc)
    if sums is not None:
        sums.append(acc)
    return status, status != 4, ncc


def batch_reference(refs, w_match, h_match, res, R, min_ncc, min_texture, sums=None, axes=None):
    """Every reference of a collected result ``res`` for the ReferenceInputs ``refs`` (CPU tensors, nbr_images included)."""
    off = np.asarray(res.ref_offsets)
    cell, slot = res.cell.cpu().numpy(), res.slot.cpu().numpy()
    status, ncc = np.zeros(cell.shape, np.uint8), np.full(cell.shape, np.nan, f32)
    for r, ri in enumerate(refs):
        a, b = int(off[r]), int(off[r + 1])
        status[a:b], _, ncc[a:b] = reference([c.cpu().numpy() for c in ri.cert], [w.cpu().numpy() for w in ri.warp], ri.image.cpu().numpy(),
                                             ri.mask_a.cpu().numpy() if ri.mask_a is not None else None,
                                             [m.cpu().numpy() if m is not None else None for m in ri.mask_b] if ri.mask_b is not None else None,
                                             [t.cpu().numpy() for t in ri.nbr_images], w_match, h_match, cell[a:b], slot[a:b], R, min_ncc,
                                             min_texture, sums, axes)
    return status, status != 4, ncc


def filtered(res, kept):
    """What the gate must return for ``res`` under the mask ``kept``: (xyz, rgb, err, cell, slot arrays, ref_offsets, seg_counts)."""
    off = np.asarray(res.ref_offsets)
    n_refs, k = res.seg_counts.shape
    new_off = np.zeros_like(off)
    seg = np.zeros((n_refs, k), np.int32)
    slot = res.slot.cpu().numpy()
    for r in range(n_refs):
        a, b = int(off[r]), int(off[r + 1])
        new_off[r + 1] = new_off[r] + int(kept[a:b].sum())
        s = slot[a:b][kept[a:b]]
        seg[r] = np.bincount(s[s < k], minlength=k)[:k]
    cols = [getattr(res, name).cpu().numpy()[kept] for name in ("xyz", "rgb", "err", "cell", "slot")]
    return cols, new_off, seg
