"""The yardstick of the gain statistics' tests (lfd_gain_accumulate): a brute-force NumPy evaluation of the rule as the
header states it.

Per point X of reference r, made by winning slot s on cell c, and per slot j of the reference:

    guard    X or its colour not finite, c outside the grid, s >= number of slots: the point has no sample at all
    views    slot s unless its observation is not finite; every slot j != s that is live (raw certainty > 0, mask pixel set) and agrees
             with X within tau - tests/colour_ref.py's set, by its routines
    colour   of the neighbour: tests/colour_ref.py's four-tap f32 blend of its match-size image at its observation
    sample   counts iff the reference's r, g, b (the colour the point carries) and the neighbour's all lie in [0.05f, 0.95f]
    sums     row [r * k + j] of a uint64 (n_refs * k, 7) table: N += 1, Sref += trunc(c_ref * 2^24), Snbr += trunc(c_nbr * 2^24)

The sums are plain Python-sized integer additions (np.uint64), so nothing depends on an order."""
from __future__ import annotations

import numpy as np

import colour_ref
import support_ref

f32 = np.float32
LO, HI, SCALE = f32(0.05), f32(0.95), f32(16777216.0)


def quantise(c):
    """(uint64) of trunc(c * 2^24) for f32 c in [0.05, 0.95]: the product is exact (a power of two), the conversion truncates"""
    return (np.asarray(c, f32) * SCALE).astype(np.uint32).astype(np.uint64)


def in_range(c):
    c = np.asarray(c, f32)
    return ((c >= LO) & (c <= HI)).all(axis=-1)


def reference(cams, ref_cam, nbr_cams, cert, warp, masks_b, nbr_images, w_match, h_match, cell, slot, xyz, rgb, tau, k):
    """One reference's points -> (k, 7) uint64 rows (rows of slots the reference does not have stay zero), and per (point, slot) whether a
    view took part and whether its sample counted: (table, part (n, k) bool, counted (n, k) bool)."""
    ns = len(nbr_cams)
    cell, slot = np.asarray(cell).astype(np.int64), np.asarray(slot).astype(np.int64)
    xyz, rgb = np.asarray(xyz, f32).reshape(-1, 3), np.asarray(rgb, f32).reshape(-1, 3)
    n = cell.size
    H, W = np.asarray(cert[0]).shape
    guard = ~(np.isfinite(xyz).all(axis=1) & np.isfinite(rgb).all(axis=1)) | (cell < 0) | (cell >= H * W) | (slot >= ns)
    cs, ss = np.where(guard, 0, cell), np.where(guard, 0, slot)
    table = np.zeros((k, 7), np.uint64)
    part, counted = np.zeros((n, k), bool), np.zeros((n, k), bool)
    with np.errstate(all="ignore"):
        ref_ok = in_range(rgb)
        for j in range(ns):
            cam = cams[int(nbr_cams[j])]
            wj = np.asarray(warp[j], f32).reshape(H * W, -1)[cs]
            xb, yb = wj[:, -2], wj[:, -1]
            live = np.asarray(cert[j], f32).reshape(-1)[cs] > 0
            if masks_b is not None and masks_b[j] is not None:
                live &= support_ref.mask_lookup(np.asarray(masks_b[j]), xb, yb, H, W, w_match, h_match)
            ok = live & colour_ref.agree(cam.P, support_ref.pixel_scale(cam.width, w_match), support_ref.pixel_scale(cam.height, h_match), xyz,
                                         xb, yb, w_match, h_match, tau)
            part[:, j] = np.where(ss == j, np.isfinite(xb) & np.isfinite(yb), ok) & ~guard
            for i in np.nonzero(part[:, j])[0]:                              # brute force: a point at a time
                col = colour_ref.bilinear(np.asarray(nbr_images[j]), colour_ref.match_px(xb[i:i + 1], w_match - 1),
                                          colour_ref.match_px(yb[i:i + 1], h_match - 1))[0]
                if not (ref_ok[i] and in_range(col)):
                    continue
                counted[i, j] = True
                table[j, 0] += np.uint64(1)
                table[j, 1:4] += quantise(rgb[i])
                table[j, 4:7] += quantise(col)
    return table, part, counted


def batch_reference(cams, refs, nbr_images, w_match, h_match, res, tau, k):
    """Every reference of a collected result ``res`` for the ReferenceInputs ``refs`` (CPU tensors); nbr_images [r][j] arrays.  Returns the
    (n_refs * k, 7) uint64 table and the concatenated (n, k) part / counted masks."""
    off = np.asarray(res.ref_offsets)
    cell, slot, xyz, rgb = res.cell.cpu().numpy(), res.slot.cpu().numpy(), res.xyz.cpu().numpy(), res.rgb.cpu().numpy()
    tables, parts, counteds = [], [], []
    for r, ri in enumerate(refs):
        a, b = int(off[r]), int(off[r + 1])
        t, p, c = reference(cams, ri.ref_cam, ri.nbr_cams, [c.cpu().numpy() for c in ri.cert], [w.cpu().numpy() for w in ri.warp],
                            [m.cpu().numpy() if m is not None else None for m in ri.mask_b] if ri.mask_b is not None else None,
                            [np.asarray(im) for im in nbr_images[r]], w_match, h_match, cell[a:b], slot[a:b], xyz[a:b], rgb[a:b], tau, k)
        tables.append(t)
        parts.append(p)
        counteds.append(c)
    return np.concatenate(tables, axis=0), np.concatenate(parts, axis=0), np.concatenate(counteds, axis=0)
