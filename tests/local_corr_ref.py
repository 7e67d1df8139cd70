"""The yardstick of the local-correlation tests (lfd_local_corr): an f64 evaluation of

    out[b, n, k] = sum_c A[b, n, c] * bilinear(Bf[b, :, :, c]; warp[b, n, k])      (grid_sample: bilinear, zeros, align_corners=False)

from the f32 inputs, and the derived error bound every implementation has to stay under:

    |out - ref| <= (C + 10) u S + 2 delta T,   u = 2^-24,  delta = 3 u (max(W1, H1) + 1)
    S = sum_c |A[c]| * bilinear(|Bf[.., c]|; ix, iy)
    T = sum_c |A[c]| * R_c,  R_c = max - min of Bf[.., c] over the 3 x 3 texels centred on (round(ix), round(iy)), outside texels = 0

and out == 0 exactly where the right-hand side is 0.  First term: C - 1 additions in any order, one product, a four-term blend.  Second term:
the f32 un-normalisation of the coordinate rounds three times, each by at most u (W1 + 1), so the position is off by at most delta per axis,
and a bilinear interpolant moves by at most the local texel range per texel of shift.  A non-finite coordinate contributes 0 (the documented
departure from grid_sample), so there ref = S = T = 0.

``reference_numpy`` is the definition (NumPy, chunked); ``reference_torch`` is the same arithmetic in torch f64 for the shapes of the GPU
tests, where NumPy on one core would take minutes - the GPU tests check it against ``reference_numpy`` on their small cases first.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
PAD = 2          # zero texels round the map: a clamped index beyond the map lands on one of them


def delta(H1: int, W1: int) -> float:
    return 3.0 * U * (max(H1, W1) + 1)


def reference_numpy(A, Bf, warp, chunk: int = 1 << 13):
    """(ref, bound), both (B, N, K) f64."""
    A, Bf, warp = np.asarray(A), np.asarray(Bf), np.asarray(warp)
    B, N, C = A.shape
    _, H1, W1, _ = Bf.shape
    K = warp.shape[2]
    ref = np.zeros((B, N * K), np.float64)
    bound = np.zeros((B, N * K), np.float64)
    for b in range(B):
        pad = np.zeros((H1 + 2 * PAD, W1 + 2 * PAD, C), np.float64)
        pad[PAD:PAD + H1, PAD:PAD + W1] = Bf[b]
        a64 = A[b].astype(np.float64)
        xy = warp[b].reshape(N * K, 2).astype(np.float64)
        for s0 in range(0, N * K, chunk):
            s1 = min(N * K, s0 + chunk)
            x, y = xy[s0:s1, 0], xy[s0:s1, 1]
            fin = np.isfinite(x) & np.isfinite(y)
            with np.errstate(all="ignore"):
                ix = np.where(fin, ((x + 1.0) * W1 - 1.0) / 2.0, -4.0)
                iy = np.where(fin, ((y + 1.0) * H1 - 1.0) / 2.0, -4.0)
            # beyond four texels outside nothing of the map is within reach of the taps or of the 3 x 3 window: clamp the position there
            ix, iy = np.clip(ix, -4.0, W1 + 3.0), np.clip(iy, -4.0, H1 + 3.0)
            a = a64[np.arange(s0, s1) // K]
            x0, y0 = np.floor(ix), np.floor(iy)
            r = np.zeros(s1 - s0)
            S = np.zeros(s1 - s0)
            for dy in (0, 1):
                for dx in (0, 1):
                    w = (1.0 - np.abs(ix - (x0 + dx))) * (1.0 - np.abs(iy - (y0 + dy)))
                    v = pad[_index(y0 + dy, H1), _index(x0 + dx, W1)]
                    r += w * (a * v).sum(1)
                    S += w * (np.abs(a) * np.abs(v)).sum(1)
            rx, ry = np.floor(ix + 0.5), np.floor(iy + 0.5)
            hi = lo = None
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    v = pad[_index(ry + dy, H1), _index(rx + dx, W1)]
                    hi = v if hi is None else np.maximum(hi, v)
                    lo = v if lo is None else np.minimum(lo, v)
            T = (np.abs(a) * (hi - lo)).sum(1)
            ref[b, s0:s1] = r
            bound[b, s0:s1] = (C + 10) * U * S + 2.0 * delta(H1, W1) * T
    return ref.reshape(B, N, K), bound.reshape(B, N, K)


def _index(i, size):
    return np.clip(i.astype(np.int64) + PAD, 0, size + 2 * PAD - 1)


def reference_torch(A, Bf, warp, chunk: int = 1 << 16):
    """``reference_numpy`` in torch f64 on the tensors' device; (ref, bound) as (B, N, K) f64 tensors there."""
    import torch
    B, N, C = A.shape
    _, H1, W1, _ = Bf.shape
    K = warp.shape[2]
    dev = A.device
    ref = torch.zeros((B, N * K), dtype=torch.float64, device=dev)
    bound = torch.zeros((B, N * K), dtype=torch.float64, device=dev)

    def index(i, size):
        return (i.to(torch.int64) + PAD).clamp(0, size + 2 * PAD - 1)

    for b in range(B):
        pad = torch.zeros((H1 + 2 * PAD, W1 + 2 * PAD, C), dtype=torch.float64, device=dev)
        pad[PAD:PAD + H1, PAD:PAD + W1] = Bf[b].double()
        a64 = A[b].double()
        xy = warp[b].reshape(N * K, 2).double()
        for s0 in range(0, N * K, chunk):
            s1 = min(N * K, s0 + chunk)
            x, y = xy[s0:s1, 0], xy[s0:s1, 1]
            fin = torch.isfinite(x) & torch.isfinite(y)
            far = torch.full_like(x, -4.0)
            ix = torch.where(fin, ((x + 1.0) * W1 - 1.0) / 2.0, far).clamp(-4.0, W1 + 3.0)
            iy = torch.where(fin, ((y + 1.0) * H1 - 1.0) / 2.0, far).clamp(-4.0, H1 + 3.0)
            a = a64[torch.arange(s0, s1, device=dev) // K]
            x0, y0 = torch.floor(ix), torch.floor(iy)
            r = torch.zeros(s1 - s0, dtype=torch.float64, device=dev)
            S = torch.zeros_like(r)
            for dy in (0, 1):
                for dx in (0, 1):
                    w = (1.0 - (ix - (x0 + dx)).abs()) * (1.0 - (iy - (y0 + dy)).abs())
                    v = pad[index(y0 + dy, H1), index(x0 + dx, W1)]
                    r += w * (a * v).sum(1)
                    S += w * (a.abs() * v.abs()).sum(1)
            rx, ry = torch.floor(ix + 0.5), torch.floor(iy + 0.5)
            hi = lo = None
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    v = pad[index(ry + dy, H1), index(rx + dx, W1)]
                    hi = v if hi is None else torch.maximum(hi, v)
                    lo = v if lo is None else torch.minimum(lo, v)
            T = (a.abs() * (hi - lo)).sum(1)
            ref[b, s0:s1] = r
            bound[b, s0:s1] = (C + 10) * U * S + 2.0 * delta(H1, W1) * T
    return ref.reshape(B, N, K), bound.reshape(B, N, K)


def violations(out, ref, bound, scale: float = 1.0):
    """(number of elements outside ``scale * bound`` or non-zero where the bound is 0, largest |out - ref| / bound over bound > 0).  NumPy arrays
    or torch tensors."""
    err = abs(out - ref)
    bad = (err > scale * bound) | ((bound == 0) & (out != 0)) | (out != out)
    pos = bound > 0
    worst = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    return int(bad.sum()), worst


def model_case(B, C, h, w, r, seed, H1=None, W1=None, sigma=0.3):
    """Inputs shaped like the refiners' call: A (B, h w, C) already divided by sqrt(C), Bf (B, H1, W1, C), warp (B, h w, (2r + 1)^2, 2) = the
    identity grid of the (h, w) queries + N(0, sigma) + a (2r + 1)^2 lattice at one-query-pixel spacing.  f32 NumPy arrays."""
    rng = np.random.RandomState(seed)
    H1, W1 = H1 or h, W1 or w
    A = (rng.standard_normal((B, h * w, C)) / np.sqrt(C)).astype(np.float32)
    Bf = rng.standard_normal((B, H1, W1, C)).astype(np.float32)
    gx = (np.arange(w) + 0.5) * 2.0 / w - 1.0
    gy = (np.arange(h) + 0.5) * 2.0 / h - 1.0
    centre = np.stack(np.meshgrid(gx, gy, indexing="xy"), -1).reshape(1, h * w, 1, 2) + sigma * rng.standard_normal((B, h * w, 1, 2))
    oy, ox = np.meshgrid(np.arange(-r, r + 1) * 2.0 / h, np.arange(-r, r + 1) * 2.0 / w, indexing="ij")
    window = np.stack([ox, oy], -1).reshape(1, 1, (2 * r + 1) ** 2, 2)
    return A, Bf, (centre + window).astype(np.float32)
