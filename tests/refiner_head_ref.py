"""The yardstick of the refiner-head tests (lfd_refiner_head): an f64 evaluation of the output head of RoMa-v2's refiners

    a_o = b_o + sum_c w_oc z_c                                     o = 0..5
    warp = prev_warp + (a_0 / (r W), a_1 / (r H))                  r = refine_init
    sp(v) = v if v > 20 else log1p(exp(v));  l00 = sp(a_3) + eps, l10 = a_4, l11 = sp(a_5) + eps        eps = (f32) 1e-6
    d = (a_2, l00^2, l00 l10, l10^2 + l11^2);  conf = prev + d     (prev_dim 1: channels 1..3 of prev are 0; prev_dim 0: conf = d)

from the f32 / bf16 inputs, and the derived error bound an f32 implementation of the specified order has to stay under.  With u = 2^-24,
gamma(n) = n u / (1 - n u), S_o = |b_o| + sum_c |w_oc z_c|, starred values the f64 ones and E(.) the bound of a value:

    E(a_o)   = 1.01 gamma(C + 1) S_o                                C fmafs on partial sums of magnitude at most S_o
    E(t)     = 1.01 (E(a) + 2 u (|a*| + E(a))) / q*                 t = a / q: the product q = r W and the division round once each
    E(warp)  = E(t) + 1.01 u (|warp*| + E(t))                       one add
    E(sp)    = E(a) + 1.01 u |sp*| (+ e^-20 where |a* - 20| <= E(a))   softplus has a derivative <= 1; its f64 value is rounded to f32 once;
                                                                    the two sides of the threshold differ by log1p(e^-v) <= e^-20
    E(l)     = E(sp) + 1.01 u (|l*| + E(sp))                        the add of eps;  E(l10) = E(a_4)
    E(x y)   = (|x*| E(y) + |y*| E(x) + E(x) E(y)) (1 + u) + 1.01 u |x* y*|           a rounded product
    E(d_3)   = E(l10 l10) + E(l11 l11) + 1.01 u (|d_3*| + E(l10 l10) + E(l11 l11))     two rounded products, then one add
    E(conf_k) = E(d_k) + 1.01 u (|conf_k*| + E(d_k))                the last add; without a previous confidence E(conf_k) = E(d_k)

Valid while nothing under- or overflows: the tests use O(1) values.

Device against twin (``twin_bound``): warp and conf[..., 0] contain no library call and are the same bits.  The libraries' exp and log1p agree
to a few f64 ulp, so (f32) log1p(exp(v)) differs by at most one f32 ulp between them and - a rounded add is monotone - so do l00 and l11: by a
factor (1 + delta), |delta| <= 2^-23.  l00^2 then differs by 2^-22 plus two roundings of 2^-24: 0.75 * 2^-21 of itself; l00 l10 by 2^-23 plus
two roundings: 2^-22; l10^2 + l11^2 by at most 0.75 * 2^-21 (l11^2's share, both terms are positive) plus the sum's two roundings, 2^-23:
2^-21.  So |d_k - d_k'| <= 2^-21 |d_k|, k = 1..3, and the last add contributes its own two roundings, 2^-23 |conf_k|.  The bound is evaluated
on the f64 reference's magnitudes with the factor 1.01 for the second-order terms.

Also here, shared by the CPU, the GPU and the shim tests: the shapes, the seeded cases (computed once per process), torch's own tail and
stand-ins for the model's refiner module with the attribute names the shim recognises.
"""
from __future__ import annotations

import functools

import numpy as np

U = 2.0 ** -24
CHOL_EPS = float(np.float32(1e-6))
SP_THRESHOLD = 20.0
REFINE_INIT = 4.0

# (B, C, H, W): the smallest shapes at which the kernel can go wrong - a lane owns 2 adjacent pixels of an image (4 from 2^18 pixels on), a
# workgroup has 64 threads (256 once that makes 1024 workgroups), eight planes are in flight per step; an odd H W takes the element-wise path
SHAPES = [
    (1, 1, 1, 1),               # the smallest possible input
    (1, 3, 4, 5),               # fewer channels than a step, even H W
    (2, 32, 7, 9),              # batch stride, odd H W: element-wise loads and a half-used last lane
    (1, 32, 3, 131),            # odd W, odd H W
    (1, 32, 17, 64),            # more than one workgroup, vector loads
    (1, 128, 5, 70),            # the patch-2 refiner's width
    (2, 512, 3, 6),             # the patch-4 refiner's width
    (1, 33, 9, 9),              # a channel count that leaves a remainder behind the steps of eight
]
WIDE_SHAPE = (1, 2, 512, 512)   # 2^18 pixels: the 4-pixel lanes (GPU tier)
LARGE_SHAPE = (1, 1, 1024, 1024)  # 2^20 pixels: 1024 workgroups of 256 threads (GPU tier)
# (shape, z is f32, prev_dim, previous state handed over as permuted planar views)
VARIANTS = [(s, f32, pd, planar) for s in SHAPES for f32 in (False, True) for pd, planar in ((0, False), (1, True), (4, False), (4, True))]


def variant_id(v):
    (B, C, H, W), f32, pd, planar = v
    return f"{B}x{C}x{H}x{W}-{'f32' if f32 else 'bf16'}-prev{pd}-{'planar' if planar else 'contiguous'}"


def gamma(n: int) -> float:
    return n * U / (1.0 - n * U)


def bf16_round(x) -> np.ndarray:
    """f32 array -> the nearest bf16 values (ties to even) as f32."""
    bits = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    rounded = (bits.astype(np.uint64) + 0x7FFF + ((bits >> np.uint32(16)) & np.uint32(1))) >> np.uint64(16)
    return (rounded.astype(np.uint32) << np.uint32(16)).view(np.float32)


def softplus64(v):
    v = np.asarray(v, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.where(v > SP_THRESHOLD, v, np.log1p(np.exp(v)))


def _product(x, ex, y, ey):
    """the bound of a rounded product of two values with bounds ex, ey"""
    return (np.abs(x) * ey + np.abs(y) * ex + ex * ey) * (1.0 + U) + 1.01 * U * np.abs(x * y)


def reference(z, head_w, head_b, prev_warp, prev_conf=None, refine_init: float = REFINE_INIT):
    """(warp, warp_bound, conf, conf_bound, d), all f64: (B, H, W, 2) twice, (B, H, W, 4) three times; d = conf - prev, the bound's
    magnitudes for ``twin_bound``.  ``z`` (B, C, H, W) holds the values the kernel reads (bf16 values already rounded), any float dtype."""
    z = np.asarray(z, np.float64)
    B, C, H, W = z.shape
    w, b = np.asarray(head_w, np.float64).reshape(6, C), np.asarray(head_b, np.float64).reshape(6)
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.einsum("oc,bchw->bhwo", w, z) + b
        S = np.einsum("oc,bchw->bhwo", np.abs(w), np.abs(z)) + np.abs(b)
        Ea = 1.01 * gamma(C + 1) * S
        q = np.float64(np.float32(refine_init)) * np.array([W, H], np.float64)
        t = a[..., :2] / q
        Et = 1.01 * (Ea[..., :2] + 2 * U * (np.abs(a[..., :2]) + Ea[..., :2])) / q
        warp = np.asarray(prev_warp, np.float64) + t
        Ewarp = Et + 1.01 * U * (np.abs(warp) + Et)

        def chol(k):
            sp = softplus64(a[..., k])
            Esp = Ea[..., k] + 1.01 * U * np.abs(sp) + np.where(np.abs(a[..., k] - SP_THRESHOLD) <= Ea[..., k], np.exp(-SP_THRESHOLD), 0.0)
            l = sp + CHOL_EPS
            return l, Esp + 1.01 * U * (np.abs(l) + Esp)

        (l00, E00), (l11, E11), l10, E10 = chol(3), chol(5), a[..., 4], Ea[..., 4]
        s0, s1, Es0, Es1 = l10 * l10, l11 * l11, _product(l10, E10, l10, E10), _product(l11, E11, l11, E11)
        d = np.stack([a[..., 2], l00 * l00, l00 * l10, s0 + s1], -1)
        Ed = np.stack([Ea[..., 2], _product(l00, E00, l00, E00), _product(l00, E00, l10, E10), Es0 + Es1 + 1.01 * U * (np.abs(s0 + s1) + Es0 + Es1)], -1)
        if prev_conf is None:
            return warp, Ewarp, d, Ed, d
        prev = np.asarray(prev_conf, np.float64)
        if prev.shape[-1] == 1:
            prev = np.concatenate([prev, np.zeros(prev.shape[:3] + (3,))], -1)
        conf = prev + d
        return warp, Ewarp, conf, Ed + 1.01 * U * (np.abs(conf) + Ed), d


def twin_bound(conf_ref, d_ref, prev_dim: int):
    """The largest |device - twin| of conf, (B, H, W, 4): 0 for channel 0, the derived distance for channels 1..3 (the module's docstring)."""
    tol = 1.01 * (2.0 ** -21 * np.abs(d_ref) + (2.0 ** -23 * np.abs(conf_ref) if prev_dim else 0.0))
    tol[..., 0] = 0.0
    return tol


def violations(out, ref, bound):
    """(elements outside the bound or not finite, the largest |out - ref| / bound)."""
    out = np.asarray(out, np.float64)
    err = np.abs(out - ref)
    bad = ~(err <= bound)
    pos = bound > 0
    worst = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    return int(bad.sum()), worst


@functools.lru_cache(maxsize=None)
def case(shape, prev_dim: int = 4, seed: int = 22):
    """Seeded heads on a seeded activation of ``shape``: O(1) values.  A dict of NumPy arrays - the modules' parameters (warp_w (2, C, 1, 1),
    warp_b, conf_w (4, C, 1, 1), conf_b), head_w (6, C) / head_b (6) as the kernel takes them, z (f32, NOT rounded), zb (rounded to bf16),
    prev_warp (B, H, W, 2), prev_conf (B, H, W, prev_dim) or None - with the f64 reference and bounds for the bf16 activation (``ref``) and
    for the f32 one (``ref32``): (warp, warp_bound, conf, conf_bound, d).  Shared: do not modify."""
    B, C, H, W = shape
    rng = np.random.RandomState(seed + 1000 * C + H * W + 7 * prev_dim)
    d = dict(z=rng.standard_normal(shape).astype(np.float32),
             warp_w=(rng.standard_normal((2, C, 1, 1)) / np.sqrt(C)).astype(np.float32), warp_b=(0.1 * rng.standard_normal(2)).astype(np.float32),
             conf_w=(rng.standard_normal((4, C, 1, 1)) / np.sqrt(C)).astype(np.float32), conf_b=(0.1 * rng.standard_normal(4)).astype(np.float32),
             prev_warp=rng.uniform(-1.0, 1.0, (B, H, W, 2)).astype(np.float32))
    if prev_dim:
        d["prev_conf"] = rng.standard_normal((B, H, W, prev_dim)).astype(np.float32)
    d["zb"] = bf16_round(d["z"])
    d["head_w"] = np.ascontiguousarray(np.concatenate([d["warp_w"].reshape(2, C), d["conf_w"].reshape(4, C)], 0))
    d["head_b"] = np.concatenate([d["warp_b"], d["conf_b"]])
    for v in d.values():
        v.setflags(write=False)
    d["prev_conf"] = d.get("prev_conf")
    d["ref"] = reference(d["zb"], d["head_w"], d["head_b"], d["prev_warp"], d["prev_conf"])
    d["ref32"] = reference(d["z"], d["head_w"], d["head_b"], d["prev_warp"], d["prev_conf"])
    return d


def planar_view(x, device="cpu"):
    """(B, H, W, D) NumPy -> a torch tensor of that shape whose memory is (B, D, H, W): what the model's bhwc_interpolate hands over."""
    import torch
    return torch.from_numpy(np.transpose(x, (0, 3, 1, 2)).copy()).to(device).permute(0, 2, 3, 1)


def tensors(d, f32_input: bool, planar: bool = False, device="cpu"):
    """The arguments of ``refiner_head`` for a case: (z, head_w, head_b, prev_warp, prev_conf or None) as torch tensors on ``device``."""
    import torch
    z = torch.from_numpy(d["z"].copy()) if f32_input else torch.from_numpy(d["zb"].copy()).to(torch.bfloat16)
    give = (lambda x: planar_view(x, device)) if planar else (lambda x: torch.from_numpy(x.copy()).to(device))
    return [z.to(device), torch.from_numpy(d["head_w"].copy()).to(device), torch.from_numpy(d["head_b"].copy()).to(device), give(d["prev_warp"]),
            None if d["prev_conf"] is None else give(d["prev_conf"])]


def torch_tail(z, warp_head, confidence_head, prev_warp, prev_confidence, refine_init: float = REFINE_INIT):
    """The operator list of the model's tail on torch's own kernels: the f32 cast, the two convolutions, the permutes, the warp update,
    softplus, the precision conversion, the stack, the padding of a 1-channel previous confidence, the last add.  (warp, confidence)."""
    import torch
    import torch.nn.functional as F
    z = z.float()
    B, _, H, W = z.shape
    displacement = warp_head(z).permute(0, 2, 3, 1).view(B, H, W, 2)
    delta = confidence_head(z).permute(0, 2, 3, 1).view(B, H, W, 4)
    warp = prev_warp + displacement / (refine_init * torch.tensor((W, H), device=z.device)[None, None, None])
    l00, l10, l11 = F.softplus(delta[..., 1]) + 1e-6, delta[..., 2], F.softplus(delta[..., 3]) + 1e-6
    delta = torch.stack([delta[..., 0], l00 * l00, l00 * l10, l10 * l10 + l11 * l11], dim=-1)
    if prev_confidence is None:
        return warp, delta
    if prev_confidence.shape[-1] == 4:
        return warp, prev_confidence + delta
    padded = torch.zeros_like(delta)
    padded[..., :1] = prev_confidence
    return warp, padded + delta


def stand_in_heads(d, device="cpu"):
    """(warp_head, confidence_head): 1x1 Conv2d modules holding the parameters of case ``d``, eval mode, no grad."""
    import torch
    from torch import nn
    C = int(d["head_w"].shape[1])
    wh, ch = nn.Conv2d(C, 2, 1, 1, 0), nn.Conv2d(C, 4, 1, 1, 0)
    with torch.no_grad():
        for p, key in ((wh.weight, "warp_w"), (wh.bias, "warp_b"), (ch.weight, "conf_w"), (ch.bias, "conf_b")):
            p.copy_(torch.from_numpy(d[key].copy()))
    return wh.to(device).eval().requires_grad_(False), ch.to(device).eval().requires_grad_(False)


def to_numpy(t) -> np.ndarray:
    return t.detach().float().cpu().numpy()
