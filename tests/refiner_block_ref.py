"""The yardstick of the refiner-block tests (lfd_refiner_block): an f64 evaluation of one conv block of RoMa-v2's refiners

    a = sum over the 5 x 5 taps inside the plane of w[c][tap] x[tap]      g = s[c] a + t[c]      h = max(g, 0)
    z[o] = pb[o] + sum_c Wt[c][o] h[c]                                     (the pointwise part, C == 32)

from the bf16-rounded input and the f32 parameters, and the derived error bound an implementation of the specified order has to stay under.
With u = 2^-24 (f32), v = 2^-8 (bf16 has 8 significant bits), gamma(n) = n u / (1 - n u), starred values the f64 ones:

    G_c = |s_c| sum_taps |w x| + |t_c|          e_c = v h*_c + 1.01 gamma(27) G_c
    without the pointwise part   |out - h*_c| <= e_c
    with it                      |out_o - z*_o| <= v |z*_o| + 1.01 (gamma(C) (|pb_o| + sum_c |Wt_co| (h*_c + e_c)) + sum_c |Wt_co| e_c)

25 fmafs and the affine one are 26 roundings on sums of magnitude at most G_c (27 leaves room for the second-order terms together with the
factor 1.01); ReLU does not increase a difference; the bf16 rounding of h adds v |h|.  The pointwise chain is C more fmafs on terms whose
magnitudes are bounded by the starred values plus e_c, it inherits sum |Wt| e_c from its inputs, and its result is rounded to bf16 once.  Valid
while nothing under- or overflows in bf16: the tests use O(1) values.

Also here, shared by the CPU, the GPU and the shim tests: the shapes, the seeded cases (computed once per process), the folding of the
BatchNorm and a stand-in for the model's block module with the four attribute names the shim recognises.
"""
from __future__ import annotations

import functools

import numpy as np

U = 2.0 ** -24
V = 2.0 ** -8
EPS = 1e-5                      # BatchNorm2d's default

# (B, C, H, W): the smallest shapes at which the kernels can go wrong - they work on 64 x 16 tiles
SHAPES = [
    (1, 1, 1, 1),               # the smallest possible input
    (1, 3, 4, 5),               # image smaller than the window; every tap pattern at a border
    (1, 1, 2, 131),             # odd W, several tiles along x
    (2, 32, 7, 9),              # batch stride
    (1, 32, 17, 67),            # tile plus remainder on both axes
    (1, 32, 35, 131),           # ... and an interior tile row
    (1, 33, 9, 9),              # channel count not a multiple of anything
    (1, 128, 20, 70),           # the patch-2 refiner's width
    (2, 512, 6, 6),             # the patch-4 refiner's width
]
# (shape, input is f32, with the pointwise part)
VARIANTS = [(s, f32, pw) for s in SHAPES for f32 in (False, True) for pw in ((False, True) if s[1] == 32 else (False,))]


def variant_id(v):
    (B, C, H, W), f32, pw = v
    return f"{B}x{C}x{H}x{W}-{'f32' if f32 else 'bf16'}-{'pw' if pw else 'dw'}"


def gamma(n: int) -> float:
    return n * U / (1.0 - n * U)


def bf16_round(x) -> np.ndarray:
    """f32 array -> the nearest bf16 values (ties to even) as f32, NaN kept quiet: the library's integer rule, in NumPy."""
    bits = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    nan = (bits & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    rounded = (bits.astype(np.uint64) + 0x7FFF + ((bits >> np.uint32(16)) & np.uint32(1))) >> np.uint64(16)
    top = np.where(nan, (bits >> np.uint32(16)) | np.uint32(0x40), rounded.astype(np.uint32)).astype(np.uint32)
    return (top << np.uint32(16)).view(np.float32)


def bf16_bits(x) -> np.ndarray:
    """f32 array of bf16 values -> their 16 bits."""
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def fold(gamma_bn, beta, mean, var, b_dw, eps: float = EPS):
    """s = gamma / sqrt(var + eps), t = beta + (b_dw - mean) s: in f64 from the f32 parameters, each rounded once to f32."""
    g, be, m, v, b = (np.asarray(a, np.float64) for a in (gamma_bn, beta, mean, var, b_dw))
    s = g / np.sqrt(v + eps)
    return s.astype(np.float32), (be + (b - m) * s).astype(np.float32)


def reference(xb, w, s, t, wt=None, pb=None):
    """(ref, bound), both (B, C, H, W) f64.  ``xb``: the input already rounded to bf16, any float dtype."""
    xb = np.asarray(xb, np.float64)
    B, C, H, W = xb.shape
    w64, s64, t64 = (np.asarray(a, np.float64) for a in (w, s, t))
    pad = np.zeros((B, C, H + 4, W + 4))
    pad[:, :, 2:2 + H, 2:2 + W] = xb
    a = np.zeros((B, C, H, W))
    mag = np.zeros((B, C, H, W))
    for ky in range(5):
        for kx in range(5):
            term = w64.reshape(C, 25)[None, :, 5 * ky + kx, None, None] * pad[:, :, ky:ky + H, kx:kx + W]
            a += term
            mag += np.abs(term)
    sc, tc = s64[None, :, None, None], t64[None, :, None, None]
    h = np.maximum(sc * a + tc, 0.0)
    e = V * h + 1.01 * gamma(27) * (np.abs(sc) * mag + np.abs(tc))
    if wt is None:
        return h, e
    wt64, pb64 = np.asarray(wt, np.float64).reshape(C, C), np.asarray(pb, np.float64)
    z = pb64[None, :, None, None] + np.einsum("co,bchw->bohw", wt64, h)
    carried = np.einsum("co,bchw->bohw", np.abs(wt64), e)
    sizes = np.abs(pb64)[None, :, None, None] + np.einsum("co,bchw->bohw", np.abs(wt64), h + e)
    return z, V * np.abs(z) + 1.01 * (gamma(C) * sizes + carried)


def violations(out, ref, bound):
    """(elements outside the bound or not finite, the largest |out - ref| / bound)."""
    out = np.asarray(out, np.float64)
    err = np.abs(out - ref)
    bad = ~(err <= bound)
    pos = bound > 0
    worst = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    return int(bad.sum()), worst


@functools.lru_cache(maxsize=None)
def case(shape, pointwise: bool = False, seed: int = 18):
    """A seeded block on a seeded input of ``shape``: O(1) values, normal weights, running variance from [0.5, 2].  A dict of NumPy arrays -
    the module's parameters (dw_w (C, 1, 5, 5), dw_b, bn_gamma, bn_beta, bn_mean, bn_var, pw_w (C, C, 1, 1), pw_b), the folded s / t, wt =
    pw_w transposed, x (f32, NOT rounded), xb (rounded to bf16) - with the f64 reference and bound of the variant.  Shared: do not modify."""
    B, C, H, W = shape
    rng = np.random.RandomState(seed + 1000 * C + H * W)
    d = dict(x=rng.standard_normal(shape).astype(np.float32),
             dw_w=(rng.standard_normal((C, 1, 5, 5)) * 0.2).astype(np.float32), dw_b=(rng.standard_normal(C) * 0.1).astype(np.float32),
             bn_gamma=(1.0 + 0.2 * rng.standard_normal(C)).astype(np.float32), bn_beta=(0.2 * rng.standard_normal(C)).astype(np.float32),
             bn_mean=(0.2 * rng.standard_normal(C)).astype(np.float32), bn_var=rng.uniform(0.5, 2.0, C).astype(np.float32),
             pw_w=(rng.standard_normal((C, C, 1, 1)) / np.sqrt(C)).astype(np.float32), pw_b=(0.1 * rng.standard_normal(C)).astype(np.float32))
    d["xb"] = bf16_round(d["x"])
    d["s"], d["t"] = fold(d["bn_gamma"], d["bn_beta"], d["bn_mean"], d["bn_var"], d["dw_b"])
    d["wt"] = np.ascontiguousarray(d["pw_w"].reshape(C, C).T)
    d["ref"], d["bound"] = reference(d["xb"], d["dw_w"], d["s"], d["t"], d["wt"] if pointwise else None, d["pw_b"] if pointwise else None)
    for v in d.values():
        v.setflags(write=False)
    return d


def tensors(d, f32_input: bool, pointwise: bool, device="cpu"):
    """The arguments of ``refiner_block`` for a case: (x, dw_w, s, t, wt or None, pb or None) as torch tensors on ``device``."""
    import torch
    x = torch.from_numpy(d["x"].copy()) if f32_input else torch.from_numpy(d["xb"].copy()).to(torch.bfloat16)
    small = [torch.from_numpy(d[k].copy()) for k in ("dw_w", "s", "t")] + ([torch.from_numpy(d["wt"].copy()), torch.from_numpy(d["pw_b"].copy())]
                                                                         if pointwise else [None, None])
    small[0] = small[0].reshape(-1, 25)
    return [x.to(device)] + [None if t is None else t.to(device) for t in small]


def to_numpy(out) -> np.ndarray:
    """A bf16 torch tensor -> f32 NumPy, exactly."""
    return out.detach().float().cpu().numpy()


def stand_in_block(d, enable_amp: bool = True, device="cpu"):
    """A module with the structure of the model's block - ``conv_depthwise`` (5 x 5, groups = channels), ``norm`` (BatchNorm2d), ``relu``,
    ``conv_pointwise`` (1 x 1) and ``enable_amp``, its forward the four of them under bf16 autocast - holding the parameters of case ``d``,
    in eval mode.  The model itself is not importable in the test tiers."""
    import torch
    from torch import nn

    class Block(nn.Module):
        def __init__(self, C):
            super().__init__()
            self.conv_depthwise = nn.Conv2d(C, C, kernel_size=5, padding=2, groups=C)
            self.norm = nn.BatchNorm2d(C)
            self.relu = nn.ReLU(inplace=True)
            self.conv_pointwise = nn.Conv2d(C, C, 1, 1, 0)
            self.enable_amp = enable_amp

        def forward(self, x):
            with torch.autocast(device_type=x.device.type, enabled=self.enable_amp, dtype=torch.bfloat16):
                return self.conv_pointwise(self.relu(self.norm(self.conv_depthwise(x))))

    C = int(d["dw_b"].shape[0])
    blk = Block(C)
    with torch.no_grad():
        for p, key in ((blk.conv_depthwise.weight, "dw_w"), (blk.conv_depthwise.bias, "dw_b"), (blk.norm.weight, "bn_gamma"),
                       (blk.norm.bias, "bn_beta"), (blk.norm.running_mean, "bn_mean"), (blk.norm.running_var, "bn_var"),
                       (blk.conv_pointwise.weight, "pw_w"), (blk.conv_pointwise.bias, "pw_b")):
            p.copy_(torch.from_numpy(d[key].copy()))
    return blk.to(device).eval().requires_grad_(False)
