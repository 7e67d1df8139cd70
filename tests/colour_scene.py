"""What the tests of the multi-view colour share (tests/test_multiview_colour_*.py on the CPU, tests/test_gpu_multiview_colour.py on the device):
a textured plane z = 0 under a ring of cameras, one reference with k neighbours.  Warps are the exact projections of the plane points the
reference's grid cells see (optionally with matching noise), certainties distinct values in (0.2, 0.9); every view's match-size image is
RENDERED - per pixel the ray is intersected with the plane, a smooth albedo (one low-frequency sinusoid product per channel, in [0.4, 0.8])
is evaluated there, multiplied by the view's gain and quantised to u8 - so that all views photograph the same surface and differ by their
gain (exposure) and, optionally, by an occluder patch of constant colour painted into one of them."""
import dataclasses

import numpy as np
import torch

import lichtfeld_densification_plugin_amd as lfd
from lichtfeld_densification_plugin_amd import synthetic as syn
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

N_CAMS = 40
ALBEDO_AMP = 0.2
ALBEDO_FREQ = ((0.5, 0.4), (0.45, 0.55), (0.6, 0.35))        # rad per scene unit along x, y, per channel
ALBEDO_PHASE = ((0.3, 0.1), (1.1, 0.7), (2.0, 1.9))
ALBEDO_GRAD = max(ALBEDO_AMP * float(np.hypot(fx, fy)) for fx, fy in ALBEDO_FREQ)       # |grad albedo| <= amp * |(fx, fy)|, per scene unit
OCCLUDER = (255, 0, 255)
_cams = []


def cameras():
    if not _cams:
        _cams.extend(syn.ring_cameras(N_CAMS, radius=3.0, cam_height=6.0))
    return _cams


def albedo(X, Y):
    """(..., 3) f64 in [0.4, 0.8]"""
    return np.stack([0.6 + ALBEDO_AMP * np.sin(fx * X + px) * np.cos(fy * Y + py) for (fx, fy), (px, py) in zip(ALBEDO_FREQ, ALBEDO_PHASE)], axis=-1)


def plane_hits(cam, x_px, y_px, match: int):
    """World (X, Y) where the rays through match pixels (x_px, y_px) (f64 arrays) of ``cam`` meet z = 0 (every ray of these cameras does)."""
    K, R, Cc = np.asarray(cam.K, np.float64), np.asarray(cam.R, np.float64), np.asarray(cam.C, np.float64)
    u, v = x_px * (cam.width / float(match)), y_px * (cam.height / float(match))
    d = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], axis=-1) @ R
    assert (d[..., 2] < -1e-3).all()
    s = -Cc[2] / d[..., 2]
    return Cc[0] + s * d[..., 0], Cc[1] + s * d[..., 1]


def render(cam, match: int, gain: float, patch=None):
    """(match, match, 3) u8: round(255 gain albedo) per pixel; ``patch`` (y0, y1, x0, x1) is painted OCCLUDER."""
    yy, xx = np.meshgrid(np.arange(match, dtype=np.float64), np.arange(match, dtype=np.float64), indexing="ij")
    X, Y = plane_hits(cam, xx, yy, match)
    img = np.rint(255.0 * gain * albedo(X, Y)).clip(0, 255).astype(np.uint8)
    if patch is not None:
        img[patch[0]:patch[1], patch[2]:patch[3]] = OCCLUDER
    return img


def pixel_footprint(cam, match: int) -> float:
    """The largest distance on the plane between the hits of two pixels one step apart in x and y (the diagonal of a pixel's footprint)."""
    yy, xx = np.meshgrid(np.arange(match, dtype=np.float64), np.arange(match, dtype=np.float64), indexing="ij")
    X, Y = plane_hits(cam, xx, yy, match)
    d = [np.hypot(X[1:, 1:] - X[:-1, :-1], Y[1:, 1:] - Y[:-1, :-1]), np.hypot(X[1:, :-1] - X[:-1, 1:], Y[1:, :-1] - Y[:-1, 1:])]
    return float(max(a.max() for a in d))


@dataclasses.dataclass
class Scene:
    ref: int
    nbrs: list
    inputs: hb.ReferenceInputs           # CPU tensors, nbr_images included
    images: list                         # [k] (match, match, 3) u8 arrays: the neighbours' renderings
    truth: np.ndarray                    # (H, W, 3) f64: the albedo at the plane point each grid cell of the reference sees
    match: int
    gains: tuple


def make(ref: int, k: int, H: int, W: int, match: int = 128, channels: int = 2, masks: bool = False, gains=None, patch_in=None, patch=None,
         noise_px: float = 0.0, seed: int = 0) -> Scene:
    """``gains``: (reference, neighbour 0, ...), default all 1; ``patch_in``: the neighbour slot whose image carries the occluder ``patch``;
    ``masks``: every neighbour's mask blanks a band of its image (another one per slot), the reference has none."""
    cams = cameras()
    nbrs = syn.ring_neighbours(N_CAMS, ref, k)
    gains = tuple(gains) if gains is not None else (1.0,) * (k + 1)
    rng = np.random.default_rng(1000 * seed + ref)
    camA = cams[ref]
    ax = syn.identity_axis_torch(W, "cpu").numpy().astype(np.float64)
    ay = syn.identity_axis_torch(H, "cpu").numpy().astype(np.float64)
    xA, yA = np.meshgrid((ax + 1.0) * 0.5 * (match - 1), (ay + 1.0) * 0.5 * (match - 1))
    X, Y = plane_hits(camA, xA, yA, match)
    Xw = np.stack([X, Y, np.zeros_like(X)], axis=-1)
    warps, certs, images, mask_b = [], [], [], []
    for j, nb in enumerate(nbrs):
        cam = cams[nb]
        Xc = Xw @ np.asarray(cam.R, np.float64).T + np.asarray(cam.t, np.float64).reshape(3)
        u = cam.K[0, 0] * Xc[..., 0] / Xc[..., 2] + cam.K[0, 2] + noise_px * rng.standard_normal((H, W))
        v = cam.K[1, 1] * Xc[..., 1] / Xc[..., 2] + cam.K[1, 2] + noise_px * rng.standard_normal((H, W))
        xb = u / (cam.width / float(match)) / (0.5 * (match - 1)) - 1.0
        yb = v / (cam.height / float(match)) / (0.5 * (match - 1)) - 1.0
        wp = np.stack([xb, yb], axis=-1)
        if channels == 4:
            wp = np.concatenate([np.stack(np.meshgrid(ax, ay), axis=-1), wp], axis=-1)
        warps.append(torch.from_numpy(wp.astype(np.float32)).contiguous())
        certs.append(torch.from_numpy((0.2 + 0.7 * (rng.permutation(H * W).reshape(H, W) + 0.5 + 0.1 * j) / (H * W)).astype(np.float32)))
        images.append(render(cam, match, gains[j + 1], patch if patch_in == j else None))
        m = np.ones((match, match), np.uint8)
        a = (match // 8) * (1 + j % 5)
        m[:, a:a + match // 10] = 0
        m[a:a + match // 16, :] = 0
        mask_b.append(torch.from_numpy(m))
    ri = hb.ReferenceInputs(ref_cam=ref, nbr_cams=nbrs, cert=certs, warp=warps, image=torch.from_numpy(render(camA, match, gains[0])),
                            mask_b=mask_b if masks else None, nbr_images=[torch.from_numpy(im) for im in images])
    return Scene(ref, nbrs, ri, images, albedo(X, Y), match, gains)


def to_device(ri: hb.ReferenceInputs, dev) -> hb.ReferenceInputs:
    mv = lambda t: t.to(dev) if t is not None else None
    return dataclasses.replace(ri, cert=[mv(c) for c in ri.cert], warp=[mv(w) for w in ri.warp], image=mv(ri.image), mask_a=mv(ri.mask_a),
                               mask_b=[mv(m) for m in ri.mask_b] if ri.mask_b is not None else None,
                               nbr_images=[mv(t) for t in ri.nbr_images])


def params(**kw):
    return hb.make_params(lfd.DensePipelineConfig(output_path="", **kw))


def bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def result_on_host(res):
    return dataclasses.replace(res, xyz=res.xyz.cpu(), rgb=res.rgb.cpu(), err=res.err.cpu(), cell=res.cell.cpu(), slot=res.slot.cpu(), _packed=None)
