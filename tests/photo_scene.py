"""What the tests of the photo-consistency gate share (tests/test_photo_*.py on the CPU, tests/test_gpu_photo.py on the device):
tests/colour_scene.py's ring of cameras over the plane z = 0, one reference with k neighbours, under a FINE, NON-PERIODIC albedo.  The albedo
is seeded Gaussian noise filtered with a Gaussian of ``sigma_px`` match pixels OF THE REFERENCE'S IMAGE (correlation length about one pixel
there), standard deviation ``AMPLITUDE`` grey levels around mid-grey, laid out in the reference's pixel frame and carried to the plane by the
reference's own projection: albedo(X) = texture(reference pixel of X), bilinear between texels.  Every view's match-size image is RENDERED - per
pixel the ray is intersected with the plane (colour_scene.plane_hits), the albedo is evaluated there, multiplied by the view's gain and
quantised to u8.  Warps are the exact projections of the plane points the reference's grid cells see.

Options: a band of grid rows whose observations, in every slot, are slid by ``slide_px`` match pixels ALONG THEIR EPIPOLAR LINE (the Sampson
distance stays 0, the point triangulates cleanly to the wrong depth and reprojects exactly); a rectangle of cells that look at an untextured
region of constant albedo; masks (one for the reference, one per neighbour); 2- or 4-channel warps."""
import dataclasses

import numpy as np
import torch

import colour_scene as cs
from lichtfeld_densification_plugin_amd import synthetic as syn
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

AMPLITUDE = 25.0 / 255.0        # standard deviation of the albedo (the issue asks for at least 20 grey levels)
TINT = (1.0, 0.92, 0.85)


def _gauss_filter(a, sigma):
    r = int(np.ceil(4 * sigma))
    t = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-0.5 * (t / sigma) ** 2)
    g /= g.sum()
    a = np.apply_along_axis(lambda v: np.convolve(v, g, mode="same"), 0, a)
    return np.apply_along_axis(lambda v: np.convolve(v, g, mode="same"), 1, a)


class Albedo:
    """texture(reference pixel): a (match + 2 margin)^2 grid of filtered noise around the reference's image."""

    def __init__(self, cam, match, sigma_px, seed, flat=None):
        self.cam, self.match, self.margin = cam, match, match // 2
        n = match + 2 * self.margin
        t = _gauss_filter(np.random.default_rng(seed).standard_normal((n, n)), sigma_px)
        self.tex = 0.5 + AMPLITUDE * (t - t.mean()) / t.std()
        self.flat = flat                          # (y0, y1, x0, x1) in reference match px: constant albedo inside

    def ref_px(self, X, Y):
        cam = self.cam
        Xc = np.stack([X, Y, np.zeros_like(X)], axis=-1) @ np.asarray(cam.R, np.float64).T + np.asarray(cam.t, np.float64).reshape(3)
        u = cam.K[0, 0] * Xc[..., 0] / Xc[..., 2] + cam.K[0, 2]
        v = cam.K[1, 1] * Xc[..., 1] / Xc[..., 2] + cam.K[1, 2]
        return u / (cam.width / float(self.match)), v / (cam.height / float(self.match))

    def __call__(self, X, Y):
        """(..., 3) f64"""
        x, y = self.ref_px(X, Y)
        n = self.tex.shape[0]
        fx, fy = np.clip(x + self.margin, 0, n - 1.001), np.clip(y + self.margin, 0, n - 1.001)
        x0, y0 = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
        ax, ay = fx - x0, fy - y0
        t = self.tex
        v = (t[y0, x0] * (1 - ax) + t[y0, x0 + 1] * ax) * (1 - ay) + (t[y0 + 1, x0] * (1 - ax) + t[y0 + 1, x0 + 1] * ax) * ay
        if self.flat is not None:
            inside = (y >= self.flat[0]) & (y <= self.flat[1]) & (x >= self.flat[2]) & (x <= self.flat[3])
            v = np.where(inside, 0.5, v)
        return np.clip(v, 0.05, 0.95)[..., None] * np.asarray(TINT)


def render(cam, match, gain, albedo):
    yy, xx = np.meshgrid(np.arange(match, dtype=np.float64), np.arange(match, dtype=np.float64), indexing="ij")
    X, Y = cs.plane_hits(cam, xx, yy, match)
    return np.rint(255.0 * gain * albedo(X, Y)).clip(0, 255).astype(np.uint8)


def _project(cam, Xw, match):
    Xc = Xw @ np.asarray(cam.R, np.float64).T + np.asarray(cam.t, np.float64).reshape(3)
    u = cam.K[0, 0] * Xc[..., 0] / Xc[..., 2] + cam.K[0, 2]
    v = cam.K[1, 1] * Xc[..., 1] / Xc[..., 2] + cam.K[1, 2]
    return u / (cam.width / float(match)), v / (cam.height / float(match))


@dataclasses.dataclass
class Scene:
    ref: int
    nbrs: list
    inputs: hb.ReferenceInputs           # CPU tensors, nbr_images included
    match: int
    gains: tuple
    slid: np.ndarray                     # (H, W) bool: the cells whose observations were slid
    flat: np.ndarray                     # (H, W) bool: the cells of the untextured rectangle


def make(ref, k, H, W, match=128, channels=2, masks=False, gains=None, slide_rows=None, slide_px=0.0, flat_cells=None, sigma_px=1.0,
         seed=0) -> Scene:
    """``gains``: (reference, neighbour 0, ...), default 1, 0.8, 0.9, 1.1, ...; ``slide_rows`` (y0, y1): the grid rows slid by ``slide_px``;
    ``flat_cells`` (y0, y1, x0, x1): the grid cells (inclusive) inside the untextured rectangle, which reaches half a cell beyond them;
    ``masks``: the reference's mask blanks a band of its image, every neighbour's another one."""
    cams = cs.cameras()
    nbrs = syn.ring_neighbours(cs.N_CAMS, ref, k)
    gains = tuple(gains) if gains is not None else (1.0,) + tuple(0.8 + 0.1 * (j % 4) for j in range(k))
    rng = np.random.default_rng(1000 * seed + ref)
    camA = cams[ref]
    ax = syn.identity_axis_torch(W, "cpu").numpy().astype(np.float64)
    ay = syn.identity_axis_torch(H, "cpu").numpy().astype(np.float64)
    xA, yA = np.meshgrid((ax + 1.0) * 0.5 * (match - 1), (ay + 1.0) * 0.5 * (match - 1))
    flat = None
    flat_mask = np.zeros((H, W), bool)
    if flat_cells is not None:
        y0, y1, x0, x1 = flat_cells
        py, px = 0.5 * (match - 1) * (ay[1] - ay[0]), 0.5 * (match - 1) * (ax[1] - ax[0])
        flat = (yA[y0, 0] - 0.5 * py, yA[y1, 0] + 0.5 * py, xA[0, x0] - 0.5 * px, xA[0, x1] + 0.5 * px)
        flat_mask[y0:y1 + 1, x0:x1 + 1] = True
    albedo = Albedo(camA, match, sigma_px, 77 + seed, flat)
    X, Y = cs.plane_hits(camA, xA, yA, match)
    Xw = np.stack([X, Y, np.zeros_like(X)], axis=-1)
    CA = np.asarray(camA.C, np.float64).reshape(3)
    far = CA + 1.1 * (Xw - CA)                                     # a second point on every cell's ray: its image fixes the epipolar line
    slid = np.zeros((H, W), bool)
    if slide_rows is not None:
        slid[slide_rows[0]:slide_rows[1] + 1] = True
    warps, certs, images, mask_b = [], [], [], []
    for j, nb in enumerate(nbrs):
        cam = cams[nb]
        u, v = _project(cam, Xw, match)
        u2, v2 = _project(cam, far, match)
        du, dv = u2 - u, v2 - v
        norm = np.hypot(du, dv)
        u = u + np.where(slid, slide_px * du / norm, 0.0)
        v = v + np.where(slid, slide_px * dv / norm, 0.0)
        wp = np.stack([u / (0.5 * (match - 1)) - 1.0, v / (0.5 * (match - 1)) - 1.0], axis=-1)
        if channels == 4:
            wp = np.concatenate([np.stack(np.meshgrid(ax, ay), axis=-1), wp], axis=-1)
        warps.append(torch.from_numpy(wp.astype(np.float32)).contiguous())
        certs.append(torch.from_numpy((0.2 + 0.7 * (rng.permutation(H * W).reshape(H, W) + 0.5 + 0.1 * j) / (H * W)).astype(np.float32)))
        images.append(torch.from_numpy(render(cam, match, gains[j + 1], albedo)))
        m = np.ones((match, match), np.uint8)
        a = (match // 8) * (1 + j % 5)
        m[:, a:a + match // 10] = 0
        m[a:a + match // 16, :] = 0
        mask_b.append(torch.from_numpy(m))
    mask_a = np.ones((match, match), np.uint8)
    mask_a[match // 3:match // 3 + match // 12, :] = 0
    ri = hb.ReferenceInputs(ref_cam=ref, nbr_cams=nbrs, cert=certs, warp=warps, image=torch.from_numpy(render(camA, match, gains[0], albedo)),
                            mask_a=torch.from_numpy(mask_a) if masks else None, mask_b=mask_b if masks else None, nbr_images=images)
    return Scene(ref, nbrs, ri, match, gains, slid, flat_mask)


to_device = cs.to_device
params = cs.params
bits = cs.bits
result_on_host = cs.result_on_host


# ---- the shapes both tiers run (tests/test_photo_host.py, tests/test_gpu_photo.py) ------------------------------------------------------------
MATCH = 128
# (H, W, k, channels, masks, R): a 6 x 8 grid, where the R = 3 window crosses every border at once, and 20 x 24; every k, channel count, mask
# setting and radius at least once
SHAPES = [(6, 8, 1, 2, False, 3), (6, 8, 3, 4, True, 1), (6, 8, 16, 2, False, 2), (20, 24, 1, 4, False, 2), (20, 24, 3, 2, True, 3),
          (20, 24, 16, 4, True, 1), (20, 24, 3, 2, False, 1)]
_made = {}


def case(H, W, k, channels, masks):
    """Two references with a slid band and an untextured rectangle each - made once per shape."""
    key = (H, W, k, channels, masks)
    if key not in _made:
        _made[key] = [make(r, k, H, W, match=MATCH, channels=channels, masks=masks, slide_rows=(H // 2, H // 2 + max(2, H // 4)), slide_px=3.0,
                           flat_cells=(0, H // 3, 0, W // 3), seed=r) for r in (5, 21)]
    return _made[key]


def one_reference_empty(res, which):
    """``res`` (a collected result of two references) with reference ``which`` left without points."""
    n0 = int(res.ref_offsets[1])
    a, b = (n0, res.count) if which == 0 else (0, n0)
    seg = res.seg_counts.copy()
    seg[which] = 0
    offs = np.array([0, 0, b - a] if which == 0 else [0, b - a, b - a], np.int64)
    return dataclasses.replace(res, xyz=res.xyz[a:b].clone(), rgb=res.rgb[a:b].clone(), err=res.err[a:b].clone(), cell=res.cell[a:b].clone(),
                               slot=res.slot[a:b].clone(), ref_offsets=offs, seg_counts=seg, _packed=None, normals=None)


def ulp_apart(a, b):
    """Largest distance in f32 steps between two f32 arrays whose NaNs sit in the same places (asserted)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(a)
    key = lambda v: np.where(v.view(np.int32) < 0, np.int64(-2 ** 31) - v.view(np.int32).astype(np.int64), v.view(np.int32).astype(np.int64))
    return int(np.abs(key(a[ok]) - key(b[ok])).max()) if ok.any() else 0
