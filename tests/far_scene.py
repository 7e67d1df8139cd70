"""What the tests of the far-field shell share (tests/test_far_*.py on the CPU, tests/test_gpu_far.py on the device): an analytic outdoor scene.

A short rig of cameras at z = 0, ``BASELINE`` apart along x, looks along +y with a little yaw and pitch each.  Rays that point below the
horizon meet the GROUND, the half plane y = 3 + 0.8 z (z <= 0): between 2.2 and 3 units in front of the rig, so it fills the lower half of
every image.  Rays that point above it meet the BACKDROP, the plane y = ``FAR_DEPTH`` = 10^5 x the rig's longest baseline, which fills the
upper half.  Both carry a smooth analytic texture (the backdrop's is a function of the direction from the rig, changing by less than a grey
level across a direction cell at the default shell resolution).  Warps are the exact projections of the surface point each grid cell of the
reference sees; certainties are analytic: a smooth value in [0.6, 0.9] where the point falls inside the neighbour's image, 0.05 where it
does not.  Match-size images are rendered per pixel, as tests/colour_scene.py renders its plane.

Options: an OCCLUDER - a rectangle of upper-half cells that ONE neighbour sees, confidently, on a surface 3 units away while the others see
the backdrop; masks; 2- or 4-channel warps.  ``write_scene`` puts the rig's photographs on disk and ``Matcher`` serves the same analytic
fields through the driver's matcher interface."""
import dataclasses
import math
import os

import numpy as np
import torch

from lichtfeld_densification_plugin_amd import synthetic as syn
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from lichtfeld_densification_plugin_amd.core.types import CameraRecord

N_CAMS = 4
BASELINE = 0.25
WIDTH, HEIGHT, FOCAL = 320, 208, 240.0
FAR_DEPTH = 1.0e5 * BASELINE * (N_CAMS - 1)
GROUND_Y0, GROUND_SLOPE = 3.0, 0.8
YAW_DEG = (-2.0, 0.0, 1.5, 3.0)
PITCH_DEG = (0.5, 0.0, -0.75, 0.25)
TEX_AMP, TEX_FREQ = 0.15, 0.6                  # backdrop: amplitude [0..1] and radians of phase per unit of tangent
_cams = []


def cameras():
    if not _cams:
        K = np.array([[FOCAL, 0.0, WIDTH / 2.0 + 0.75], [0.0, FOCAL * 1.003, HEIGHT / 2.0 - 0.5], [0.0, 0.0, 1.0]])
        for i in range(N_CAMS):
            a, p = math.radians(YAW_DEG[i]), math.radians(PITCH_DEG[i])
            fwd = np.array([math.sin(a) * math.cos(p), math.cos(a) * math.cos(p), math.sin(p)])
            right = np.cross(fwd, np.array([0.0, 0.0, 1.0]))
            right /= np.linalg.norm(right)
            down = np.cross(fwd, right)
            R = np.stack([right, down, fwd], axis=0)
            c = np.array([BASELINE * i, 0.02 * (i % 2), 0.0])
            _cams.append(CameraRecord.from_krt(i + 1, K, R, -R @ c, WIDTH, HEIGHT, image_path=f"far/{i:04d}.png"))
    return _cams


def rays(cam, x_px, y_px, match_w: int, match_h: int):
    """World directions (..., 3) f64 of match pixels, from the camera's f32 record evaluated in f64."""
    K, R = np.asarray(cam.K, np.float64), np.asarray(cam.R, np.float64)
    u, v = x_px * (cam.width / float(match_w)), y_px * (cam.height / float(match_h))
    return np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], axis=-1) @ R


def surface(cam, x_px, y_px, match_w: int, match_h: int):
    """(world point (..., 3), upper (...,) bool): the backdrop for a ray that points up, the ground for one that points down."""
    d = rays(cam, x_px, y_px, match_w, match_h)
    Cc = np.asarray(cam.C, np.float64)
    upper = d[..., 2] > 0
    s_far = (FAR_DEPTH - Cc[1]) / d[..., 1]
    s_gnd = (GROUND_Y0 + GROUND_SLOPE * Cc[2] - Cc[1]) / (d[..., 1] - GROUND_SLOPE * d[..., 2])
    s = np.where(upper, s_far, s_gnd)
    assert (s > 0).all()
    return Cc + s[..., None] * d, upper


def backdrop_texture(X):
    """(..., 3) f64 in [0.35, 0.75]: a function of the direction (X / Y, Z / Y) of the world point"""
    az, el = X[..., 0] / X[..., 1], X[..., 2] / X[..., 1]
    return np.stack([0.55 + TEX_AMP * np.sin(TEX_FREQ * (az + 0.4 * el) + 0.3), 0.55 + TEX_AMP * np.cos(TEX_FREQ * (0.7 * az - el) + 1.0),
                     0.55 + TEX_AMP * np.sin(TEX_FREQ * (el - 0.5 * az) + 2.0)], axis=-1)


def ground_texture(X):
    return np.stack([0.5 + 0.25 * np.sin(3.0 * X[..., 0]) * np.cos(2.5 * X[..., 2]), 0.45 + 0.2 * np.cos(2.0 * X[..., 0] + 1.0),
                     0.4 + 0.2 * np.sin(2.2 * X[..., 2] + 0.5)], axis=-1)


def render(cam, match_w: int, match_h: int):
    yy, xx = np.meshgrid(np.arange(match_h, dtype=np.float64), np.arange(match_w, dtype=np.float64), indexing="ij")
    X, upper = surface(cam, xx, yy, match_w, match_h)
    col = np.where(upper[..., None], backdrop_texture(X), ground_texture(X))
    return np.rint(255.0 * col).clip(0, 255).astype(np.uint8)


def project(cam, Xw, match_w: int, match_h: int):
    """Normalised coordinates of world points in ``cam`` and their depth there."""
    Xc = Xw @ np.asarray(cam.R, np.float64).T + np.asarray(cam.t, np.float64).reshape(3)
    u = cam.K[0, 0] * Xc[..., 0] / Xc[..., 2] + cam.K[0, 2]
    v = cam.K[1, 1] * Xc[..., 1] / Xc[..., 2] + cam.K[1, 2]
    return (u / (cam.width / float(match_w)) / (0.5 * (match_w - 1)) - 1.0, v / (cam.height / float(match_h)) / (0.5 * (match_h - 1)) - 1.0,
            Xc[..., 2])


def fields(ref: int, nbrs, H: int, W: int, match_w: int, match_h: int, occluder=None):
    """The analytic warps (H, W, 2) f64 and certainties (H, W) f64 of reference ``ref`` towards ``nbrs``, the reference's A-coordinates
    (xan, yan) (H, W) and ``upper`` (H, W).  ``occluder`` = (slot, y0, y1, x0, x1): the cells [y0, y1) x [x0, x1), as slot ``slot`` sees them,
    lie on a surface 3 units along their ray."""
    cams = cameras()
    camA = cams[ref]
    ax = syn.identity_axis_torch(W, "cpu").numpy().astype(np.float64)
    ay = syn.identity_axis_torch(H, "cpu").numpy().astype(np.float64)
    xan, yan = np.meshgrid(ax, ay)
    xA, yA = (xan + 1.0) * 0.5 * (match_w - 1), (yan + 1.0) * 0.5 * (match_h - 1)
    Xw, upper = surface(camA, xA, yA, match_w, match_h)
    d = rays(camA, xA, yA, match_w, match_h)
    near = np.asarray(camA.C, np.float64) + 3.0 * d / np.linalg.norm(d, axis=-1, keepdims=True)
    warps, certs = [], []
    for j, nb in enumerate(nbrs):
        P = Xw
        if occluder is not None and occluder[0] == j:
            inside = np.zeros((H, W), bool)
            inside[occluder[1]:occluder[2], occluder[3]:occluder[4]] = True
            P = np.where(inside[..., None], near, Xw)
        xb, yb, z = project(cams[nb], P, match_w, match_h)
        seen = (np.abs(xb) < 1.0) & (np.abs(yb) < 1.0) & (z > 0)
        cert = np.where(seen, 0.75 + 0.15 * np.sin(5.0 * xan + j) * np.cos(4.0 * yan - j), 0.05)
        warps.append(np.stack([xb, yb], axis=-1))
        certs.append(cert)
    return warps, certs, xan, yan, upper


@dataclasses.dataclass
class Scene:
    ref: int
    nbrs: list
    inputs: hb.ReferenceInputs           # CPU tensors
    upper: np.ndarray                    # (H, W) bool: the cells that look at the backdrop
    occluded: np.ndarray                 # (H, W) bool: the occluder's cells
    match: int


def make(ref: int, nbrs, H: int, W: int, match: int = 64, channels: int = 2, masks: bool = False, occluder=None) -> Scene:
    cams = cameras()
    warps, certs, xan, yan, upper = fields(ref, nbrs, H, W, match, match, occluder)
    tw, tc, mask_b = [], [], []
    for j in range(len(nbrs)):
        wp = warps[j]
        if channels == 4:
            wp = np.concatenate([np.stack([xan, yan], axis=-1), wp], axis=-1)
        tw.append(torch.from_numpy(wp.astype(np.float32)).contiguous())
        tc.append(torch.from_numpy(certs[j].astype(np.float32)).contiguous())
        m = np.ones((match, match), np.uint8)
        a = (match // 8) * (1 + j % 5)
        m[:, a:a + match // 10] = 0
        mask_b.append(torch.from_numpy(m))
    mask_a = np.ones((match, match), np.uint8)
    mask_a[match // 6:match // 6 + match // 12, :] = 0
    occ = np.zeros((H, W), bool)
    if occluder is not None:
        occ[occluder[1]:occluder[2], occluder[3]:occluder[4]] = True
    ri = hb.ReferenceInputs(ref_cam=ref, nbr_cams=list(nbrs), cert=tc, warp=tw, image=torch.from_numpy(render(cams[ref], match, match)),
                            mask_a=torch.from_numpy(mask_a) if masks else None, mask_b=mask_b if masks else None)
    return Scene(ref, list(nbrs), ri, upper, occ, match)


def others(ref: int, k: int):
    return [c for c in range(N_CAMS) if c != ref][:k]


def to_device(ri: hb.ReferenceInputs, dev) -> hb.ReferenceInputs:
    mv = lambda t: t.to(dev) if t is not None else None
    return dataclasses.replace(ri, cert=[mv(c) for c in ri.cert], warp=[mv(w) for w in ri.warp], image=mv(ri.image), mask_a=mv(ri.mask_a),
                               mask_b=[mv(m) for m in ri.mask_b] if ri.mask_b is not None else None)


# ---- the same scene for the driver: photographs on disk, a matcher that serves the analytic fields ---------------------------------------
def write_scene(root: str):
    """The rig's photographs at camera resolution under ``root``; returns camera records that name them."""
    from PIL import Image
    os.makedirs(root, exist_ok=True)
    out = []
    for i, c in enumerate(cameras()):
        path = os.path.join(root, f"view_{i:04d}.png")
        if not os.path.exists(path):
            Image.fromarray(render(c, c.width, c.height)).save(path)
        out.append(dataclasses.replace(c, image_path=path))
    return out


class Matcher(syn.SyntheticMatcher):
    """The analytic matcher of THIS scene: warps and certainties of ``fields`` on the preset's grid."""

    def __init__(self, cams, setting="turbo", device="cpu"):
        super().__init__(cams, setting=setting, device=device, channels=2)

    def fields(self, ref, nbrs):
        key = (int(ref), tuple(int(n) for n in nbrs))
        hit = self.table.get(key)
        if hit is None:
            warps, certs, _x, _y, _u = fields(key[0], list(key[1]), self.H, self.W, self.w_resized, self.h_resized)
            hit = [(torch.from_numpy(w.astype(np.float32)).contiguous().to(self.device), torch.from_numpy(c.astype(np.float32)).contiguous().to(self.device))
                   for w, c in zip(warps, certs)]
            self.table[key] = hit
        return key, [(w, c.clone()) for w, c in hit]
