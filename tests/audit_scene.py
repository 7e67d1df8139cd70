"""What the tests of the epipolar audit share (tests/test_audit_*.py on the CPU, tests/test_gpu_audit.py on the device): an analytic rig.

Six cameras on a line at z = 0, ``BASELINE`` apart along x, all with the SAME orientation, looking along +y: a horizontal rig, so every
epipolar line is an image row.  Rays that point down meet the GROUND, the plane z = -1, unless they first reach the WALL, the plane y = 6,
which rays that point up meet as well: every cell sees a surface 1.4 to 6.5 units away and has parallax towards every neighbour.  Both
surfaces carry a smooth analytic texture.  Warps are the exact projections of the surface point each grid cell of the reference sees, through
the TRUE poses; certainties are analytic: a smooth value in [0.6, 0.9] where the point falls inside the neighbour's image, 0.05 where it does
not.

Options: ``pitched`` = (camera, degrees) - that camera's RECORD is rotated about its own x axis (the centre stays) while the warps stay those
of the true poses: a wrong pose; ``displaced`` = (y0, y1, x0, x1) - the observations of those cells are moved by ``DISPLACE_PX`` camera pixels
along the image column, across the epipolar line, in EVERY slot: something that moved between the photographs; masks; 2- or 4-channel warps.
``write_scene`` puts the rig's photographs on disk and ``Matcher`` serves the same analytic fields through the driver's matcher interface."""
import dataclasses
import math
import os

import numpy as np
import torch

from lichtfeld_densification_plugin_amd import synthetic as syn
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from lichtfeld_densification_plugin_amd.core.types import CameraRecord

N_CAMS = 6
BASELINE = 0.25
WIDTH, HEIGHT, FOCAL = 320, 240, 240.0
GROUND_Z, WALL_Y = -1.0, 6.0
DISPLACE_PX = 3.0
_cams = {}


def cameras(pitched=None):
    """The records the library is given.  ``pitched`` = (camera index, degrees): that record's rotation is Rx(theta) R, its centre unchanged."""
    key = None if pitched is None else (int(pitched[0]), float(pitched[1]))
    if key not in _cams:
        K = np.array([[FOCAL, 0.0, WIDTH / 2.0 + 0.75], [0.0, FOCAL, HEIGHT / 2.0 - 0.5], [0.0, 0.0, 1.0]])
        R0 = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])      # right = +x, down = -z, forward = +y
        out = []
        for i in range(N_CAMS):
            R = R0
            if key is not None and key[0] == i:
                a = math.radians(key[1])
                R = np.array([[1.0, 0.0, 0.0], [0.0, math.cos(a), -math.sin(a)], [0.0, math.sin(a), math.cos(a)]]) @ R0
            c = np.array([BASELINE * i, 0.0, 0.0])
            out.append(CameraRecord.from_krt(i + 1, K, R, -R @ c, WIDTH, HEIGHT, image_path=f"audit/{i:04d}.png"))
        _cams[key] = out
    return _cams[key]


def neighbours(ref: int, k: int):
    """The k nearest cameras of the rig (the lower index on ties)."""
    return sorted((c for c in range(N_CAMS) if c != ref), key=lambda c: (abs(c - ref), c))[:k]


def rays(cam, x_px, y_px, match_w: int, match_h: int):
    K, R = np.asarray(cam.K, np.float64), np.asarray(cam.R, np.float64)
    u, v = x_px * (cam.width / float(match_w)), y_px * (cam.height / float(match_h))
    return np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], axis=-1) @ R


def surface(cam, x_px, y_px, match_w: int, match_h: int):
    """(world point (..., 3), wall (...,) bool) of match pixels of a TRUE camera."""
    d = rays(cam, x_px, y_px, match_w, match_h)
    Cc = np.asarray(cam.C, np.float64)
    s_wall = (WALL_Y - Cc[1]) / d[..., 1]
    with np.errstate(divide="ignore"):
        s_gnd = np.where(d[..., 2] < 0, (GROUND_Z - Cc[2]) / np.where(d[..., 2] < 0, d[..., 2], -1.0), np.inf)
    wall = s_wall <= s_gnd
    s = np.where(wall, s_wall, s_gnd)
    assert (s > 0).all()
    return Cc + s[..., None] * d, wall


def texture(X, wall):
    g = np.stack([0.5 + 0.25 * np.sin(3.0 * X[..., 0]) * np.cos(2.5 * X[..., 1]), 0.45 + 0.2 * np.cos(2.0 * X[..., 0] + 1.0),
                  0.4 + 0.2 * np.sin(2.2 * X[..., 1] + 0.5)], axis=-1)
    w = np.stack([0.55 + 0.15 * np.sin(1.5 * X[..., 0] + 0.3), 0.55 + 0.15 * np.cos(1.2 * X[..., 2] + 1.0),
                  0.55 + 0.15 * np.sin(X[..., 0] - X[..., 2])], axis=-1)
    return np.where(wall[..., None], w, g)


def render(cam, match_w: int, match_h: int):
    yy, xx = np.meshgrid(np.arange(match_h, dtype=np.float64), np.arange(match_w, dtype=np.float64), indexing="ij")
    X, wall = surface(cam, xx, yy, match_w, match_h)
    return np.rint(255.0 * texture(X, wall)).clip(0, 255).astype(np.uint8)


def project(cam, Xw, match_w: int, match_h: int):
    Xc = Xw @ np.asarray(cam.R, np.float64).T + np.asarray(cam.t, np.float64).reshape(3)
    u = cam.K[0, 0] * Xc[..., 0] / Xc[..., 2] + cam.K[0, 2]
    v = cam.K[1, 1] * Xc[..., 1] / Xc[..., 2] + cam.K[1, 2]
    return (u / (cam.width / float(match_w)) / (0.5 * (match_w - 1)) - 1.0, v / (cam.height / float(match_h)) / (0.5 * (match_h - 1)) - 1.0,
            Xc[..., 2])


def fields(ref: int, nbrs, H: int, W: int, match_w: int, match_h: int, displaced=None):
    """The analytic warps (H, W, 2) f64 and certainties (H, W) f64 of reference ``ref`` towards ``nbrs`` through the TRUE poses, and the
    reference's A-coordinates (xan, yan) (H, W)."""
    cams = cameras()
    camA = cams[ref]
    ax = syn.identity_axis_torch(W, "cpu").numpy().astype(np.float64)
    ay = syn.identity_axis_torch(H, "cpu").numpy().astype(np.float64)
    xan, yan = np.meshgrid(ax, ay)
    xA, yA = (xan + 1.0) * 0.5 * (match_w - 1), (yan + 1.0) * 0.5 * (match_h - 1)
    Xw, _wall = surface(camA, xA, yA, match_w, match_h)
    inside = np.zeros((H, W), bool)
    if displaced is not None:
        inside[displaced[0]:displaced[1], displaced[2]:displaced[3]] = True
    warps, certs = [], []
    for j, nb in enumerate(nbrs):
        xb, yb, z = project(cams[nb], Xw, match_w, match_h)
        yb = yb + np.where(inside, DISPLACE_PX / (cams[nb].height / float(match_h)) / (0.5 * (match_h - 1)), 0.0)
        seen = (np.abs(xb) < 1.0) & (np.abs(yb) < 1.0) & (z > 0)
        cert = np.where(seen, 0.75 + 0.15 * np.sin(5.0 * xan + j) * np.cos(4.0 * yan - j), 0.05)
        warps.append(np.stack([xb, yb], axis=-1))
        certs.append(cert)
    return warps, certs, xan, yan


@dataclasses.dataclass
class Scene:
    ref: int
    nbrs: list
    inputs: hb.ReferenceInputs           # CPU tensors
    displaced: np.ndarray                # (H, W) bool
    match: int


def make(ref: int, nbrs, H: int, W: int, match: int = 64, channels: int = 2, masks: bool = False, displaced=None) -> Scene:
    cams = cameras()
    warps, certs, xan, yan = fields(ref, nbrs, H, W, match, match, displaced)
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
    inside = np.zeros((H, W), bool)
    if displaced is not None:
        inside[displaced[0]:displaced[1], displaced[2]:displaced[3]] = True
    ri = hb.ReferenceInputs(ref_cam=ref, nbr_cams=list(nbrs), cert=tc, warp=tw, image=torch.from_numpy(render(cams[ref], match, match)),
                            mask_a=torch.from_numpy(mask_a) if masks else None, mask_b=mask_b if masks else None)
    return Scene(ref, list(nbrs), ri, inside, match)


def to_device(ri: hb.ReferenceInputs, dev) -> hb.ReferenceInputs:
    mv = lambda t: t.to(dev) if t is not None else None
    return dataclasses.replace(ri, cert=[mv(c) for c in ri.cert], warp=[mv(w) for w in ri.warp], image=mv(ri.image), mask_a=mv(ri.mask_a),
                               mask_b=[mv(m) for m in ri.mask_b] if ri.mask_b is not None else None)


# ---- the same scene for the driver: photographs on disk, a matcher that serves the analytic fields ---------------------------------------
def write_scene(root: str, pitched=None):
    """The rig's photographs at camera resolution under ``root``; returns camera records (``pitched`` as in ``cameras``) that name them."""
    from PIL import Image
    os.makedirs(root, exist_ok=True)
    out = []
    for i, (true, rec) in enumerate(zip(cameras(), cameras(pitched))):
        path = os.path.join(root, f"view_{i:04d}.png")
        if not os.path.exists(path):
            Image.fromarray(render(true, true.width, true.height)).save(path)
        out.append(dataclasses.replace(rec, image_path=path))
    return out


class Matcher(syn.SyntheticMatcher):
    """The analytic matcher of THIS scene: warps and certainties of ``fields`` on the preset's grid, whatever records the run was given."""

    def __init__(self, cams, setting="turbo", device="cpu", displaced=None):
        super().__init__(cams, setting=setting, device=device, channels=2)
        self.displaced = displaced

    def fields(self, ref, nbrs):
        key = (int(ref), tuple(int(n) for n in nbrs))
        hit = self.table.get(key)
        if hit is None:
            warps, certs, _x, _y = fields(key[0], list(key[1]), self.H, self.W, self.w_resized, self.h_resized, self.displaced)
            hit = [(torch.from_numpy(w.astype(np.float32)).contiguous().to(self.device), torch.from_numpy(c.astype(np.float32)).contiguous().to(self.device))
                   for w, c in zip(warps, certs)]
            self.table[key] = hit
        return key, [(w, c.clone()) for w, c in hit]
