"""Scenes of the tests of lfd_estimate_normals: surfaces whose normal is known, seen by cameras of ``synthetic.ring_cameras``,
with warps made by exact projection (f64, rounded to f32 once) and optional seeded iid matching noise.

The cameras have a long lens (focal 8000 px at 1297 x 840): the whole grid then sees a plane tilted 75 degrees to the reference's image at
moderate depths - with the default lens the plane would run away to infinity inside the image.

    plane    tilted ``tilt_deg`` about the image's x axis: z(dy) = d0 cos t / (cos t - dy sin t) along the ray (dx, dy, 1)
    crease   two planes tilted +40 and -40 degrees about the image's y axis, the nearer of the two along every ray
    slab     the fronto-parallel plane with the columns x >= W / 2 pulled forward to 0.65 of the depth
"""
import math

import numpy as np
import torch

import lichtfeld_densification_plugin_amd as lfd
from lichtfeld_densification_plugin_amd import synthetic as syn
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

N_CAMS = 40
FOCAL = 8000.0
W_MATCH, H_MATCH = 96, 80
THR = 0.8                      # reproj_thresh of the two-view test, of the points and of the window cells
SLAB = 0.65
# the noisy scene of the device-against-twin comparison (tests/test_gpu_normals.py) and of its CPU check (tests/test_normals_host.py): a plane
# tilted 40 degrees, 20 x 24 cells, matching noise far below THR and gross outliers ACROSS the epipolar lines - every decision is far from its
# threshold, the reference flags nothing.  IN_BAND: the outliers lie ALONG the epipolar lines instead - consistent points at other depths whose
# reprojection errors spread over THR: some decisions do fall in band there.
NOISY = dict(kind="plane", H=20, W=24, channels=2, tilt_deg=40.0, noise_px=0.1, outlier_frac=0.03, seed=0)
IN_BAND = dict(NOISY, outliers_along=True)
NOISY_STEP = 0.05
_cams = []


def cameras():
    if not _cams:
        _cams.extend(syn.ring_cameras(N_CAMS, focal=FOCAL))
    return _cams


def params(**kw):
    return hb.make_params(lfd.DensePipelineConfig(output_path="", reproj_thresh=THR, **kw))


def surface(kind: str, dx: np.ndarray, dy: np.ndarray, d0: float, tilt_deg: float = 0.0):
    """Depth z along the rays (dx, dy, 1) of the reference's camera frame and the unit normal there (camera frame, facing the camera)."""
    if kind in ("plane", "slab"):
        t = math.radians(tilt_deg if kind == "plane" else 0.0)
        z = d0 * math.cos(t) / (math.cos(t) - dy * math.sin(t))
        n = np.broadcast_to(np.array([0.0, math.sin(t), -math.cos(t)]), dx.shape + (3,)).copy()
        if kind == "slab":
            z = np.where(np.arange(dx.shape[1])[None, :] >= dx.shape[1] // 2, z * SLAB, z)
        return z, n
    if kind == "crease":
        t = math.radians(40.0)
        z1 = d0 * math.cos(t) / (math.cos(t) - dx * math.sin(t))
        z2 = d0 * math.cos(t) / (math.cos(t) + dx * math.sin(t))
        first = z1 <= z2
        n = np.where(first[..., None], np.array([math.sin(t), 0.0, -math.cos(t)]), np.array([-math.sin(t), 0.0, -math.cos(t)]))
        return np.where(first, z1, z2), n
    raise ValueError(kind)


def reference_inputs(kind: str, ref: int, k: int, H: int, W: int, channels: int = 2, tilt_deg: float = 0.0, noise_px: float = 0.0, seed: int = 0,
                     w_match: int = W_MATCH, h_match: int = H_MATCH, device="cpu", outlier_frac: float = 0.0, outliers_along: bool = False):
    """(ReferenceInputs, truth): one reference with its k ring neighbours looking at the surface; truth = dict of ``normal`` (H, W, 3) f64 world
    normal facing the reference, ``xyz`` (H, W, 3) f64 the surface point of every cell.  ``noise_px``: iid normal matching noise, camera px of
    the neighbour; ``outlier_frac``: that share of every neighbour's cells is moved by 5 .. 15 px as well - across the
    epipolar lines (gross mismatches, far beyond THR) or, ``outliers_along``, along them."""
    cams = cameras()
    cam = cams[ref]
    nbrs = syn.ring_neighbours(N_CAMS, ref, k)
    ax, ay = hb.identity_axis(W).astype(np.float64), hb.identity_axis(H).astype(np.float64)
    ua = (ax + 1.0) * 0.5 * (w_match - 1) * (cam.width / float(w_match))
    va = (ay + 1.0) * 0.5 * (h_match - 1) * (cam.height / float(h_match))
    K, R, C = cam.K.astype(np.float64), cam.R.astype(np.float64), cam.C.astype(np.float64)
    dx = np.broadcast_to(((ua - K[0, 2]) / K[0, 0])[None, :], (H, W))
    dy = np.broadcast_to(((va - K[1, 2]) / K[1, 1])[:, None], (H, W))
    z, n_c = surface(kind, dx, dy, float(np.linalg.norm(C)), tilt_deg)
    Xc = np.stack([dx * z, dy * z, z], axis=-1)
    Xw = Xc @ R + C                               # R^T X_c + C, row-vector form
    n_w = n_c @ R
    rng = np.random.RandomState(1000 * seed + ref)
    warps, certs = [], []
    cell = np.arange(H * W).reshape(H, W)
    for j, nb in enumerate(nbrs):
        cb = cams[nb]
        Kb, Rb, tb = cb.K.astype(np.float64), cb.R.astype(np.float64), cb.t.astype(np.float64).reshape(3)
        Xb = Xw @ Rb.T + tb
        ub = Kb[0, 0] * Xb[..., 0] / Xb[..., 2] + Kb[0, 2]
        vb = Kb[1, 1] * Xb[..., 1] / Xb[..., 2] + Kb[1, 2]
        if noise_px > 0.0:
            ub = ub + noise_px * rng.standard_normal((H, W))
            vb = vb + noise_px * rng.standard_normal((H, W))
        if outlier_frac > 0.0:
            out = rng.uniform(size=(H, W)) < outlier_frac
            # across the epipolar lines (the ring's are nearly horizontal): along them a mismatch is a consistent point at another depth
            shift = np.where(out, rng.uniform(5.0, 15.0, size=(H, W)) * rng.choice([-1.0, 1.0], size=(H, W)), 0.0)
            ub, vb = (ub + shift, vb) if outliers_along else (ub, vb + shift)
        xb = 2.0 * (ub / (cb.width / float(w_match))) / (w_match - 1) - 1.0
        yb = 2.0 * (vb / (cb.height / float(h_match))) / (h_match - 1) - 1.0
        chans = [xb, yb] if channels == 2 else [np.broadcast_to(ax[None, :], (H, W)), np.broadcast_to(ay[:, None], (H, W)), xb, yb]
        warps.append(torch.from_numpy(np.stack(chans, axis=-1).astype(np.float32)).to(device))
        # distinct certainties whose maximum moves from slot to slot over the grid: every slot wins somewhere
        certs.append(torch.from_numpy((0.3 + 0.5 * (((cell + 3 * j) % (k + 1)) + 0.1 * j) / (k + 1)).astype(np.float32)).to(device))
    ri = hb.ReferenceInputs(ref_cam=ref, nbr_cams=nbrs, cert=certs, warp=warps, image=syn.synth_image(h_match, w_match, ref, device))
    return ri, {"normal": n_w, "xyz": Xw}


def angle(a, b):
    """Angle (rad, f64) between the rows of two (n, 3) arrays, good down to 0 (atan2 of |a x b| and a . b)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), (a * b).sum(axis=-1))


def bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a
