"""What the tests of the pose refinement share (tests/test_pose_*.py on the CPU, tests/test_gpu_pose.py on the device): an analytic rig on
which the epipolar error fixes the poses up to the gauge.

On the audit's rig (tests/audit_scene.py: centres on a line, one orientation) the problem is degenerate.  Here eight cameras stand on an arc
that leaves every line and every plane - ``BASELINE`` apart along x, swinging in y and z - and each has an orientation of its own (a few
degrees of yaw, pitch and roll around "forward = +y").  The surfaces, textures and projections are the audit scene's: the GROUND z = -1 and
the WALL y = 6.  Warps are the exact projections of the surface point each grid cell of the reference sees, through the TRUE poses;
certainties are analytic.  Two more cameras, ``TWIN`` and ``TWIN2`` (indices ``N_CAMS`` and ``N_CAMS + 1``), stand at the world's origin
with orientations of their own - t = 0 in both records, so the pair's baseline is EXACTLY zero in the library's arithmetic: a pair with
coincident centres, for the degenerate case only; ``neighbours`` never names them.

Options: ``perturbed`` = (camera, rotation vector in degrees (3,), translation (3,)): that camera's RECORD gets R' = exp([w]x) R and the centre
c + translation while the warps stay those of the true poses - a wrong pose; ``noise_px`` adds seeded Gaussian noise to the neighbour's
observations; masks; 2- or 4-channel warps.  ``write_scene`` puts the photographs on disk, ``Matcher`` serves the analytic fields to the
driver."""
import dataclasses
import math
import os

import numpy as np
import torch

import audit_scene as asc
from lichtfeld_densification_plugin_amd import synthetic as syn
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from lichtfeld_densification_plugin_amd.core.types import CameraRecord

N_CAMS = 8
TWIN, TWIN2 = N_CAMS, N_CAMS + 1
BASELINE = 0.25
WIDTH, HEIGHT, FOCAL = asc.WIDTH, asc.HEIGHT, asc.FOCAL
_cams = {}


def _rot(axis: int, deg: float) -> np.ndarray:
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def rodrigues(w) -> np.ndarray:
    w = np.asarray(w, np.float64)
    th = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + math.sin(th) / th * K + (1.0 - math.cos(th)) / th ** 2 * (K @ K)


def true_pose(i: int):
    """(R, centre) f64 of camera ``i`` (``TWIN``, ``TWIN2``: at the origin)."""
    R0 = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])          # right = +x, down = -z, forward = +y
    c = np.array([BASELINE * i, 0.15 * math.sin(0.9 * i), 0.12 * math.cos(1.3 * i)]) if i < N_CAMS else np.zeros(3)
    R = _rot(2, 2.0 * math.sin(2.3 * i)) @ _rot(0, 3.0 * math.cos(1.1 * i)) @ _rot(1, 4.0 * math.sin(1.7 * i + 0.3)) @ R0
    return R, c


def cameras(perturbed=None):
    """The records the library is given: N_CAMS + 2 of them (the last two are ``TWIN`` and ``TWIN2``)."""
    key = None if perturbed is None else (int(perturbed[0]), tuple(float(v) for v in perturbed[1]), tuple(float(v) for v in perturbed[2]))
    if key not in _cams:
        K = np.array([[FOCAL, 0.0, WIDTH / 2.0 + 0.75], [0.0, FOCAL, HEIGHT / 2.0 - 0.5], [0.0, 0.0, 1.0]])
        out = []
        for i in range(N_CAMS + 2):
            R, c = true_pose(i)
            if key is not None and key[0] == i:
                R = rodrigues(np.radians(np.asarray(key[1]))) @ R
                c = c + np.asarray(key[2])
            out.append(CameraRecord.from_krt(i + 1, K, R, np.zeros(3) if i >= N_CAMS else -R @ c, WIDTH, HEIGHT, image_path=f"pose/{i:04d}.png"))
        _cams[key] = out
    return _cams[key]


def neighbours(ref: int, k: int):
    """The k nearest cameras of the rig (the lower index on ties); never ``TWIN``."""
    return sorted((c for c in range(N_CAMS) if c != ref), key=lambda c: (abs(c - ref), c))[:k]


def fields(ref: int, nbrs, H: int, W: int, match_w: int, match_h: int, noise_px: float = 0.0, seed: int = 0):
    """The analytic warps (H, W, 2) f64 and certainties (H, W) f64 of reference ``ref`` towards ``nbrs`` through the TRUE poses, and the
    reference's A-coordinates (xan, yan) (H, W)."""
    cams = cameras()
    camA = cams[ref]
    ax = syn.identity_axis_torch(W, "cpu").numpy().astype(np.float64)
    ay = syn.identity_axis_torch(H, "cpu").numpy().astype(np.float64)
    xan, yan = np.meshgrid(ax, ay)
    xA, yA = (xan + 1.0) * 0.5 * (match_w - 1), (yan + 1.0) * 0.5 * (match_h - 1)
    Xw, _wall = asc.surface(camA, xA, yA, match_w, match_h)
    warps, certs = [], []
    for j, nb in enumerate(nbrs):
        xb, yb, z = asc.project(cams[nb], Xw, match_w, match_h)
        if noise_px > 0.0:
            rng = np.random.default_rng([seed, ref, nb])                # (by pair, whatever the slot)
            xb = xb + rng.normal(0.0, noise_px, xb.shape) / (cams[nb].width / float(match_w)) / (0.5 * (match_w - 1))
            yb = yb + rng.normal(0.0, noise_px, yb.shape) / (cams[nb].height / float(match_h)) / (0.5 * (match_h - 1))
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
    match: int


def make(ref: int, nbrs, H: int, W: int, match: int = 64, channels: int = 2, masks: bool = False, noise_px: float = 0.0, match_h=None) -> Scene:
    """``match``: the match size (its width, with ``match_h`` its height: the driver's presets are not square)."""
    cams = cameras()
    match_h = match if match_h is None else int(match_h)
    warps, certs, xan, yan = fields(ref, nbrs, H, W, match, match_h, noise_px)
    tw, tc, mask_b = [], [], []
    for j in range(len(nbrs)):
        wp = warps[j]
        if channels == 4:
            wp = np.concatenate([np.stack([xan, yan], axis=-1), wp], axis=-1)
        tw.append(torch.from_numpy(wp.astype(np.float32)).contiguous())
        tc.append(torch.from_numpy(certs[j].astype(np.float32)).contiguous())
        m = np.ones((match_h, match), np.uint8)
        a = (match // 8) * (1 + j % 5)
        m[:, a:a + match // 10] = 0
        mask_b.append(torch.from_numpy(m))
    mask_a = np.ones((match_h, match), np.uint8)
    mask_a[match_h // 6:match_h // 6 + match_h // 12, :] = 0
    ri = hb.ReferenceInputs(ref_cam=ref, nbr_cams=list(nbrs), cert=tc, warp=tw, image=torch.from_numpy(asc.render(cams[ref], match, match_h)),
                            mask_a=torch.from_numpy(mask_a) if masks else None, mask_b=mask_b if masks else None)
    return Scene(ref, list(nbrs), ri, match)


to_device = asc.to_device
TABLE_WRONG = (2, (0.3, -0.2, 0.25), (0.01, -0.02, 0.015))       # the records of the table tests: camera 2 off in all six parameters
_made = {}


def batch_case(H: int, W: int, k: int, channels: int, masks: bool, poisoned: bool, cert: float = 0.5):
    """Three references with k, k - 1 (at least 1) and k neighbours drawn (with repetition) from the rig's other cameras, their observations
    0.7 px noisy - what the table tests of the twin and of the device share, against the records ``cameras(TABLE_WRONG)``: residuals of
    both signs in every pair, some of them outliers.  ``poisoned``: every kind of entry the rule singles out - NaN certainties, a certainty exactly at
    the threshold ``cert``, NaN and infinite observations, targets outside the neighbour - and the first reference is
    ``TWIN`` (with camera 0's neighbours) whose last neighbour is ``TWIN2`` at the same centre: every sample of that pair is degenerate."""
    key = (H, W, k, channels, masks, poisoned, cert)
    if key not in _made:
        refs = []
        for r, n in ((1, k), (4, max(1, k - 1)), (2, k)):
            near = neighbours(0 if poisoned and r == 1 else r, 5)
            nbrs = [near[j % 5] for j in range(n)]
            if poisoned and r == 1:
                r, nbrs[-1] = TWIN, TWIN2
            ri = make(r, nbrs, H, W, match=64, channels=channels, masks=masks, noise_px=0.7).inputs
            if poisoned:
                c, w = [t.clone() for t in ri.cert], [t.clone() for t in ri.warp]
                c[0][2, 3:9] = float("nan")
                c[0][6, 1:15] = cert
                w[0][3, 5:11, -2] = float("nan")
                w[-1][4, 7:13, -1] = float("inf")
                w[0][5, 2:8, -2] = 1.5
                ri = dataclasses.replace(ri, cert=c, warp=w)
            refs.append(ri)
        _made[key] = refs
    return _made[key]


EXACT_PX = 2.0


def exact_rig():
    """Two cameras and one reference on which the rule's arithmetic is exact, for a residual EXACTLY at pose_inlier_px = ``EXACT_PX``: R = I,
    centres (0, 0, 0) and (1, 0, 0), f = 64, principal point (32, 32), 65 x 65 px images matched at 65 x 65 (a camera px per match px, wm1 =
    64), four-channel warps whose coordinates are dyadic: the epipolar line of (ua, va) is the row va, d = 1 / 64 and num = (vb - va) / 64
    without a rounding.  Grid row y holds va = 8 + y and vb = va + DELTAS[y].  Returns (records, ReferenceInputs, DELTAS)."""
    K = np.array([[64.0, 0.0, 32.0], [0.0, 64.0, 32.0], [0.0, 0.0, 1.0]])
    recs = [CameraRecord.from_krt(1 + i, K, np.eye(3), -np.array([float(i), 0.0, 0.0]), 65, 65, image_path=f"exact/{i}.png") for i in range(2)]
    deltas = [2.0, -2.0, 1.75, 2.0 - 2.0 ** -10, -2.0 + 2.0 ** -10, 2.0 + 2.0 ** -10, 0.0, 0.5]
    H, W = len(deltas), 8
    ua = np.tile(16.0 + 2.0 * np.arange(W), (H, 1))
    va = np.tile((8.0 + np.arange(H))[:, None], (1, W))
    vb = va + np.asarray(deltas)[:, None]
    ub = ua - 4.0
    norm = lambda px: px / 32.0 - 1.0                                   # noqa: E731  (exact: ((n + 1) * 0.5) * 64 = px)
    warp = torch.from_numpy(np.stack([norm(ua), norm(va), norm(ub), norm(vb)], axis=-1).astype(np.float32)).contiguous()
    ri = hb.ReferenceInputs(ref_cam=0, nbr_cams=[1], cert=[torch.full((H, W), 0.9)], warp=[warp], image=torch.zeros((65, 65, 3), dtype=torch.uint8),
                            mask_a=None, mask_b=None)
    return recs, ri, deltas


def rotation_angle_deg(R) -> float:
    """(atan2 of the skew part's length and the trace: an arc cosine alone loses a small angle in the rounding of the trace)"""
    s = 0.5 * math.sqrt((R[2, 1] - R[1, 2]) ** 2 + (R[0, 2] - R[2, 0]) ** 2 + (R[1, 0] - R[0, 1]) ** 2)
    return math.degrees(math.atan2(s, (float(np.trace(R)) - 1.0) / 2.0))


def worst_relative_rotation_deg(poses, pairs) -> float:
    """The largest angle between the relative rotation R_b R_a^T of ``poses`` {camera index: (R, t)} and the true one, over ``pairs``."""
    worst = 0.0
    for a, b in pairs:
        Ra, Rb = true_pose(a)[0], true_pose(b)[0]
        worst = max(worst, rotation_angle_deg((poses[b][0] @ poses[a][0].T) @ (Rb @ Ra.T).T))
    return worst


# ---- the same scene for the driver: photographs on disk, a matcher that serves the analytic fields ---------------------------------------
def write_scene(root: str, perturbed=None):
    """The rig's photographs (the N_CAMS cameras, without the two at the origin) under ``root``; returns camera records (``perturbed`` as in ``cameras``)."""
    from PIL import Image
    os.makedirs(root, exist_ok=True)
    out = []
    for i, (true, rec) in enumerate(zip(cameras()[:N_CAMS], cameras(perturbed)[:N_CAMS])):
        path = os.path.join(root, f"view_{i:04d}.png")
        if not os.path.exists(path):
            Image.fromarray(asc.render(true, true.width, true.height)).save(path)
        out.append(dataclasses.replace(rec, image_path=path))
    return out


def write_colmap(root: str, perturbed=None, images_subdir: str = "images"):
    """The rig as the CLI reads it: ``root/sparse/0/{cameras,images,points3D}.bin`` with the poses of ``cameras(perturbed)`` (one PINHOLE camera
    per view; 400 surface points with their tracks for the reference selection) and the photographs under ``root/<images_subdir>``.  Returns
    the records as ``densify.plan_scene`` will load them."""
    from lichtfeld_densification_plugin_amd.core import colmap_io as cio
    sparse = os.path.join(root, "sparse", "0")
    os.makedirs(sparse, exist_ok=True)
    recs = write_scene(os.path.join(root, images_subdir), perturbed)
    yy, xx = np.meshgrid(np.linspace(8.0, HEIGHT - 8.0, 20), np.linspace(8.0, WIDTH - 8.0, 20), indexing="ij")
    Xw, _wall = asc.surface(cameras()[N_CAMS // 2], xx.reshape(-1), yy.reshape(-1), WIDTH, HEIGHT)
    pts = {i + 1: (Xw[i], np.array([128, 128, 128], np.uint8), 0.5) for i in range(Xw.shape[0])}
    tracks = {pid: [] for pid in pts}
    cams_bin, imgs = [], []
    for i, (true, rec) in enumerate(zip(cameras()[:N_CAMS], recs)):
        K = np.asarray(rec.K, np.float64)
        cams_bin.append(cio.Camera(i + 1, "PINHOLE", rec.width, rec.height, [K[0, 0], K[1, 1], K[0, 2], K[1, 2]]))
        xb, yb, z = asc.project(true, Xw, WIDTH, HEIGHT)
        seen = (np.abs(xb) < 1.0) & (np.abs(yb) < 1.0) & (z > 0)
        ids = (np.flatnonzero(seen) + 1).astype(np.int64)
        for j, pid in enumerate(ids):
            tracks[int(pid)].append((i + 1, j))
        uv = np.stack([(xb[seen] + 1.0) * 0.5 * (WIDTH - 1), (yb[seen] + 1.0) * 0.5 * (HEIGHT - 1)], axis=1)
        imgs.append(cio.Image(i + 1, cio.quaternion_from_rotation(np.asarray(rec.R, np.float64)), np.asarray(rec.t, np.float64).reshape(3), i + 1,
                              os.path.basename(rec.image_path), uv, ids))
    cio.write_cameras_bin(os.path.join(sparse, "cameras.bin"), cams_bin)
    cio.write_images_bin(os.path.join(sparse, "images.bin"), imgs)
    cio.write_colmap_points3D_bin(os.path.join(sparse, "points3D.bin"), pts, tracks)
    return recs


class Matcher(syn.SyntheticMatcher):
    """The analytic matcher of THIS scene: warps and certainties of ``fields`` on the preset's grid, whatever records the run was given."""

    def __init__(self, cams, setting="turbo", device="cpu", noise_px: float = 0.0):
        super().__init__(cams, setting=setting, device=device, channels=2)
        self.noise = float(noise_px)

    def fields(self, ref, nbrs):
        key = (int(ref), tuple(int(n) for n in nbrs))
        hit = self.table.get(key)
        if hit is None:
            warps, certs, _x, _y = fields(key[0], list(key[1]), self.H, self.W, self.w_resized, self.h_resized, self.noise)
            hit = [(torch.from_numpy(w.astype(np.float32)).contiguous().to(self.device), torch.from_numpy(c.astype(np.float32)).contiguous().to(self.device))
                   for w, c in zip(warps, certs)]
            self.table[key] = hit
        return key, [(w, c.clone()) for w, c in hit]
