"""A scene with a near field and a far field for the tests of the footprint-adaptive thinning: a ground plane z = 0 and a wall
x = 40, seen by twelve reference cameras 1.5 units above the ground that face +x, pitched from steeply down (ground at 2 - 4 units) to slightly
up (the wall at 40).  Every cell of a reference's 96 x 96 match grid triangulates the point where its centre's ray meets the ground or the wall.
Nothing here calls the library."""
import math

import numpy as np

GRID = 96
CAM_PX = 960
FOV_DEG = 60.0
WALL_X = 40.0
N_REFS = 12


def cameras(n_refs=N_REFS):
    """``[(R, t, C, fx, fy), ...]``: world-to-camera rotation (rows right, down, forward), translation, centre and focal lengths in pixels."""
    f_px = 0.5 * CAM_PX / math.tan(math.radians(0.5 * FOV_DEG))
    out = []
    for i in range(n_refs):
        pitch = math.radians(-62.0 + 70.0 * i / max(n_refs - 1, 1))          # -62 .. +8 degrees
        c, s = math.cos(pitch), math.sin(pitch)
        R = np.array([[0.0, -1.0, 0.0], [s, 0.0, -c], [c, 0.0, s]], np.float64)
        C = np.array([0.25 * i, -2.75 + 0.5 * i, 1.5], np.float64)
        out.append((R, -R @ C, C, f_px, f_px))
    return out


def build(n_refs=N_REFS, grid=GRID):
    """``(xyz, err, counts, rows, cams)``: the cloud (f32, reference after reference, cell after cell), a synthetic error, the points per
    reference, the five f64 of every reference as lfd_thin_footprint takes them, and the cameras."""
    cams = cameras(n_refs)
    rng = np.random.default_rng(5)
    centre = (np.arange(grid, dtype=np.float64) + 0.5) * (CAM_PX / grid)
    u, v = np.meshgrid(centre, centre)                                        # row-major cells: v is the row
    pts, rows = [], []
    for R, t, C, fx, fy in cams:
        d_cam = np.stack([(u.ravel() - 0.5 * CAM_PX) / fx, (v.ravel() - 0.5 * CAM_PX) / fy, np.ones(grid * grid)], axis=1)
        d = d_cam @ R                                                         # R^T d_cam per row
        with np.errstate(divide="ignore", invalid="ignore"):
            t_ground = np.where(d[:, 2] < 0.0, -C[2] / d[:, 2], np.inf)
            t_wall = np.where(d[:, 0] > 0.0, (WALL_X - C[0]) / d[:, 0], np.inf)
        depth = np.minimum(t_ground, t_wall)
        assert np.isfinite(depth).all()
        pts.append(C[None, :] + depth[:, None] * d)
        rows.append([R[2, 0], R[2, 1], R[2, 2], t[2], max(CAM_PX / (fx * grid), CAM_PX / (fy * grid))])
    xyz = np.concatenate(pts).astype(np.float32)
    err = rng.uniform(0.0, 1.0, xyz.shape[0]).astype(np.float32)
    return xyz, err, np.full(n_refs, grid * grid, np.int64), np.asarray(rows, np.float64), cams


def retention(xyz, counts, cams, keep, grid=GRID):
    """Per reference, the fraction of the grid cells its own points occupy that still hold any kept point of the cloud (projected into that
    reference's camera, in front of it)."""
    kept = xyz[np.asarray(keep, np.int64)].astype(np.float64)
    offs = np.concatenate([[0], np.cumsum(counts)])
    out = []
    for r, (R, t, _C, fx, fy) in enumerate(cams):
        def cells_of(p):
            pc = p @ R.T + t
            z = pc[:, 2]
            ok = z > 0
            with np.errstate(divide="ignore", invalid="ignore"):
                cu = np.floor((pc[:, 0] / z * fx + 0.5 * CAM_PX) / (CAM_PX / grid))
                cv = np.floor((pc[:, 1] / z * fy + 0.5 * CAM_PX) / (CAM_PX / grid))
            ok &= (cu >= 0) & (cu < grid) & (cv >= 0) & (cv < grid)
            return np.unique((cv[ok] * grid + cu[ok]).astype(np.int64))
        own = cells_of(xyz[offs[r]:offs[r + 1]].astype(np.float64))
        have = cells_of(kept)
        out.append(np.intersect1d(own, have).size / max(own.size, 1))
    return np.asarray(out)


def voxel_first(xyz, voxel):
    """Uniform first-point voxel filter: the lowest input index of every occupied cell of side ``voxel`` (anchored at the minimum), ascending."""
    xyz = np.asarray(xyz, np.float64)
    q = np.floor((xyz - xyz.min(axis=0)) / voxel).astype(np.int64)
    span = q.max(axis=0) + 1
    _, first = np.unique((q[:, 0] * span[1] + q[:, 1]) * span[2] + q[:, 2], return_index=True)
    return np.sort(first)
