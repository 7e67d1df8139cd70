"""Clouds for the free-space filter's tests: ring-camera scenes whose references each saw the ground and emitted a few floaters, and the scene the
rule was prototyped on (two references fooled the same way, one fooled alone)."""
import numpy as np

import freespace_ref as fr
from lichtfeld_densification_plugin_amd import synthetic


def split(n, n_refs, rng, empty=()):
    """points per reference: a random composition of n, the references in `empty` with none"""
    live = np.asarray([g for g in range(n_refs) if g not in empty])
    ids = live[rng.integers(0, len(live), n)]
    return np.bincount(ids, minlength=n_refs).astype(np.int64)


def ring_cloud(n_refs, n, seed, empty=(), floaters=0.2, clustered=False):
    """(xyz [n, 3] f32, counts [n_refs], P, wh): ground points with a little depth noise, ``floaters`` of them lifted between the cameras and the
    ground, a few far outside every frustum or behind the cameras"""
    rng = np.random.default_rng(seed)
    cams = synthetic.ring_cameras(n_refs, seed=seed)
    P, wh = fr.cameras(cams)
    counts = split(n, n_refs, rng, empty)
    if clustered:
        centres = rng.uniform(-1.2, 1.2, (7, 2))
        xy = centres[rng.integers(0, 7, n)] + rng.normal(0.0, 0.05, (n, 2))
    else:
        xy = rng.uniform(-1.5, 1.5, (n, 2))
    z = rng.normal(0.0, 0.01, n)
    lift = rng.random(n) < floaters
    z = np.where(lift, rng.uniform(0.1, 1.5, n), z)
    xyz = np.column_stack([xy, z])
    far = rng.random(n) < 0.03
    xyz[far] = rng.uniform(-40.0, 40.0, (int(far.sum()), 3))
    return xyz.astype(np.float32), counts, P, wh


def prototype_scene(seed=0):
    """8 ring cameras; every reference samples the ground patch [-1, 1]^2 with a jittered 40 x 40 grid; references 0 and 1 both emit the same
    50-point floater patch at height 0.3 above (0.1, -0.2); reference 5 emits a lone 50-point patch at height 0.25 above (-0.3, 0.2).  Returns
    (xyz, counts, P, wh, is_floater, paired) with the floaters behind their reference's ground points.

    The extent of a patch is this scene's choice: a 25 mm square right beside the named point (offsets 0.005 .. 0.03 along x and y).  It is
    that small, and sits there, for the scene's own precondition (tests/test_freespace_host.py): the ground behind a floater at height 0.25
    is only 2 / (2 - 0.25) = 1.14 x as deep as the floater, and on a 96 x 62 plane the 3 x 3 window reaches up to two 13.5-pixel cells
    (2.6 % of the depth each) towards the camera, so "every depth of the window above 1.1 x the floater's" holds in three references only
    where the floater's ray meets the ground in the near part of a cell row of at least three cameras.  Around (-0.3, 0.2) that is the band
    0.004 <= y - 0.2 <= 0.036; a 0.1 square centred on the point leaves it (window minimum 1.086 x in the third-best reference).  The band
    follows from the cameras and the plane size alone - f64 geometry, nothing the filter computes."""
    rng = np.random.default_rng(seed)
    cams = synthetic.ring_cameras(8)
    P, wh = fr.cameras(cams)
    g = (np.arange(40) + 0.5) / 40.0 * 2.0 - 1.0
    gx, gy = np.meshgrid(g, g)
    patch = lambda cx, cy, hgt: np.column_stack([cx + rng.uniform(0.005, 0.03, 50), cy + rng.uniform(0.005, 0.03, 50), np.full(50, hgt)])   # noqa: E731
    pair, lone = patch(0.1, -0.2, 0.3), patch(-0.3, 0.2, 0.25)
    parts, counts, floater, paired = [], [], [], []
    for r in range(8):
        jit = rng.uniform(-0.4, 0.4, (1600, 2)) * (2.0 / 40.0)
        ground = np.column_stack([gx.reshape(-1) + jit[:, 0], gy.reshape(-1) + jit[:, 1], np.zeros(1600)])
        extra = pair if r in (0, 1) else lone if r == 5 else np.zeros((0, 3))
        parts += [ground, extra]
        counts.append(1600 + len(extra))
        floater += [np.zeros(1600, bool), np.ones(len(extra), bool)]
        paired += [np.zeros(1600, bool), np.full(len(extra), r in (0, 1))]
    return (np.concatenate(parts).astype(np.float32), np.asarray(counts, np.int64), P, wh, np.concatenate(floater), np.concatenate(paired))
