"""What the tests of the gain compensation share beyond tests/colour_scene.py: a GROUP of cameras over that module's textured plane in which
every camera has ONE exposure gain - its rendering carries it wherever the camera appears, as a reference or as a neighbour - and every
camera is a reference with all the others as its neighbours.  Warps are the exact projections of the plane points the reference's grid
cells see, certainties distinct values in (0.2, 0.9)."""
import numpy as np
import torch

import colour_scene as cs
from lichtfeld_densification_plugin_amd import synthetic as syn
from lichtfeld_densification_plugin_amd.core import hip_backend as hb


def make_group(cam_ids, gains, H, W, match, channels: int = 2, seed: int = 0):
    """One cs.Scene per camera of ``cam_ids`` (the reference; the others, in the order given, are its neighbours); ``gains[i]`` is the
    exposure of camera ``cam_ids[i]``."""
    cams = cs.cameras()
    gain_of = {int(c): float(g) for c, g in zip(cam_ids, gains)}
    images = {c: cs.render(cams[c], match, gain_of[c]) for c in gain_of}
    ax = syn.identity_axis_torch(W, "cpu").numpy().astype(np.float64)
    ay = syn.identity_axis_torch(H, "cpu").numpy().astype(np.float64)
    xA, yA = np.meshgrid((ax + 1.0) * 0.5 * (match - 1), (ay + 1.0) * 0.5 * (match - 1))
    scenes = []
    for ref in cam_ids:
        nbrs = [int(c) for c in cam_ids if c != ref]
        rng = np.random.default_rng(1000 * seed + ref)
        X, Y = cs.plane_hits(cams[ref], xA, yA, match)
        Xw = np.stack([X, Y, np.zeros_like(X)], axis=-1)
        warps, certs = [], []
        for j, nb in enumerate(nbrs):
            cam = cams[nb]
            Xc = Xw @ np.asarray(cam.R, np.float64).T + np.asarray(cam.t, np.float64).reshape(3)
            u = cam.K[0, 0] * Xc[..., 0] / Xc[..., 2] + cam.K[0, 2]
            v = cam.K[1, 1] * Xc[..., 1] / Xc[..., 2] + cam.K[1, 2]
            wp = np.stack([u / (cam.width / float(match)) / (0.5 * (match - 1)) - 1.0, v / (cam.height / float(match)) / (0.5 * (match - 1)) - 1.0],
                          axis=-1)
            if channels == 4:
                wp = np.concatenate([np.stack(np.meshgrid(ax, ay), axis=-1), wp], axis=-1)
            warps.append(torch.from_numpy(wp.astype(np.float32)).contiguous())
            certs.append(torch.from_numpy((0.2 + 0.7 * (rng.permutation(H * W).reshape(H, W) + 0.5 + 0.1 * j) / (H * W)).astype(np.float32)))
        ri = hb.ReferenceInputs(ref_cam=int(ref), nbr_cams=nbrs, cert=certs, warp=warps, image=torch.from_numpy(images[ref]),
                                nbr_images=[torch.from_numpy(images[c]) for c in nbrs])
        scenes.append(cs.Scene(int(ref), nbrs, ri, [images[c] for c in nbrs], cs.albedo(X, Y), match, tuple(gain_of[c] for c in [ref] + nbrs)))
    return scenes
