"""What the tests of the precision-weighted re-triangulation share (tests/test_wrefine_*.py on the CPU, tests/test_gpu_wrefine.py on the device): the
probe scene of tests/support_scene.py with heteroscedastic matching noise (synthetic.synth_reference(noise_model="hetero")) and its TRUE precision
planes, the noise-free truth of a result's points, and plane tables for the exact properties."""
import dataclasses

import numpy as np
import torch

from lichtfeld_densification_plugin_amd import synthetic as syn
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

import refine_ref as rr
import support_scene as sc

THR = 0.8            # reproj_thresh of the two-view filter and of the acceptance test
SEED = 0


def reference_inputs(ref: int, k: int, H: int, W: int, channels: int = 2, masks: bool = False, device="cpu", noise_model: str = "hetero",
                     noise_px: float = 0.5, outlier_frac: float = 0.05, seed: int = SEED):
    """ReferenceInputs of one reference of the probe scene with its k ring neighbours and their precision planes (under "iid": I / noise_px^2 in
    match px^-2)."""
    nbrs = syn.ring_neighbours(sc.N_CAMS, ref, k)
    s = syn.synth_reference(sc.cameras(), ref, nbrs, H, W, sc.MATCH, sc.MATCH, noise_px=noise_px, outlier_frac=outlier_frac, channels=channels,
                            seed=seed, cert_mode="tiefree", device=device, noise_model=noise_model)
    if s.precision is not None:
        prec = [s.precision[j].clone() for j in range(k)]
    else:
        cams = sc.cameras()
        inv = 1.0 / max(noise_px, 1e-3) ** 2
        prec = []
        for n in nbrs:
            sx, sy = np.float32(cams[n].width / sc.MATCH), np.float32(cams[n].height / sc.MATCH)
            prec.append(torch.tensor([inv * sx * sx, 0.0, inv * sy * sy], dtype=torch.float32, device=device).expand(H, W, 3).contiguous())
    return hb.ReferenceInputs(ref_cam=ref, nbr_cams=nbrs, cert=[s.cert[j].clone() for j in range(k)], warp=[s.warp[j].clone() for j in range(k)],
                              image=s.image, mask_b=sc.masks_for(ref, nbrs, device) if masks else None, precision=prec)


def truth_of(ri, src, H: int, W: int, channels: int = 2) -> np.ndarray:
    """(n, 3) f64: the noise-free field of the reference triangulated in f64 at the result's (cell, slot)."""
    k = len(ri.nbr_cams)
    _s, clean = sc.reference_inputs(ri.ref_cam, k, H, W, channels=channels, noise_px=0.0, outlier_frac=0.0)
    return rr.two_view_f64(sc.cameras(), ri.ref_cam, ri.nbr_cams, [w.numpy() for w in clean.warp], sc.MATCH, sc.MATCH, src.cell.cpu().numpy(),
                           src.slot.cpu().numpy())


def with_planes(ri, planes):
    return dataclasses.replace(ri, precision=list(planes))


def filled(ri, values):
    """Every plane of ``ri`` filled with the three ``values``."""
    v = torch.tensor(values, dtype=torch.float32, device=ri.precision[0].device)
    return with_planes(ri, [v.expand(q.shape).contiguous() for q in ri.precision])


def to_device(ri, device):
    mv = lambda t: t.to(device) if t is not None else None
    return hb.ReferenceInputs(ref_cam=ri.ref_cam, nbr_cams=list(ri.nbr_cams), cert=[mv(c) for c in ri.cert], warp=[mv(w) for w in ri.warp],
                              image=mv(ri.image), mask_a=mv(ri.mask_a), mask_b=[mv(m) for m in ri.mask_b] if ri.mask_b is not None else None,
                              precision=[mv(q) for q in ri.precision] if ri.precision is not None else None)
