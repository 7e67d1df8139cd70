"""What the tests of the multi-view support filter share (tests/test_support_filter_*.py on the CPU, tests/test_gpu_support_filter.py on the
device): the probe scene of DESIGN.md 4.8 (a ring of 40 cameras, 512^2 match size, tie-free certainties, 0.5 px noise and 5 % outliers), batches
built from it, and the comparison of one filtered result with the f64 reference of tests/support_ref.py."""
import numpy as np
import torch

import lichtfeld_densification_plugin_amd as lfd
from lichtfeld_densification_plugin_amd import synthetic as syn
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

import support_ref

N_CAMS = 40
MATCH = 512
BAND_CAP = 0.005
_cams = []


def cameras():
    if not _cams:
        _cams.extend(syn.ring_cameras(N_CAMS))
    return _cams


def masks_for(ref: int, nbrs, device="cpu"):
    """A mask per neighbour that blanks a band of its image (another band for every neighbour), none for the reference."""
    out = []
    for j, _n in enumerate(nbrs):
        m = torch.ones((MATCH, MATCH), dtype=torch.uint8)
        a = 60 + 90 * (j % 4)
        m[:, a:a + 70] = 0
        m[a:a + 40, :] = 0
        out.append(m.to(device))
    return out


def reference_inputs(ref: int, k: int, H: int, W: int, channels: int = 2, masks: bool = False, device="cpu", noise_px: float = 0.5,
                     outlier_frac: float = 0.05, seed: int = 0):
    """(SyntheticReference, ReferenceInputs) of one reference of the probe scene with its k ring neighbours."""
    nbrs = syn.ring_neighbours(N_CAMS, ref, k)
    s = syn.synth_reference(cameras(), ref, nbrs, H, W, MATCH, MATCH, noise_px=noise_px, outlier_frac=outlier_frac, channels=channels, seed=seed,
                            cert_mode="tiefree", device=device)
    ri = hb.ReferenceInputs(ref_cam=ref, nbr_cams=nbrs, cert=[s.cert[j].clone() for j in range(k)],
                            warp=[s.warp[j].clone() for j in range(k)], image=s.image, mask_b=masks_for(ref, nbrs, device) if masks else None)
    return s, ri


def with_neighbour_images(ri, device="cpu"):
    """``ri`` with a match-size u8 image per neighbour (ReferenceInputs.nbr_images), what the photo-consistency gate samples: textures of the
    neighbours' own, unrelated to the warps - the gate then refutes some matches and lets others pass, and whoever is given the same images
    decides the same."""
    ri.nbr_images = [syn.synth_image(MATCH, MATCH, 7000 + int(n), device) for n in ri.nbr_cams]
    return ri


def params(**kw):
    return hb.make_params(lfd.DensePipelineConfig(output_path="", **kw))


def bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_points(a, b) -> bool:
    """Two TriangulationOutputs hold the same points, offsets and counts, bit for bit."""
    return (a.xyz.shape == b.xyz.shape and all(np.array_equal(bits(getattr(a, n)), bits(getattr(b, n))) for n in ("xyz", "rgb", "err", "cell", "slot"))
            and np.array_equal(a.ref_offsets, b.ref_offsets) and np.array_equal(a.seg_counts, b.seg_counts))


def check_is_stable_subset(src, res, support, min_support: int, k: int):
    """``res`` is ``src`` restricted to support >= min_support, in order, bit for bit; offsets and per-slot counts are the recount."""
    sup = support.cpu().numpy()
    keep = sup >= min_support
    for name in ("xyz", "rgb", "err", "cell", "slot"):
        assert np.array_equal(bits(getattr(res, name)), bits(getattr(src, name))[keep]), name
    off = np.asarray(src.ref_offsets)
    want = np.concatenate([[0], np.cumsum([int(keep[off[r]:off[r + 1]].sum()) for r in range(len(off) - 1)])])
    assert np.array_equal(np.asarray(res.ref_offsets), want)
    slot = src.slot.cpu().numpy()
    for r in range(len(off) - 1):
        recount = np.bincount(slot[off[r]:off[r + 1]][keep[off[r]:off[r + 1]]], minlength=k)[:k]
        assert np.array_equal(res.seg_counts[r], recount), (r, res.seg_counts[r], recount)


def against_reference(refs, src, support, tau: float):
    """Every reference of ``src`` (a collected result for the ReferenceInputs ``refs``) through tests/support_ref.py.  Returns (tests counted,
    tests in band, points whose support count differs from the reference's although none of their tests is in band)."""
    sup = support.cpu().numpy().astype(np.int64)
    off = np.asarray(src.ref_offsets)
    cell, slot, xyz = src.cell.cpu().numpy(), src.slot.cpu().numpy(), src.xyz.cpu().numpy()
    tests = in_band = wrong = 0
    for r, ri in enumerate(refs):
        a, b = int(off[r]), int(off[r + 1])
        ref = support_ref.reference(cameras(), ri.ref_cam, ri.nbr_cams, [c.cpu().numpy() for c in ri.cert], [w.cpu().numpy() for w in ri.warp],
                                    [m.cpu().numpy() if m is not None else None for m in ri.mask_b] if ri.mask_b is not None else None,
                                    MATCH, MATCH, cell[a:b], slot[a:b], xyz[a:b], tau)
        counted = ref["tested"] & ref["live"]
        tests += int(counted.sum())
        in_band += int((counted & ref["band"]).sum())
        wrong += int((ref["clean"] & (sup[a:b] != ref["support"])).sum())
        # a point with tests in band may differ from the reference by at most their number
        slack = (counted & ref["band"]).sum(axis=1)
        assert (np.abs(sup[a:b] - ref["support"]) <= slack).all()
    return tests, in_band, wrong


def on_host(refs):
    """The same ReferenceInputs with every tensor copied to the CPU (what the twin is given when the device is the other side of a comparison)."""
    cpu = lambda t: t.cpu() if t is not None else None
    return [hb.ReferenceInputs(ref_cam=r.ref_cam, nbr_cams=list(r.nbr_cams), cert=[cpu(c) for c in r.cert], warp=[cpu(w) for w in r.warp],
                               image=cpu(r.image), mask_a=cpu(r.mask_a), mask_b=[cpu(m) for m in r.mask_b] if r.mask_b is not None else None,
                               nbr_images=[cpu(m) for m in r.nbr_images] if r.nbr_images is not None else None)
            for r in refs]


def result_on_host(res):
    import dataclasses
    return dataclasses.replace(res, xyz=res.xyz.cpu(), rgb=res.rgb.cpu(), err=res.err.cpu(), cell=res.cell.cpu(), slot=res.slot.cpu(), _packed=None)
