"""What the driver tests of the forward-backward filter share (tests/test_cycle_gate_driver.py on the host backend, tests/test_gpu_cycle_gate.py on
the device): a small generated scene on disk, the analytic matcher with clipped forward warps, and a recorder of the (cell, slot) pairs a run emits."""
import contextlib
import os

import numpy as np
import torch

import lichtfeld_densification_plugin_amd as lfd
from lichtfeld_densification_plugin_amd import densify, synthetic
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from lichtfeld_densification_plugin_amd.core import pipeline as pl


def make_scene(root: str, n_cams: int = 8):
    synthetic.write_colmap_scene(root, n_cams=n_cams, width=320, height=208, fmt="png")
    args = densify.build_argparser().parse_args(["--scene_root", root, "--images_subdir", "images_4", "--num_refs", "0.75", "--nns_per_ref", "3"])
    records, refs, nn, _ = densify.plan_scene(args)
    return dict(cams=records, refs=[int(r) for r in refs], nn=nn, root=root)


class ClippedMatcher(synthetic.SyntheticMatcher):
    """The analytic matcher with every forward coordinate inside [-0.99, 0.99]: no cell leaves the neighbour's image, so a gate with an enormous
    threshold rejects nothing."""

    def fields(self, ref, nbrs):
        key, vals = super().fields(ref, nbrs)
        out = []
        for v in vals:
            w = v[0].clone()
            w[..., -2:].clamp_(-0.99, 0.99)
            out.append((w,) + tuple(v[1:]))
        return key, out


def matcher_for(scene, device="cpu", clipped=False, **kw):
    cls = ClippedMatcher if clipped else synthetic.SyntheticMatcher
    return cls(scene["cams"], setting="turbo", device=device, channels=kw.pop("channels", 2), **kw)


@contextlib.contextmanager
def recorded_cells():
    """Every result a run collects from the kernels' (or the twin's) output buffers, reference by reference: a list of sets of (cell, slot)."""
    per_ref = []
    plain = hb.OutputBuffers.collect

    def collect(self, *a, **kw):
        res = plain(self, *a, **kw)
        if res.cell is not None and res.slot is not None:
            cell, slot, off = res.cell.cpu().numpy(), res.slot.cpu().numpy(), np.asarray(res.ref_offsets)
            for r in range(len(off) - 1):
                per_ref.append(set(zip(cell[off[r]:off[r + 1]].tolist(), slot[off[r]:off[r + 1]].tolist())))
        return res

    hb.OutputBuffers.collect = collect
    try:
        yield per_ref
    finally:
        hb.OutputBuffers.collect = plain


def run(scene, matcher, out_name, backend="host", device=None, **cfg_kw):
    exp = cfg_kw.pop("experimental", {})
    cfg = lfd.DensePipelineConfig(output_path=os.path.join(scene["root"], out_name), nns_per_ref=3, seed=3, viz_interval=0, matches_per_ref=2500,
                                  pack_workers=1, backend=backend, experimental=exp, **cfg_kw)
    kw = {"device": device} if device is not None else {}
    return pl.run_dense_pipeline(scene["cams"], scene["refs"], scene["nn"], cfg, matcher=matcher, **kw)


def same_cloud(a, b) -> bool:
    bits = lambda x: np.ascontiguousarray(x).view(np.uint32)
    return (a.xyz.shape == b.xyz.shape and np.array_equal(bits(a.xyz), bits(b.xyz)) and np.array_equal(bits(a.rgb), bits(b.rgb))
            and np.array_equal(bits(a.err), bits(b.err)) and np.array_equal(a.points_per_reference, b.points_per_reference))
