#!/usr/bin/env python3
"""The multi-view colour on one GPU (lfd_colour_multiview, csrc/lfd_colour.hip): the kernel's time behind the dense kernel at the bench's shape
- 64 references x 3 neighbours x 512^2, match 512^2 - and at k = 8, in both modes, beside the dense kernel's own time on the same shape in the
same session.  The points are the dense launch's survivors on the noisy probe scene (ring of 185 cameras, 0.5 px iid matching noise, 5 %
outliers), the neighbours' images synthetic textures.  What DESIGN.md 4.21 records.

    python profiles/colour_timing.py                   # needs the GPU; writes profiles/r23/colour.txt
    python profiles/colour_timing.py --resources       # registers / scratch / occupancy of the kernels from the compiler (needs hipcc only)

One GPU step: run it under a time limit of its own (``timeout -k 10 600 python ...``).

Method: every launch warmed first, then ``--passes`` passes that alternate the two modes and the dense launch; a pass times a group of
back-to-back calls through the C entry point (arguments built once, colours written out of place so that every call reads the same input)
between two device events and divides by the group's size.  Reported: the median pass, the lowest and highest one as the spread."""
from __future__ import annotations

import argparse
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N_REFS, SIDE, MATCH = 64, 512, 512
THR, TAU = 0.8, 1.6


def timed(fn, group):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(group):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / group          # microseconds


def references(cams, dev, k):
    from lichtfeld_densification_plugin_amd import synthetic as syn
    from lichtfeld_densification_plugin_amd.core import hip_backend as hb
    images = {}
    refs = []
    for i in range(N_REFS):
        r = (10 + 2 * i) % 185
        nbrs = syn.ring_neighbours(185, r, k)
        s = syn.synth_reference(cams, r, nbrs, SIDE, SIDE, MATCH, MATCH, noise_px=0.5, outlier_frac=0.05, cert_mode="tiefree", device=dev)
        for n in nbrs:
            if n not in images:
                images[n] = syn.synth_image(MATCH, MATCH, n, dev)
        refs.append(hb.ReferenceInputs(ref_cam=r, nbr_cams=nbrs, cert=[s.cert[j].clone() for j in range(k)], warp=[s.warp[j].clone() for j in range(k)],
                                       image=s.image, nbr_images=[images[n] for n in nbrs]))
    return refs


def one_shape(k, passes, out):
    import torch
    import lichtfeld_densification_plugin_amd as lfd
    from lichtfeld_densification_plugin_amd import synthetic as syn
    from lichtfeld_densification_plugin_amd.core import hip_backend as hb
    dev = torch.device("cuda:0")
    dens = hb.HipDensifier(dev)
    lib = hb.load_library()
    cams = syn.ring_cameras(185)
    dens.upload_cameras(cams)
    params = hb.make_params(lfd.DensePipelineConfig(output_path="", reproj_thresh=THR))
    batch = hb.PreparedBatch(references(cams, dev, k), MATCH, MATCH)
    cap = N_REFS * SIDE * SIDE
    src = hb.OutputBuffers(cap, N_REFS, k, dev)
    tri = lambda: dens.launch_dense(batch, params, src)
    tri()
    dens.check_launches()
    n = int(src.ref_offsets[-1].item())
    rgb_out = torch.empty((cap, 3), device=dev)
    status = torch.zeros((cap,), dtype=torch.uint8, device=dev)

    def launcher(mode, st):
        args = (dens._ctx, C.byref(batch.c), C.byref(src.c), src.ref_offsets.data_ptr(), C.cast(batch.nbr_images, C.c_void_p), C.c_float(TAU), mode,
                rgb_out.data_ptr(), st, None)
        return lambda: lib.lfd_colour_multiview(*args)

    assert launcher(1, status.data_ptr())() == 0
    dens.check_launches()
    views = float(status[:n].float().mean().item())
    out(f"# {N_REFS} references x {k} neighbours x {SIDE}^2, match {MATCH}^2: {n} dense survivors, {views:.2f} views blended per point")
    calls = {"mean": launcher(1, None), "median": launcher(2, None)}
    for fn in calls.values():
        assert fn() == 0
    torch.cuda.synchronize()
    times = {key: [] for key in calls}
    t_dense = []
    group = 5
    for fn in list(calls.values()) + [tri]:
        timed(fn, 2)
    for _ in range(passes):
        for key, fn in calls.items():
            times[key].append(timed(fn, group))
        t_dense.append(timed(tri, group))
    med = lambda v: float(np.median(v))
    out(f"k = {k}  dense kernel (lfd_triangulate_dense): {med(t_dense):9.1f} us per launch of {N_REFS} references ({min(t_dense):.1f}..{max(t_dense):.1f})")
    out(f"k = {k}  mode     colour kernel us per launch (lo..hi)    x dense kernel    us per reference")
    for mode, v in times.items():
        out(f"k = {k}  {mode:7s} {med(v):9.1f} ({min(v):.1f}..{max(v):.1f})   {med(v) / med(t_dense):18.3f}   {med(v) / N_REFS:10.2f}")
    dens.close()


def resources(out):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "lichtfeld-densification-plugin_amd", "csrc"))
    import build as lfd_build
    with tempfile.TemporaryDirectory() as tmp:
        cmd = lfd_build.compile_command("lfd_colour.hip", os.path.join(tmp, "c.o"), ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"])
        err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    cur = None
    for ln in err.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = m.group(1)
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and cur and "colour" in cur:
            out(f"{cur}: {m.group(1)} {m.group(2)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--out", type=str, default=os.path.join(HERE, "r23", "colour.txt"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(HERE))
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    if a.resources:
        resources(out)
        return
    import torch
    out(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; passes {a.passes}; support_thresh_px {TAU}, reproj_thresh {THR}")
    for k in (3, 8):
        one_shape(k, a.passes, out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
