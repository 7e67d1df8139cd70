#!/usr/bin/env python3
"""The photo-consistency gate on one GPU (lfd_photo_gate, csrc/lfd_photo.hip): the time of the whole call - its own kernel plus the support
filter's scan and scatter - at window radius 1, 2 and 3 on the survivors of the bench's dense workload (64 references x 3 neighbours x 512^2,
match 512^2), beside two yardsticks on the same points in the same session: lfd_colour_multiview (mean) and the dense kernel's own launch;
then the same call on a sampled-mode result (one reference, 20 000 matches asked for).  The points are the dense launch's survivors on the
noisy probe scene (ring of 185 cameras, 0.5 px iid matching noise, 5 % outliers), the images synthetic textures: what the gate DECIDES here
means nothing, only what it costs.  What DESIGN.md 4.25 records.

    python profiles/photo_timing.py                   # needs the GPU; writes profiles/r27/photo.txt
    python profiles/photo_timing.py --resources       # registers / scratch / occupancy of the kernels from the compiler (needs hipcc only)

One GPU step: run it under a time limit of its own (``timeout -k 10 600 python ...``).

Method: every launch warmed first, then ``--passes`` passes that alternate the three radii, the colour launch and the dense launch; a pass
times a group of back-to-back calls through the C entry point (arguments built once, out of place so that every call reads the same input)
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
sys.path.insert(0, HERE)
from colour_timing import MATCH, N_REFS, SIDE, TAU, THR, references, timed       # noqa: E402  (the same workload, built by the same code)

MIN_NCC, MIN_TEXTURE = 0.8, 2.0


def dense_shape(passes, out):
    import torch
    import lichtfeld_densification_plugin_amd as lfd
    from lichtfeld_densification_plugin_amd import synthetic as syn
    from lichtfeld_densification_plugin_amd.core import hip_backend as hb
    k = 3
    dev = torch.device("cuda:0")
    dens = hb.HipDensifier(dev)
    lib = hb.load_library()
    cams = syn.ring_cameras(185)
    dens.upload_cameras(cams)
    params = hb.make_params(lfd.DensePipelineConfig(output_path="", reproj_thresh=THR))
    refs = references(cams, dev, k)
    batch = hb.PreparedBatch(refs, MATCH, MATCH)
    cap = N_REFS * SIDE * SIDE
    src, dst = hb.OutputBuffers(cap, N_REFS, k, dev), hb.OutputBuffers(cap, N_REFS, k, dev)
    tri = lambda: dens.launch_dense(batch, params, src)
    tri()
    dens.check_launches()
    n = int(src.ref_offsets[-1].item())
    rgb_out = torch.empty((cap, 3), device=dev)
    counters = torch.zeros(5, dtype=torch.int64, device=dev)

    def gate(R, cnt):
        args = (dens._ctx, C.byref(batch.c), C.byref(src.c), src.ref_offsets.data_ptr(), C.cast(batch.nbr_images, C.c_void_p), R, C.c_float(MIN_NCC),
                C.c_float(MIN_TEXTURE), C.byref(dst.c), dst.ref_offsets.data_ptr(), dst.seg_counts.data_ptr(), None, None, cnt)
        return lambda: lib.lfd_photo_gate(*args)

    colour_args = (dens._ctx, C.byref(batch.c), C.byref(src.c), src.ref_offsets.data_ptr(), C.cast(batch.nbr_images, C.c_void_p), C.c_float(TAU), 1,
                   rgb_out.data_ptr(), None, None)
    colour = lambda: lib.lfd_colour_multiview(*colour_args)
    out(f"# {N_REFS} references x {k} neighbours x {SIDE}^2, match {MATCH}^2: {n} dense survivors")
    for R in (1, 2, 3):
        counters.zero_()
        assert gate(R, counters.data_ptr())() == 0
        dens.check_launches()
        out(f"# R = {R}: points guarded / under half a window / untextured / consistent / refuted: {counters.cpu().tolist()}")
    calls = {f"gate R={R}": gate(R, None) for R in (1, 2, 3)}
    calls["colour mean"] = colour
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
    out(f"dense kernel (lfd_triangulate_dense): {med(t_dense):9.1f} us per launch of {N_REFS} references ({min(t_dense):.1f}..{max(t_dense):.1f})")
    out("call           us per call (lo..hi)          x dense kernel   x colour mean   us per reference")
    for key, v in times.items():
        out(f"{key:12s} {med(v):9.1f} ({min(v):.1f}..{max(v):.1f})   {med(v) / med(t_dense):14.3f} {med(v) / med(times['colour mean']):15.3f} {med(v) / N_REFS:12.2f}")
    # a sampled-mode result: one reference, through the binding (what the driver calls)
    one = hb.PreparedBatch(refs[:1], MATCH, MATCH)
    dens.seed_rng(7)
    res = dens.triangulate_sampled(one, params, 20000)
    out(f"# sampled mode: one reference, {res.count} points")
    into = hb.OutputBuffers(res.count, 1, k, dev)
    sampled = {f"gate R={R}": (lambda R=R: dens.photo_gate(one, res, R, MIN_NCC, MIN_TEXTURE, into=into)) for R in (1, 2, 3)}
    sampled["colour mean"] = lambda: dens.colour_multiview(one, res, TAU, "mean")
    t_s = {key: [] for key in sampled}
    for fn in sampled.values():
        timed(fn, 2)
    for _ in range(passes):
        for key, fn in sampled.items():
            t_s[key].append(timed(fn, group))
    out("sampled call   us per call through the binding, read-back of the counts included (lo..hi)")
    for key, v in t_s.items():
        out(f"{key:12s} {med(v):9.1f} ({min(v):.1f}..{max(v):.1f})")
    dens.close()


def resources(out):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "lichtfeld-densification-plugin_amd", "csrc"))
    import build as lfd_build
    with tempfile.TemporaryDirectory() as tmp:
        cmd = lfd_build.compile_command("lfd_photo.hip", os.path.join(tmp, "c.o"), ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"])
        err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    cur = None
    for ln in err.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = m.group(1)
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and cur and "photo" in cur:
            out(f"{cur}: {m.group(1)} {m.group(2)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--out", type=str, default=os.path.join(HERE, "r27", "photo.txt"))
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
    out(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; passes {a.passes}; min_ncc {MIN_NCC}, min_texture {MIN_TEXTURE}, "
        f"support_thresh_px {TAU}, reproj_thresh {THR}")
    dense_shape(a.passes, out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
