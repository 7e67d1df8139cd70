#!/usr/bin/env python3
"""The per-image exposure gains on one GPU (lfd_gain_accumulate / lfd_gain_apply, csrc/lfd_gain.hip): the statistics kernel's time at the
shape of profiles/colour_timing.py - 64 references x 3 neighbours x 512^2, match 512^2 - and at k = 8, beside lfd_colour_multiview's mean mode
on the same points in the same alternating passes (the gathers are the same, the reduction is new), and lfd_gain_apply beside a torch
multiply-and-clamp on the same tensor.  The points are the dense launch's survivors on the noisy probe scene (ring of 185 cameras, 0.5 px iid
matching noise, 5 % outliers), the neighbours' images synthetic textures.  What DESIGN.md 4.23 records.

    python profiles/gain_timing.py                   # needs the GPU; writes profiles/r25/gain.txt
    python profiles/gain_timing.py --resources       # registers / scratch / occupancy of the kernels from the compiler (needs hipcc only)

One GPU step: run it under a time limit of its own (``timeout -k 10 600 python ...``).

Method: every launch warmed first, then ``--passes`` passes that alternate the launches; a pass times a group of back-to-back calls through
the C entry point (arguments built once; the colour stage writes out of place, the statistics go to one table that is never read) between
two device events and divides by the group's size.  Reported: the median pass, the lowest and highest one as the spread."""
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
from colour_timing import N_REFS, SIDE, MATCH, THR, TAU, references, timed      # noqa: E402  (the same probe, the same timer)


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
    dens.launch_dense(batch, params, src)
    dens.check_launches()
    n = int(src.ref_offsets[-1].item())
    rgb_out = torch.empty((cap, 3), device=dev)
    table = torch.zeros((N_REFS * k, hb.GAIN_QUANTITIES), dtype=torch.int64, device=dev)
    images = C.cast(batch.nbr_images, C.c_void_p)
    colour_args = (dens._ctx, C.byref(batch.c), C.byref(src.c), src.ref_offsets.data_ptr(), images, C.c_float(TAU), 1, rgb_out.data_ptr(), None, None)
    gain_args = (dens._ctx, C.byref(batch.c), C.byref(src.c), src.ref_offsets.data_ptr(), images, C.c_float(TAU), table.data_ptr())
    calls = {"colour mean": lambda: lib.lfd_colour_multiview(*colour_args), "gain accumulate": lambda: lib.lfd_gain_accumulate(*gain_args)}
    for fn in calls.values():
        assert fn() == 0
    dens.check_launches()
    samples = int(table[:, 0].sum().item())
    out(f"# {N_REFS} references x {k} neighbours x {SIDE}^2, match {MATCH}^2: {n} dense survivors, {samples} samples in range "
        f"({samples / max(n, 1):.2f} per point) in {int((table[:, 0] > 0).sum().item())} of {N_REFS * k} rows")
    # the apply beside torch's multiply-and-clamp, on the survivors' colours
    rgb = src.rgb[:n]
    counts = (src.ref_offsets[1:] - src.ref_offsets[:-1]).cpu().numpy()
    factors = torch.linspace(0.8, 1.25, N_REFS * 3, device=dev).reshape(N_REFS, 3).contiguous()
    offs = src.ref_offsets
    apply_out = torch.empty((n, 3), device=dev)
    per_point = torch.repeat_interleave(factors, torch.as_tensor(counts, device=dev), dim=0)
    apply_args = (dens._ctx, rgb.data_ptr(), n, offs.data_ptr(), N_REFS, factors.data_ptr(), apply_out.data_ptr())
    calls["gain apply"] = lambda: lib.lfd_gain_apply(*apply_args)
    calls["torch mul + clamp"] = lambda: torch.clamp(torch.mul(rgb, per_point, out=apply_out), max=1.0, out=apply_out)
    assert calls["gain apply"]() == 0
    torch.cuda.synchronize()
    times = {key: [] for key in calls}
    group = 5
    for fn in calls.values():
        timed(fn, 2)
    for _ in range(passes):
        for key, fn in calls.items():
            times[key].append(timed(fn, group))
    med = lambda v: float(np.median(v))
    out(f"k = {k}  launch              us per launch (lo..hi)        x the line above")
    prev = None
    for key, v in times.items():
        ratio = f"{med(v) / prev:10.3f}" if (prev and key in ("gain accumulate", "torch mul + clamp")) else " " * 10
        out(f"k = {k}  {key:18s} {med(v):9.1f} ({min(v):.1f}..{max(v):.1f})   {ratio}")
        prev = med(v)
    dens.close()


def resources(out):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "lichtfeld-densification-plugin_amd", "csrc"))
    import build as lfd_build
    with tempfile.TemporaryDirectory() as tmp:
        cmd = lfd_build.compile_command("lfd_gain.hip", os.path.join(tmp, "g.o"), ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"])
        err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    cur = None
    for ln in err.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = m.group(1)
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and cur and "gain" in cur:
            out(f"{cur}: {m.group(1)} {m.group(2)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--out", type=str, default=os.path.join(HERE, "r25", "gain.txt"))
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
