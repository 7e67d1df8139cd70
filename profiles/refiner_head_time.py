#!/usr/bin/env python3
"""The output head of RoMa-v2's refiners on one GPU: the fused call (lfd_refiner_head, csrc/lfd_head.hip, through core/refiner_head.py)
against what every ROCm user runs today - torch's f32 cast, two 1x1 convolutions, permutes, the warp update, softplus, the
Cholesky-to-precision conversion, stack, the padding of a 1-channel previous confidence and the last add - at the shapes of the model's three
conv refiners in the presets.  What profiles/r22/refiner_head.txt records.

    python profiles/refiner_head_time.py [--out profiles/r22/refiner_head.txt]     # timings, achieved bytes/s, the verdict per width (needs the GPU)
    python profiles/refiner_head_time.py --resources                               # registers / LDS / occupancy of the kernels (needs hipcc only)

Method: both in this one process on a bf16 ``z`` (what the ninth block returns), the previous state as planar memory behind permuted views
(what the model's interpolation hands over on the device), every shape warmed first, then ``--passes`` passes that ALTERNATE the candidates;
a pass times a group of back-to-back calls between two device events - the group sized from the warm-up so that a pass lasts about 20 ms -
and divides by the group's size.  Reported: the median pass, and the lowest and highest one as the spread.  "fused" is the tail as the shim
serves it (stream hand-over, cached head weights, the launch, two output allocations); "launch" is HipDensifier.refiner_head alone; "torch"
is the model's operator list on stand-in modules.  Achieved bytes/s: the bytes the launch has to touch - z once, the previous state once, the
outputs once - over the launch's time, against 8 TB/s.

The rule of DESIGN.md 4.20 (4.18's): the shim takes a width class only if "fused" is faster than "torch" at EVERY shape of that class here.
The share of a whole RoMa-v2 forward this tail takes is NOT measured here: it needs the model's weights.
"""
from __future__ import annotations

import argparse
import importlib.util
import math
import os
import re
import subprocess
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
# hidden width of the refiner (patch 4 / 2 / 1) -> the grid sides it runs at in the presets (match image side / patch)
SHAPES = {512: (128, 240, 320), 128: (256, 480, 640), 32: (512, 960, 1280)}
BATCHES = (1, 3)
PREV_DIMS = {512: (4, 1), 128: (4,), 32: (4,)}               # the patch-4 refiner receives the matcher's 1-channel confidence as well


def make_refiner(C, seed):
    """A stand-in with the attributes the shim's tail reads: the two 1x1 heads (seeded) and the configuration."""
    import torch
    from torch import nn
    torch.manual_seed(seed)
    r = nn.Module()
    r.warp_head, r.confidence_head = nn.Conv2d(C, 2, 1, 1, 0), nn.Conv2d(C, 4, 1, 1, 0)
    r.cfg = types.SimpleNamespace(warp_dim=2, confidence_dim=4, refine_init=4.0, channels_last=False, grid_sample_mode="bilinear")
    return r.cuda().eval().requires_grad_(False)


def torch_tail(r, z, prev_warp, prev_confidence):
    """The model's operator list behind the ninth block, on torch's own kernels."""
    import torch
    import torch.nn.functional as F
    z = z.float()
    B, _, H, W = z.shape
    displacement = r.warp_head(z).permute(0, 2, 3, 1).view(B, H, W, 2)
    delta = r.confidence_head(z).permute(0, 2, 3, 1).view(B, H, W, 4)
    warp = prev_warp + displacement / (r.cfg.refine_init * torch.tensor((W, H), device=z.device)[None, None, None])
    l00, l10, l11 = F.softplus(delta[..., 1]) + 1e-6, delta[..., 2], F.softplus(delta[..., 3]) + 1e-6
    delta = torch.stack([delta[..., 0], l00 * l00, l00 * l10, l10 * l10 + l11 * l11], dim=-1)
    if prev_confidence.shape[-1] == 4:
        return warp, prev_confidence + delta
    padded = torch.zeros_like(delta)
    padded[..., :1] = prev_confidence
    return warp, padded + delta


def timed(fn, group):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(group):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / group


def measure(passes, out_path):
    import torch
    from lichtfeld_densification_plugin_amd.core.refiner_head import FusedRefinerHead
    assert torch.cuda.is_available(), "refiner_head_time.py measures on the GPU"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    fh = open(out_path, "w")

    def say(line=""):
        print(line, flush=True)
        fh.write(line + "\n")
        fh.flush()

    dev = torch.device("cuda:0")
    shim = FusedRefinerHead()
    say(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; bf16 z, planar previous state; {passes} alternating passes per shape "
        f"after a warm-up of all; ms per call = median pass [lowest .. highest]")
    say("fused = the tail as core/refiner_head.py serves it (one launch); launch = HipDensifier.refiner_head alone; torch = the model's operator list "
        "behind the ninth block (f32 cast, two 1x1 convolutions, the element-wise chain)")
    verdict = {}
    for C, sides in SHAPES.items():
        r = make_refiner(C, seed=C)
        faster = []
        for side in sides:
            for B in BATCHES:
                for prev_dim in PREV_DIMS[C]:
                    g = torch.Generator(device="cuda").manual_seed(C + side + B)
                    z = torch.randn((B, C, side, side), generator=g, device=dev).to(torch.bfloat16)
                    pw = (torch.rand((B, 2, side, side), generator=g, device=dev) * 2 - 1).permute(0, 2, 3, 1)
                    pc = torch.randn((B, prev_dim, side, side), generator=g, device=dev).permute(0, 2, 3, 1)
                    with torch.inference_mode():
                        ctx = shim._context(dev)
                        ctx.set_stream(torch.cuda.current_stream(dev))
                        head = shim._head(r, C, dev)
                        fns = {"fused": lambda: shim.tail(r, z, pw, pc), "launch": lambda: ctx.refiner_head(z, head[0], head[1], pw, pc, 4.0),
                               "torch": lambda: torch_tail(r, z, pw, pc)}
                        ours, theirs = fns["fused"](), fns["torch"]()
                        diff = max(float((ours["warp"] - theirs[0]).abs().max()), float((ours["confidence"] - theirs[1]).abs().max()))
                        group = {}
                        for k, fn in fns.items():                              # warm-up, and the group size from it
                            timed(fn, 2)
                            group[k] = max(3, min(400, int(math.ceil(20.0 / max(timed(fn, 3), 1e-3)))))
                        t = {k: [] for k in fns}
                        for _ in range(passes):
                            for k, fn in fns.items():                          # alternating
                                t[k].append(timed(fn, group[k]))
                    med = {k: float(np.median(v)) for k, v in t.items()}
                    px = B * side * side
                    by = px * C * 2 + px * (2 + prev_dim) * 4 + px * 6 * 4
                    faster.append(med["fused"] < med["torch"])
                    say(f"C={C:<3} {side:>4}^2 B={B} prev {prev_dim}  fused {med['fused']:8.4f} [{min(t['fused']):8.4f} .. {max(t['fused']):8.4f}]  "
                        f"launch {med['launch']:8.4f} [{min(t['launch']):8.4f} .. {max(t['launch']):8.4f}]  "
                        f"torch {med['torch']:8.4f} [{min(t['torch']):8.4f} .. {max(t['torch']):8.4f}]  torch/fused {med['torch'] / med['fused']:6.2f}x "
                        f"(lowest torch / highest fused {min(t['torch']) / max(t['fused']):6.2f}x)  compulsory {by / 1e6:7.1f} MB -> launch "
                        f"{by / (med['launch'] * 1e-3) / 1e12:5.2f} TB/s = {by / (med['launch'] * 1e-3) / HBM_PEAK:5.3f} of HBM peak  "
                        f"max |fused - torch| {diff:.2e}")
                    del z, pw, pc, fns, ours, theirs
                    torch.cuda.empty_cache()
        verdict[C] = all(faster)
        del r
    shim.close()
    say()
    for C, ok in verdict.items():
        say(f"width {C}: fused faster than torch (median pass) at every shape above: {'yes - the shim takes it' if ok else 'NO - it stays with torch'}")
    fh.close()


def resources():
    """The compiler's resource report of csrc/lfd_head.hip for gfx950."""
    spec = importlib.util.spec_from_file_location("_lfd_build", os.path.join(ROOT, "lichtfeld-densification-plugin_amd", "csrc", "build.py"))
    bld = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bld)
    with tempfile.TemporaryDirectory(prefix="lfd_head_res_") as tmp:
        res = subprocess.run(bld.compile_command("lfd_head.hip", os.path.join(tmp, "lfd_head.o"), ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"]),
                             capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError(res.stderr)
    print("compiler resource report (gfx950, the build's flags; <z type, vector or element loads, pixels per lane>):")
    name, vals = None, {}
    for line in res.stderr.splitlines():
        m = re.search(r"remark: +(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        key, _, val = m.group(1).partition(": ")
        if key == "Function Name":
            name, vals = val, {}
        else:
            vals[key.strip()] = val
        if key.strip() == "LDS Size [bytes/block]":
            short = re.sub(r"_Z\d+(lfd_head_kernel)ILb(\d)ELb(\d)ELi(\d)EEv.*",
                           lambda g: f"{g.group(1)}<{'f32' if g.group(2) == '1' else 'bf16'}, {'vector' if g.group(3) == '1' else 'element'}, {g.group(4)}>", name)
            print(f"  {short:<40} VGPRs {vals['VGPRs']:>3}  AGPRs {vals['AGPRs']}  SGPRs {vals['TotalSGPRs']:>3}  scratch {vals['ScratchSize [bytes/lane]']} B/lane  "
                  f"spills {vals['SGPRs Spill']} SGPR {vals['VGPRs Spill']} VGPR  LDS {vals['LDS Size [bytes/block]']} B  "
                  f"occupancy {vals['Occupancy [waves/SIMD]']} waves/SIMD")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22", "refiner_head.txt"))
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        resources()
        return
    measure(a.passes, a.out)


if __name__ == "__main__":
    main()
