#!/usr/bin/env python3
"""One conv block of RoMa-v2's refiners on one GPU: the fused call (lfd_refiner_block, csrc/lfd_block.hip, through core/refiner_blocks.py)
against what every ROCm user runs today - torch's depthwise convolution, BatchNorm, ReLU and 1x1 convolution under bf16 autocast - at the
shapes of the model's three conv refiners in the presets.  What profiles/r18/refiner_block.txt records.

    python profiles/refiner_block_time.py [--out profiles/r18/refiner_block.txt]     # timings, achieved bytes/s, the verdict per width (needs the GPU)
    python profiles/refiner_block_time.py --resources                                # registers / LDS / occupancy of the kernels (needs hipcc only)

Method: both in this one process on bf16 input (eight of a refiner's nine blocks receive the previous block's bf16 output), every shape
warmed first, then ``--passes`` passes that ALTERNATE the two; a pass times a group of back-to-back calls between two device events - the
group sized from the warm-up so that a pass lasts about 20 ms - and divides by the group's size.  Reported: the median pass, and the lowest
and highest one as the spread.  "fused" is the block as the shim serves it: ONE launch for width 32, the fused depthwise launch plus the
block's own 1x1 convolution under autocast for the other widths; "launch" is the HIP launch alone.  Achieved bytes/s: the bytes the launch has
to touch - the activation read once and written once, 2 x B C H W x 2 bytes - over the launch's time, against 8 TB/s.

The rule of DESIGN.md 4.18: the shim takes a width class only if "fused" is faster than "torch" at EVERY shape of that class here.
The share of a whole RoMa-v2 forward these blocks take is NOT measured here: it needs the model's weights.
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

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
# hidden width of the refiner (patch 4 / 2 / 1) -> the grid sides it runs at in the presets (match image side / patch)
SHAPES = {512: (128, 240, 320), 128: (256, 480, 640), 32: (512, 960, 1280)}
BATCHES = (1, 3)


def make_block(C, seed):
    """A stand-in for the model's block: the same four layers under bf16 autocast, seeded parameters, eval mode."""
    import torch
    from torch import nn

    class Block(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv_depthwise = nn.Conv2d(C, C, kernel_size=5, padding=2, groups=C)
            self.norm = nn.BatchNorm2d(C)
            self.relu = nn.ReLU(inplace=True)
            self.conv_pointwise = nn.Conv2d(C, C, 1, 1, 0)
            self.enable_amp = True

        def forward(self, x):
            with torch.autocast(device_type=x.device.type, enabled=self.enable_amp, dtype=torch.bfloat16):
                return self.conv_pointwise(self.relu(self.norm(self.conv_depthwise(x))))

    torch.manual_seed(seed)
    blk = Block()
    with torch.no_grad():
        blk.norm.running_var.uniform_(0.5, 2.0)
        blk.norm.running_mean.normal_(0.0, 0.2)
        blk.norm.weight.normal_(1.0, 0.2)
        blk.norm.bias.normal_(0.0, 0.2)
    return blk.cuda().eval().requires_grad_(False)


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
    from lichtfeld_densification_plugin_amd.core.refiner_blocks import FusedRefinerBlocks
    assert torch.cuda.is_available(), "refiner_block_time.py measures on the GPU"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    fh = open(out_path, "w")

    def say(line=""):
        print(line, flush=True)
        fh.write(line + "\n")
        fh.flush()

    dev = torch.device("cuda:0")
    shim = FusedRefinerBlocks()
    say(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; bf16 input; {passes} alternating passes per shape after a warm-up of "
        f"both; ms per call = median pass [lowest .. highest]")
    say("fused = the block as core/refiner_blocks.py serves it (width 32: one launch; other widths: the fused depthwise launch + the block's own "
        "1x1 convolution under autocast); launch = the HIP launch alone; torch = the block's own forward (four operators under bf16 autocast)")
    verdict = {}
    for C, sides in SHAPES.items():
        blk = make_block(C, seed=C)
        faster = []
        for side in sides:
            for B in BATCHES:
                g = torch.Generator(device="cuda").manual_seed(C + side + B)
                x = torch.randn((B, C, side, side), generator=g, device=dev).to(torch.bfloat16)
                with torch.inference_mode():
                    ctx = shim._context(dev)
                    ctx.set_stream(torch.cuda.current_stream(dev))
                    folded = shim._fold(blk, C, dev)
                    fns = {"fused": lambda: shim.forward(blk, x), "launch": lambda: ctx.refiner_block(x, *folded), "torch": lambda: blk(x)}
                    diff = float((fns["fused"]().float() - fns["torch"]().float()).abs().max())
                    group = {}
                    for k, fn in fns.items():                              # warm-up, and the group size from it
                        timed(fn, 2)
                        group[k] = max(3, min(200, int(math.ceil(20.0 / max(timed(fn, 3), 1e-3)))))
                    t = {k: [] for k in fns}
                    for _ in range(passes):
                        for k, fn in fns.items():                          # alternating
                            t[k].append(timed(fn, group[k]))
                med = {k: float(np.median(v)) for k, v in t.items()}
                by = 2 * B * C * side * side * 2
                faster.append(med["fused"] < med["torch"])
                say(f"C={C:<3} {side:>4}^2 B={B}  fused {med['fused']:8.3f} [{min(t['fused']):8.3f} .. {max(t['fused']):8.3f}]  "
                    f"launch {med['launch']:8.3f} [{min(t['launch']):8.3f} .. {max(t['launch']):8.3f}]  "
                    f"torch {med['torch']:8.3f} [{min(t['torch']):8.3f} .. {max(t['torch']):8.3f}]  torch/fused {med['torch'] / med['fused']:5.2f}x "
                    f"(lowest torch / highest fused {min(t['torch']) / max(t['fused']):5.2f}x)  compulsory {by / 1e6:7.1f} MB -> launch "
                    f"{by / (med['launch'] * 1e-3) / 1e12:5.2f} TB/s = {by / (med['launch'] * 1e-3) / HBM_PEAK:5.3f} of HBM peak  "
                    f"max |fused - torch| {diff:.3f}")
                del x, fns
                torch.cuda.empty_cache()
        verdict[C] = all(faster)
        del blk
    shim.close()
    say()
    for C, ok in verdict.items():
        say(f"width {C}: fused faster than torch (median pass) at every shape above: {'yes - the shim takes it' if ok else 'NO - it stays with torch'}")
    fh.close()


def resources():
    """The compiler's resource report of csrc/lfd_block.hip for gfx950."""
    spec = importlib.util.spec_from_file_location("_lfd_build", os.path.join(ROOT, "lichtfeld-densification-plugin_amd", "csrc", "build.py"))
    bld = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bld)
    with tempfile.TemporaryDirectory(prefix="lfd_block_res_") as tmp:
        res = subprocess.run(bld.compile_command("lfd_block.hip", os.path.join(tmp, "lfd_block.o"), ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"]),
                             capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError(res.stderr)
    print("compiler resource report (gfx950, the build's flags; <F32>: the input is f32 and rounded on load):")
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
            short = re.sub(r"_Z\d+(lfd_block_\w+?kernel)ILb(\d)EEv.*", lambda g: g.group(1) + ("<f32>" if g.group(2) == "1" else "<bf16>"), name)
            print(f"  {short:<28} VGPRs {vals['VGPRs']:>3}  AGPRs {vals['AGPRs']}  SGPRs {vals['TotalSGPRs']:>3}  scratch {vals['ScratchSize [bytes/lane]']} B/lane  "
                  f"spills {vals['SGPRs Spill']} SGPR {vals['VGPRs Spill']} VGPR  LDS {vals['LDS Size [bytes/block]']} B  "
                  f"occupancy {vals['Occupancy [waves/SIMD]']} waves/SIMD")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18", "refiner_block.txt"))
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        resources()
        return
    measure(a.passes, a.out)


if __name__ == "__main__":
    main()
