#!/usr/bin/env python3
"""RoMa-v2's local correlation on one GPU: the fused kernel (lfd_local_corr, csrc/lfd_corr.hip) against the formulation every ROCm user runs
today - grid_sample of the neighbour's features into a (C, h, w, K) tensor, product with the reference features, sum over C - at the shapes
of the model's two conv refiners in all five presets.  What profiles/r7/local_corr.txt records.

    python profiles/local_corr_time.py                  # timings, peak memory, achieved bytes/s (needs the GPU)
    python profiles/local_corr_time.py --resources      # registers / LDS / occupancy of the kernels from the compiler (needs hipcc only)
    python profiles/local_corr_time.py --trace          # three fused calls per shape only: the run to put under rocprofv3 --kernel-trace --stats

Method: both formulations in this one process, every shape warmed first, then ``--passes`` passes that ALTERNATE the two; a pass times a
group of back-to-back calls between two device events and divides by the group's size.  Reported: the median pass, and the lowest and highest
one as the spread.  Peak memory: torch.cuda.max_memory_allocated over one call, above what was allocated before it (the inputs).  Achieved
bytes/s: the bytes the operator has to touch - A, Bf, warp read once, out written once - over the time of the launch alone ("kernel"), against 8 TB/s.

The share of a whole RoMa-v2 forward this operator takes is NOT measured here: it needs the model's weights.
"""
from __future__ import annotations

import argparse
import importlib.util
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
# preset -> (low-resolution side, high-resolution side or None, both directions); the patch-4 refiner works at side / 4 with C = 192 and a
# 7 x 7 window, the patch-2 refiner at side / 2 with C = 48 and a 3 x 3 window
PRESETS = {"turbo": (320, None, False), "fast": (512, None, False), "base": (640, None, False), "high": (640, 960, True),
           "precise": (800, 1280, True)}
REFINERS = {"patch 4": (4, 192, 3), "patch 2": (2, 48, 1)}


def rows():
    """(preset, stage, refiner, C, h, r, calls per pair), and the distinct (C, h, r) among them."""
    out = []
    for preset, (lr, hr, bidir) in PRESETS.items():
        for stage, side in (("lr", lr), ("hr", hr)):
            if side is None:
                continue
            for name, (patch, C, r) in REFINERS.items():
                out.append((preset, stage, name, C, side // patch, r, 2 if bidir else 1))
    return out, sorted({(C, h, r) for _p, _s, _n, C, h, r, _c in out}, key=lambda t: (-t[0], t[1]))


def inputs(B, C, h, r, seed):
    """The tensors the model's wrapper builds: reference features / sqrt(C) as (B, N, C), the neighbour's channel-last, the warp = identity
    grid + N(0, 0.05) + the (2r + 1)^2 window at one-pixel spacing."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    f0 = torch.randn((B, C, h, h), generator=g, device="cuda")
    f1 = torch.randn((B, C, h, h), generator=g, device="cuda")
    axis = torch.linspace(-1 + 1 / h, 1 - 1 / h, h, device="cuda")
    grid = torch.stack([axis.view(1, h).expand(h, h), axis.view(h, 1).expand(h, h)], dim=-1)
    warp = grid[None] + 0.05 * torch.randn((B, h, h, 2), generator=g, device="cuda")
    side = 2 * r + 1
    off = torch.linspace(-2 * r / h, 2 * r / h, side, device="cuda")
    window = torch.stack([off.view(1, side).expand(side, side), off.view(side, 1).expand(side, side)], dim=-1).reshape(1, 1, 1, side * side, 2)
    return f0, f1, warp, window


def fused_call(dens, f0, f1, warp, window):
    B, C, h, _ = f0.shape
    a = f0.reshape(B, C, h * h).permute(0, 2, 1) / (C ** 0.5)
    bf = f1.permute(0, 2, 3, 1)
    wk = (warp[..., None, :] + window[0]).reshape(B, h * h, -1, 2)
    return dens.local_corr(a, bf, wk)                 # (B, N, K); the channel-last copies of a and bf are part of the call


def fused_kernel_only(dens, a, bf, wk):
    return dens.local_corr(a, bf, wk)


def torch_call(f0, f1, warp, window):
    """grid_sample + multiply + sum, one batch element at a time (a (C, h, w, K) tensor twice per element)."""
    import torch
    import torch.nn.functional as F
    B, C, h, _ = f0.shape
    K = window.shape[3]
    out = torch.empty((B, K, h, h), device=f0.device)
    for b in range(B):
        coords = (warp[b, :, :, None, :] + window[0, 0]).reshape(1, h, h * K, 2)
        sampled = F.grid_sample(f1[b:b + 1], coords, mode="bilinear", padding_mode="zeros", align_corners=False).reshape(C, h, h, K)
        out[b] = (f0[b, ..., None] / (C ** 0.5) * sampled).sum(dim=0).permute(2, 0, 1)
    return out


def timed(fn, group):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(group):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / group


def peak_of(fn):
    import torch
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def measure(passes, trace):
    import torch
    from lichtfeld_densification_plugin_amd.core import hip_backend as hb
    assert torch.cuda.is_available(), "local_corr_time.py measures on the GPU"
    dens = hb.HipDensifier(torch.device("cuda:0"))
    table, shapes = rows()
    print(f"device: {torch.cuda.get_device_name(0)}; {passes} alternating passes per shape after a warm-up of both; ms per call = median pass "
          f"[lowest .. highest]")
    print("fused = HipDensifier.local_corr on the model's permuted views (its channel-last copies of both feature tensors included); "
          "kernel = the same on channel-last inputs (the launch alone); torch = grid_sample + multiply + sum")
    results = {}
    for C, h, r in shapes:
        K = (2 * r + 1) ** 2
        for B in (1, 3):
            f0, f1, warp, window = inputs(B, C, h, r, seed=C + h + B)
            a = (f0.reshape(B, C, h * h).permute(0, 2, 1) / (C ** 0.5)).contiguous()
            bf = f1.permute(0, 2, 3, 1).contiguous()
            wk = (warp[..., None, :] + window[0]).reshape(B, h * h, K, 2).contiguous()
            fns = {"fused": lambda: fused_call(dens, f0, f1, warp, window), "kernel": lambda: fused_kernel_only(dens, a, bf, wk),
                   "torch": lambda: torch_call(f0, f1, warp, window)}
            if trace:                                                 # the whole fused call: the layout copies show next to the kernel
                for _ in range(3):
                    fns["fused"]()
                torch.cuda.synchronize()
                continue
            ref = fns["torch"]().reshape(B, K, h * h).permute(0, 2, 1)
            err = float((fns["fused"]() - ref).abs().max())
            group = {"fused": 20, "kernel": 20, "torch": 3}
            for k, fn in fns.items():
                timed(fn, 2)                                           # warm-up
            t = {k: [] for k in fns}
            for _ in range(passes):
                for k, fn in fns.items():                             # alternating
                    t[k].append(timed(fn, group[k]))
            peak = {k: peak_of(fns[k]) for k in ("fused", "torch")}
            by = 4 * (B * h * h * C * 2 + 3 * B * h * h * K)
            med = {k: float(np.median(v)) for k, v in t.items()}
            results[(C, h, r, B)] = med
            print(f"C={C:<3} h=w={h:<3} K={K:<2} B={B}  fused {med['fused']:8.3f} [{min(t['fused']):8.3f} .. {max(t['fused']):8.3f}]  "
                  f"kernel {med['kernel']:8.3f} [{min(t['kernel']):8.3f} .. {max(t['kernel']):8.3f}]  "
                  f"torch {med['torch']:9.3f} [{min(t['torch']):9.3f} .. {max(t['torch']):9.3f}]  torch/fused {med['torch'] / med['fused']:6.1f}x "
                  f"(lowest torch / highest fused {min(t['torch']) / max(t['fused']):6.1f}x)  peak MB fused {peak['fused'] / 2**20:8.1f} torch {peak['torch'] / 2**20:9.1f}  "
                  f"algorithmic {by / 1e6:7.1f} MB -> kernel {by / (med['kernel'] * 1e-3) / 1e12:5.2f} TB/s = {by / (med['kernel'] * 1e-3) / HBM_PEAK:5.3f} of HBM peak  "
                  f"max |fused - torch| {err:.2e}", flush=True)
            del f0, f1, warp, window, a, bf, wk, ref, fns
            torch.cuda.empty_cache()
    dens.close()
    if trace:
        return
    print("\nper preset (B = 1, ms per pair = calls per pair x ms per call, both refiners and stages):")
    for preset in PRESETS:
        fused = sum(c * results[(C, h, r, 1)]["fused"] for p, _s, _n, C, h, r, c in table if p == preset)
        eager = sum(c * results[(C, h, r, 1)]["torch"] for p, _s, _n, C, h, r, c in table if p == preset)
        parts = ", ".join(f"{s} {n} {h}x{h}" + (" x2" if c == 2 else "") for p, s, n, _C, h, _r, c in table if p == preset)
        print(f"  {preset:<8} fused {fused:8.3f} ms  torch {eager:9.3f} ms  ({eager / fused:5.1f}x)   [{parts}]")


def resources():
    """The compiler's resource report of csrc/lfd_corr.hip for gfx950."""
    spec = importlib.util.spec_from_file_location("_lfd_build", os.path.join(ROOT, "lichtfeld-densification-plugin_amd", "csrc", "build.py"))
    bld = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bld)
    with tempfile.TemporaryDirectory(prefix="lfd_corr_res_") as tmp:
        res = subprocess.run(bld.compile_command("lfd_corr.hip", os.path.join(tmp, "lfd_corr.o"), ["-Rpass-analysis=kernel-resource-usage"]),
                             capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError(res.stderr)
    print("compiler resource report (gfx950, the build's flags; vec<G, CPL>: G lanes per query pixel, CPL float4 of A per lane, 0 = re-read):")
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
            short = re.sub(r"_Z\d+(lfd_corr_\w+?kernel)(ILi(\d+)ELi(\d+)EEv)?.*", lambda g: g.group(1) + (f"<{g.group(3)}, {g.group(4)}>" if g.group(2) else ""), name)
            print(f"  {short:<28} VGPRs {vals['VGPRs']:>3}  AGPRs {vals['AGPRs']}  SGPRs {vals['TotalSGPRs']:>3}  scratch {vals['ScratchSize [bytes/lane]']} B/lane  "
                  f"LDS {vals['LDS Size [bytes/block]']} B  occupancy {vals['Occupancy [waves/SIMD]']} waves/SIMD")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        resources()
        return
    measure(a.passes, a.trace)


if __name__ == "__main__":
    main()
