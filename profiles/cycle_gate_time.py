#!/usr/bin/env python3
"""The forward-backward gate on one GPU (lfd_cycle_gate, csrc/lfd_cycle.hip) against the same operation written in torch - grid_sample(border) of
the backward warp at the forward warp, the pixel conversion, the comparison, ``where`` - at the grids of the RoMa presets with 1, 3 and 8 pairs
per launch, and ``dense_init`` end to end on the 185-camera synthetic scene with the filter off and at 1 px.  What profiles/r8/cycle_gate.txt records.

    python profiles/cycle_gate_time.py                       # both parts (needs the GPU)
    python profiles/cycle_gate_time.py --resources           # registers / occupancy of the kernels from the compiler (needs hipcc only)
    python profiles/cycle_gate_time.py --parent-tree DIR     # also time dense_init (filter off) of another checkout of this repository, built

Method, operator: both forms in this one process, every shape warmed first, then ``--passes`` passes that ALTERNATE the two; a pass times a group
of back-to-back calls between two device events and divides by the group's size.  The kernel is timed through the C entry point with its
arguments built once ("launch") and through ``HipDensifier.cycle_gate`` ("call": + the binding's checks).  Reported: the median pass, the lowest
and highest one as the spread, and 24 bytes x cells (certainty 4, warp_AB 8, warp_BA 8, store 4) over the launch time as a share of 8 TB/s - an
HBM share in name: at the small shapes the planes sit in the Infinity Cache and the time is the dispatch, not the memory.
The torch form is given its best layout (warp_BA already channel-first and contiguous, the pairs stacked) outside the timed region.
Method, end to end: ``densify.dense_init`` down to the written PLY with the analytic matcher (fields precomputed, no latency), ``--e2e-passes``
passes that alternate filter off / 1 px per mode after one warm-up run each.
NOT measurable here: what forcing the backward pass costs in the presets turbo / fast / base - it needs the model's weights."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HBM_PEAK = 8.0e12
SIDES = (320, 512, 960, 1280)
PAIRS = (1, 3, 8)


def fields(syn, cams, side, k, dev):
    nbrs = syn.ring_neighbours(len(cams), 10, k)
    wm = min(side, 800)
    kw = dict(noise_px=0.5, outlier_frac=0.05, occlusion_steps=True, device=dev)
    s = syn.synth_reference(cams, 10, nbrs, side, side, wm, wm, **kw)
    back = [syn.synth_reference(cams, n, [10], side, side, wm, wm, **kw).warp[0].contiguous() for n in nbrs]
    return [s.cert[j].contiguous() for j in range(k)], [s.warp[j].contiguous() for j in range(k)], back, wm


def torch_gate(cert, wab, wba_nchw, ax, ay, half_wm1, half_hm1, th, tau2):
    import torch
    import torch.nn.functional as F
    back = F.grid_sample(wba_nchw, wab, mode="bilinear", padding_mode="border", align_corners=False)
    dx = (back[:, 0] - ax) * half_wm1
    dy = (back[:, 1] - ay) * half_hm1
    keep = (wab.abs() <= 1.0).all(dim=-1) & (dx * dx + dy * dy <= tau2)
    return torch.where(keep, cert.clamp_min(th), torch.zeros((), device=cert.device))


def timed(fn, group):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(group):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / group          # microseconds


def operator_part(passes, out):
    import torch
    from lichtfeld_densification_plugin_amd import synthetic as syn
    from lichtfeld_densification_plugin_amd.core import hip_backend as hb
    dev = torch.device("cuda:0")
    dens = hb.HipDensifier(dev)
    lib = hb.load_library()
    cams = syn.ring_cameras(185)
    out("side  k   launch us (lo..hi)     HBM share   call us   torch us (lo..hi)      torch / launch   faster beyond the spread")
    verdict = True
    for side in SIDES:
        for k in PAIRS:
            cert, wab, wba, wm = fields(syn, cams, side, k, dev)
            outs = [torch.empty_like(c) for c in cert]
            tab = lambda ts: (C.c_void_p * k)(*[t.data_ptr() for t in ts])
            args = (dens._ctx, k, tab(cert), tab(wab), tab(wba), side, side, 2, side, side, None, None, wm, wm, C.c_float(0.2), C.c_float(1.0), tab(outs), None, None)
            launch = lambda: lib.lfd_cycle_gate(*args)
            call = lambda: dens.cycle_gate(cert, wab, wba, wm, wm, 0.2, 1.0)
            cs, ws, bs = torch.stack(cert), torch.stack(wab), torch.stack(wba).permute(0, 3, 1, 2).contiguous()
            ax = torch.from_numpy(hb.identity_axis(side)).to(dev).view(1, 1, side)
            ay = torch.from_numpy(hb.identity_axis(side)).to(dev).view(1, side, 1)
            form = lambda: torch_gate(cs, ws, bs, ax, ay, 0.5 * (wm - 1), 0.5 * (wm - 1), 0.2, 1.0)
            assert launch() == 0
            same = float((form() == outs_stack(outs)).float().mean())
            group = 200 if side <= 512 else 50
            for fn in (launch, call, form):
                timed(fn, group)
            t_l, t_c, t_t = [], [], []
            for _ in range(passes):
                t_l.append(timed(launch, group))
                t_t.append(timed(form, group))
                t_c.append(timed(call, group))
            med = lambda v: float(np.median(v))
            share = 24.0 * k * side * side / (med(t_l) * 1e-6) / HBM_PEAK
            clear = max(t_l) < min(t_t)
            verdict &= clear
            out(f"{side:5d} {k:2d}   {med(t_l):8.1f} ({min(t_l):.1f}..{max(t_l):.1f})   {100 * share:6.1f} %   {med(t_c):8.1f}   {med(t_t):8.1f} ({min(t_t):.1f}..{max(t_t):.1f})"
                f"   {med(t_t) / med(t_l):6.1f} x        {'yes' if clear else 'NO'}      (decisions equal to torch's: {100 * same:.3f} %)")
    out(f"kernel faster than the torch form at every shape by more than the spread of the passes: {'yes' if verdict else 'NO'}")
    dens.close()


def outs_stack(outs):
    import torch
    return torch.stack(outs)


def run_dense_init(scene_root, matcher, mode, tau):
    import torch
    from lichtfeld_densification_plugin_amd import densify
    name = f"cycle_{mode}.ply"
    argv = ["--scene_root", scene_root, "--images_subdir", "images_4", "--roma_setting", "fast", "--num_refs", "0.8", "--nns_per_ref", "3",
            "--matches_per_ref", "10000", "--reproj_thresh", "0.8", "--out_name", name, "--triangulation_mode", mode, "--device_image_prep"]
    if mode == "dense":
        argv += ["--refs_per_launch", "16", "--stream_output"]
    if tau > 0:
        argv += ["--cycle_thresh_px", str(tau)]
    args = densify.build_argparser().parse_args(argv)
    if hasattr(matcher, "set_backward_warp"):
        matcher.set_backward_warp(tau > 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = densify.dense_init(args, matcher=matcher)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert rc == 0
    path = os.path.join(scene_root, "sparse", "0", name)
    with open(path, "rb") as f:
        head = f.read(400).split(b"end_header")[0].decode()
    n = int([ln for ln in head.split("\n") if ln.startswith("element vertex")][0].split()[-1])
    os.remove(path)
    return dt, n


def e2e_part(passes, scene_root, taus, out):
    """dense_init on the 185-camera scene; every tau of ``taus`` per mode, alternating.  Returns {(mode, tau): [seconds]}."""
    import torch
    from lichtfeld_densification_plugin_amd import densify, synthetic
    dev = torch.device("cuda:0")
    synthetic.write_colmap_scene(scene_root, n_cams=185, images_subdir="images_4", fmt="jpg")
    plan = densify.build_argparser().parse_args(["--scene_root", scene_root, "--images_subdir", "images_4", "--num_refs", "0.8", "--nns_per_ref", "3"])
    records, refs, nn, _ = densify.plan_scene(plan)
    matcher = synthetic.SyntheticMatcher(records, setting="fast", device=dev, noise_px=0.5, outlier_frac=0.05, channels=2, seed=0)
    if hasattr(matcher, "set_backward_warp") and any(t > 0 for t in taus):
        matcher.set_backward_warp(True)
    matcher.precompute(refs, nn, 3)
    res = {}
    for mode in ("sampled", "dense"):
        for tau in taus:
            run_dense_init(scene_root, matcher, mode, tau)                 # warm-up
        for _ in range(passes):
            for tau in taus:
                dt, n = run_dense_init(scene_root, matcher, mode, tau)
                res.setdefault((mode, tau), []).append((dt, n))
        for tau in taus:
            v = [d for d, _n in res[(mode, tau)]]
            out(f"dense_init {mode:8s} filter {'off' if tau == 0 else f'{tau:g} px'}: median {np.median(v):.3f} s ({min(v):.3f}..{max(v):.3f}), "
                f"{len(refs)} references, {res[(mode, tau)][0][1]} points")
    return res


def resources(out):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "lichtfeld-densification-plugin_amd", "csrc"))
    import build as lfd_build
    with tempfile.TemporaryDirectory() as tmp:
        cmd = lfd_build.compile_command("lfd_cycle.hip", os.path.join(tmp, "c.o"), ["-Rpass-analysis=kernel-resource-usage"])
        err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    cur = None
    for ln in err.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = m.group(1)
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and cur and "lfd_cycle" in cur:
            out(f"{cur}: {m.group(1)} {m.group(2)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--e2e-passes", type=int, default=3)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--skip-operator", action="store_true")
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--parent-tree", type=str, default=None)
    ap.add_argument("--scene", type=str, default=None)
    ap.add_argument("--tree", type=str, default=os.path.dirname(HERE), help="(worker) the checkout whose package is imported")
    ap.add_argument("--worker", action="store_true", help="(worker) dense_init, filter off only; prints one JSON line")
    ap.add_argument("--out", type=str, default=os.path.join(HERE, "r8", "cycle_gate.txt"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    if a.resources:
        resources(out)
        return
    scene = a.scene or os.path.join(tempfile.gettempdir(), "lfd_cycle_scene")
    if a.worker:
        res = e2e_part(a.e2e_passes, scene, [0.0], lambda s: None)
        print(json.dumps({f"{m}": [d for d, _n in v] for (m, _t), v in res.items()}))
        return
    import torch
    out(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; passes {a.passes} (operator), {a.e2e_passes} (end to end)")
    if not a.skip_operator:
        operator_part(a.passes, out)
    if not a.skip_e2e:
        e2e_part(a.e2e_passes, scene, [0.0, 1.0], out)
        if a.parent_tree:
            env = dict(os.environ)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--tree", a.parent_tree, "--scene", scene, "--e2e-passes", str(a.e2e_passes)],
                               capture_output=True, text=True, env=env, timeout=900)
            if r.returncode != 0:
                out("parent tree: the worker failed: " + r.stderr[-400:])
            else:
                for mode, v in json.loads(r.stdout.strip().splitlines()[-1]).items():
                    out(f"dense_init {mode:8s} parent commit, filter absent: median {np.median(v):.3f} s ({min(v):.3f}..{max(v):.3f})")
    out("cost of the forced backward pass in turbo / fast / base: not measurable here (no model weights)")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
