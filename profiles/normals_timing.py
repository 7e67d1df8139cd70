#!/usr/bin/env python3
"""The per-point normals on one GPU (lfd_estimate_normals, csrc/lfd_normals.hip): the kernel's time per reference at 512^2, k = 3, for the
radii 1 .. 4, in dense mode (every survivor of the dense launch: neighbouring lanes hold neighbouring cells) and in sampled mode (the
survivors of ~9000 cells per reference drawn at random from them, in cell order), beside the dense kernel's time on the same shape in the same
session; and the angular error of the normals on the noisy probe scene (ring of 185 cameras, 0.5 px iid matching noise, 5 % outliers) per
radius, against the normals the same routine gives at radius 1 on the noise-free scene.  What DESIGN.md 4.14 records.

    python profiles/normals_timing.py                   # needs the GPU
    python profiles/normals_timing.py --resources       # registers / occupancy of the kernels from the compiler (needs hipcc only)

One GPU step: run it under a time limit of its own (``timeout -k 10 600 python ...``).

Method: every launch warmed first, then ``--passes`` passes that alternate the four radii and the dense launch; a pass times a group of
back-to-back calls through the C entry point (arguments built once) between two device events and divides by the group's size.  Reported: the
median pass, the lowest and highest one as the spread."""
from __future__ import annotations

import argparse
import ctypes as C
import dataclasses
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N_REFS, K, SIDE, MATCH = 16, 3, 512, 512
THR, STEP = 0.8, 0.05
SAMPLED_CELLS = 9000


def timed(fn, group):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(group):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / group          # microseconds


def references(cams, dev, noise_px, outlier_frac):
    from lichtfeld_densification_plugin_amd import synthetic as syn
    from lichtfeld_densification_plugin_amd.core import hip_backend as hb
    refs = []
    for i in range(N_REFS):
        r = (10 + 2 * i) % 185
        nbrs = syn.ring_neighbours(185, r, K)
        s = syn.synth_reference(cams, r, nbrs, SIDE, SIDE, MATCH, MATCH, noise_px=noise_px, outlier_frac=outlier_frac, cert_mode="tiefree", device=dev)
        refs.append(hb.ReferenceInputs(ref_cam=r, nbr_cams=nbrs, cert=[s.cert[j].clone() for j in range(K)], warp=[s.warp[j].clone() for j in range(K)],
                                       image=s.image))
    return refs


def subsample(res, rng):
    """~SAMPLED_CELLS points per reference of a collected dense result, in their order: what a sampled run hands the stage."""
    import torch
    off = np.asarray(res.ref_offsets)
    keep, new_off = [], [0]
    for r in range(len(off) - 1):
        n = int(off[r + 1] - off[r])
        pick = np.sort(rng.choice(n, size=min(n, SAMPLED_CELLS), replace=False)) + int(off[r])
        keep.append(pick)
        new_off.append(new_off[-1] + pick.size)
    idx = torch.from_numpy(np.concatenate(keep)).to(res.xyz.device)
    return dataclasses.replace(res, xyz=res.xyz[idx].contiguous(), rgb=res.rgb[idx].contiguous(), err=res.err[idx].contiguous(),
                               cell=res.cell[idx].contiguous(), slot=res.slot[idx].contiguous(), ref_offsets=np.asarray(new_off, np.int64), _packed=None)


def gpu_part(passes, out):
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
    refs = references(cams, dev, 0.5, 0.05)
    batch = hb.PreparedBatch(refs, MATCH, MATCH)
    cap = N_REFS * SIDE * SIDE
    src = hb.OutputBuffers(cap, N_REFS, K, dev)
    tri = lambda: dens.launch_dense(batch, params, src)
    tri()
    dens.check_launches()
    res = src.collect()
    sampled = subsample(res, np.random.default_rng(0))
    out(f"# {N_REFS} references x {K} neighbours x {SIDE}^2, match {MATCH}^2: {res.count} dense survivors, {sampled.count} sampled points")
    normals = torch.empty((cap, 3), device=dev)

    def launcher(pts, offs, R):
        args = (dens._ctx, C.byref(batch.c), C.byref(pts), offs.data_ptr(), R, C.c_float(STEP), C.c_float(THR), normals.data_ptr(), None, None)
        return lambda: lib.lfd_estimate_normals(*args)

    s_off = torch.from_numpy(sampled.ref_offsets).to(dev)
    s_pts = hb.lfd_points(xyz=sampled.xyz.data_ptr(), rgb=None, err=None, cell=sampled.cell.data_ptr(), slot=sampled.slot.data_ptr(), capacity=sampled.count)
    calls = {("dense", R): launcher(src.c, src.ref_offsets, R) for R in (1, 2, 3, 4)}
    calls.update({("sampled", R): launcher(s_pts, s_off, R) for R in (1, 2, 3, 4)})
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
    out(f"dense kernel (lfd_triangulate_dense): {med(t_dense) / N_REFS:8.1f} us per reference ({min(t_dense) / N_REFS:.1f}..{max(t_dense) / N_REFS:.1f})")
    out("mode      R   kernel us per reference (lo..hi)    x dense kernel")
    for (mode, R), v in times.items():
        out(f"{mode:8s} {R:2d}   {med(v) / N_REFS:8.1f} ({min(v) / N_REFS:.1f}..{max(v) / N_REFS:.1f})   {med(v) / med(t_dense):18.2f}")
    # accuracy: the noisy scene's normals against the noise-free scene's at radius 1, cell by cell
    clean = hb.PreparedBatch(references(cams, dev, 0.0, 0.0), MATCH, MATCH)
    truth_pts = dens.triangulate_dense(clean, params)
    truth = dens.estimate_normals(clean, truth_pts, 1, STEP, THR).normals
    off = torch.from_numpy(np.asarray(truth_pts.ref_offsets)).to(dev)
    ref_of = torch.repeat_interleave(torch.arange(N_REFS, device=dev), off[1:] - off[:-1])
    table = torch.zeros((N_REFS * SIDE * SIDE, 3), device=dev)
    table[ref_of * SIDE * SIDE + truth_pts.cell.long()] = truth
    n_off = torch.from_numpy(np.asarray(res.ref_offsets)).to(dev)
    n_ref = torch.repeat_interleave(torch.arange(N_REFS, device=dev), n_off[1:] - n_off[:-1])
    want = table[n_ref * SIDE * SIDE + res.cell.long()]
    known = want.norm(dim=1) > 0.5
    out("R   fitted %   mean deg   median deg   (noisy probe scene, 0.5 px, 5 % outliers; fitted points with a noise-free normal)")
    for R in (1, 2, 3, 4):
        got, status = dens.estimate_normals(batch, res, R, STEP, THR, with_status=True)
        use = known & ((status & 0x80) != 0)
        a, b = got.normals[use].double(), want[use].double()
        ang = torch.rad2deg(torch.atan2(torch.cross(a, b, dim=1).norm(dim=1), (a * b).sum(1)))
        out(f"{R}   {100.0 * float(((status & 0x80) != 0).float().mean()):7.2f}   {float(ang.mean()):8.2f}   {float(ang.median()):10.2f}")
    dens.close()


def resources(out):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "lichtfeld-densification-plugin_amd", "csrc"))
    import build as lfd_build
    with tempfile.TemporaryDirectory() as tmp:
        cmd = lfd_build.compile_command("lfd_normals.hip", os.path.join(tmp, "c.o"), ["-Rpass-analysis=kernel-resource-usage"])
        err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    cur = None
    for ln in err.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = m.group(1)
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and cur and "normals" in cur:
            out(f"{cur}: {m.group(1)} {m.group(2)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--out", type=str, default=os.path.join(HERE, "normals_timing.txt"))
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
    out(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; passes {a.passes}; depth_step_rel {STEP}, reproj_thresh {THR}")
    gpu_part(a.passes, out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
