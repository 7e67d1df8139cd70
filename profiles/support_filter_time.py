#!/usr/bin/env python3
"""The multi-view support filter on one GPU (lfd_support_filter, csrc/lfd_support.hip) against the same operation written in torch - gathers of
the other neighbours' certainty and warp at the points' cells, the projection, the cross-multiplied comparison, boolean compaction - at the
survivor counts of the bench shapes, beside the lfd_triangulate_dense call it follows, and ``dense_init`` end to end on the 185-camera synthetic
scene with the filter off and at one supporter.  What profiles/r9/support_filter.txt records.

    python profiles/support_filter_time.py --skip-e2e        # the operator part (needs the GPU)
    python profiles/support_filter_time.py --skip-operator --append    # the end-to-end part, appended to the same file
    python profiles/support_filter_time.py --resources       # registers / occupancy of the kernels from the compiler (needs hipcc only)

Each part is one GPU step: run it under a time limit of its own (``timeout -k 10 600 python ...``) and chain the parts with ``&&``.

Method, operator: both forms in this one process, every shape warmed first, then ``--passes`` passes that ALTERNATE kernel, torch form and the
dense launch; a pass times a group of back-to-back calls between two device events and divides by the group's size.  The filter is timed through
the C entry point with its arguments built once (three launches: count, scan, scatter).  Reported: the median pass, the lowest and highest one as
the spread; the algorithmic bytes - per input point 17 (cell, slot, xyz) + 12 (k - 1) (certainty, warp pair of every other neighbour) + 1 + 1
(its support count written and read back), per survivor 16 more read (rgb, err) and 33 written - over the filter's time as a share of 8 TB/s;
and the filter's time as a share of the dense launch's.  The torch form is given its best case outside the timed region: the planes of all
references stacked, the projection matrices and pixel scales as tensors, every point's reference already known."""
from __future__ import annotations

import argparse
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HBM_PEAK = 8.0e12
# (label, references, neighbours, grid side, match side, source)
SHAPES = (("64 x 3 x 512^2 dense", 64, 3, 512, 512, "dense"), ("16 x 8 x 512^2 dense", 16, 8, 512, 512, "dense"),
          ("16 x 3 x 640^2 dense (high, 960^2 match)", 16, 3, 640, 960, "dense"), ("16 x 3 x 512^2 sampled chain, M = 10000", 16, 3, 512, 512, "chain"))
TAU, MIN_SUPPORT = 1.6, 1


def timed(fn, group):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(group):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / group          # microseconds


def torch_filter(cert, warp, P, sxy, wm1, hm1, xyz, rgb, err, cell, slot, ref, tau, m):
    """cert (R, k, HW), warp (R, k, HW, 2), P (R, k, 3, 4), sxy (R, k, 2); the points' arrays and their reference index."""
    import torch
    k = cert.shape[1]
    c = cert[ref, :, cell]                                           # (n, k)
    w = warp[ref, :, cell]                                           # (n, k, 2)
    Pp = P[ref]                                                      # (n, k, 3, 4)
    p = (Pp[..., :3] * xyz[:, None, None, :]).sum(-1) + Pp[..., 3]   # (n, k, 3)
    s = sxy[ref]
    ub = (w[..., 0] + 1.0) * 0.5 * wm1 * s[..., 0]
    vb = (w[..., 1] + 1.0) * 0.5 * hm1 * s[..., 1]
    pz = p[..., 2]
    du, dv = p[..., 0] - ub * pz, p[..., 1] - vb * pz
    t = tau * pz
    ok = (pz > 0) & (du * du + dv * dv <= t * t) & (c > 0) & (torch.arange(k, device=c.device)[None, :] != slot[:, None])
    keep = ok.sum(1) >= m
    return xyz[keep], rgb[keep], err[keep], cell[keep], slot[keep]


def operator_part(passes, out):
    import torch
    import lichtfeld_densification_plugin_amd as lfd
    from lichtfeld_densification_plugin_amd import synthetic as syn
    from lichtfeld_densification_plugin_amd.core import hip_backend as hb
    dev = torch.device("cuda:0")
    dens = hb.HipDensifier(dev)
    lib = hb.load_library()
    cams = syn.ring_cameras(185)
    dens.upload_cameras(cams)
    out("shape                                         points in    kept    filter us (lo..hi)     HBM share   torch us (lo..hi)    torch / filter   "
        "triangulation us   filter / triangulation")
    verdict = True
    for label, R, k, side, wm, source in SHAPES:
        refs = []
        for i in range(R):
            r = (10 + 2 * i) % 185
            nbrs = syn.ring_neighbours(185, r, k)
            s = syn.synth_reference(cams, r, nbrs, side, side, wm, wm, noise_px=0.5, outlier_frac=0.05, cert_mode="tiefree", device=dev)
            refs.append(hb.ReferenceInputs(ref_cam=r, nbr_cams=nbrs, cert=[s.cert[j].clone() for j in range(k)], warp=[s.warp[j].clone() for j in range(k)],
                                           image=s.image))
        batch = hb.PreparedBatch(refs, wm, wm)
        M = 10000
        params = hb.make_params(lfd.DensePipelineConfig(output_path="", matches_per_ref=M))
        cap = R * side * side if source == "dense" else R * (M + 24 * 24 + 64)
        src, dst = hb.OutputBuffers(cap, R, k, dev), hb.OutputBuffers(cap, R, k, dev)
        if source == "dense":
            tri = lambda: dens.launch_dense(batch, params, src)
        else:
            def tri():
                dens.seed_rng(1)
                dens.launch_sampled_chain(batch, params, M, src)
        tri()
        dens.check_launches()
        res = src.collect(indexed=source != "dense")
        n_in = res.count
        args = (dens._ctx, C.byref(batch.c), C.byref(src.c), src.ref_offsets.data_ptr(), MIN_SUPPORT, C.c_float(TAU), C.byref(dst.c),
                dst.ref_offsets.data_ptr(), dst.seg_counts.data_ptr(), None)
        launch = lambda: lib.lfd_support_filter(*args)
        assert launch() == 0
        torch.cuda.synchronize()
        n_kept = int(dst.ref_offsets[-1])
        # the torch form's inputs, prepared outside the timed region
        cert = torch.stack([torch.stack([c.reshape(-1) for c in r.cert]) for r in refs])
        warp = torch.stack([torch.stack([w.reshape(side * side, 2) for w in r.warp]) for r in refs])
        P = torch.tensor(np.stack([np.stack([np.asarray(cams[n].P, np.float32) for n in r.nbr_cams]) for r in refs]), device=dev)
        sxy = torch.tensor(np.stack([np.stack([[np.float32(cams[n].width / wm), np.float32(cams[n].height / wm)] for n in r.nbr_cams]) for r in refs]), device=dev)
        off = torch.from_numpy(np.asarray(res.ref_offsets)).to(dev)
        ref_of = torch.repeat_interleave(torch.arange(R, device=dev), off[1:] - off[:-1])
        cell_l, slot_l = res.cell.long(), res.slot.long()
        form = lambda: torch_filter(cert, warp, P, sxy, float(wm - 1), float(wm - 1), res.xyz, res.rgb, res.err, cell_l, slot_l, ref_of, TAU, MIN_SUPPORT)
        same = int(form()[0].shape[0])
        group = 20 if n_in > 1000000 else 100
        for fn in (launch, form, tri):
            timed(fn, max(2, group // 4))
        t_l, t_t, t_d = [], [], []
        for _ in range(passes):
            t_l.append(timed(launch, group))
            t_t.append(timed(form, group))
            t_d.append(timed(tri, max(2, group // 4)))
        med = lambda v: float(np.median(v))
        nbytes = n_in * (17 + 12 * (k - 1) + 2) + n_kept * (16 + 33)
        clear = max(t_l) < min(t_t)
        verdict &= clear
        out(f"{label:44s} {n_in:9d} {n_kept:9d}   {med(t_l):8.1f} ({min(t_l):.1f}..{max(t_l):.1f})   {100 * nbytes / (med(t_l) * 1e-6) / HBM_PEAK:6.1f} %   "
            f"{med(t_t):8.1f} ({min(t_t):.1f}..{max(t_t):.1f})   {med(t_t) / med(t_l):6.1f} x   {med(t_d):10.1f}   {100 * med(t_l) / med(t_d):6.1f} %"
            f"      (torch keeps {same}: {'equal' if same == n_kept else 'differs by ' + str(same - n_kept)}; faster beyond the spread: {'yes' if clear else 'NO'})")
        del refs, batch, src, dst, cert, warp, res
        torch.cuda.empty_cache()
    out(f"kernel faster than the torch form at every shape by more than the spread of the passes: {'yes' if verdict else 'NO'}")
    dens.close()


def run_dense_init(scene_root, matcher, mode, m):
    import torch
    from lichtfeld_densification_plugin_amd import densify
    name = f"support_{mode}.ply"
    argv = ["--scene_root", scene_root, "--images_subdir", "images_4", "--roma_setting", "fast", "--num_refs", "0.8", "--nns_per_ref", "3",
            "--matches_per_ref", "10000", "--reproj_thresh", "0.8", "--out_name", name, "--triangulation_mode", mode, "--device_image_prep"]
    if mode == "dense":
        argv += ["--refs_per_launch", "16"]          # (no streamed output: the filter works on arrays, and both settings take the same route)
    if m > 0:
        argv += ["--min_support_views", str(m)]
    args = densify.build_argparser().parse_args(argv)
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


def e2e_part(passes, scene_root, out):
    import torch
    from lichtfeld_densification_plugin_amd import densify, synthetic
    dev = torch.device("cuda:0")
    synthetic.write_colmap_scene(scene_root, n_cams=185, images_subdir="images_4", fmt="jpg")
    plan = densify.build_argparser().parse_args(["--scene_root", scene_root, "--images_subdir", "images_4", "--num_refs", "0.8", "--nns_per_ref", "3"])
    records, refs, nn, _ = densify.plan_scene(plan)
    matcher = synthetic.SyntheticMatcher(records, setting="fast", device=dev, noise_px=0.5, outlier_frac=0.05, channels=2, seed=0)
    matcher.precompute(refs, nn, 3)
    for mode in ("sampled", "dense"):
        res = {}
        for m in (0, 1):
            run_dense_init(scene_root, matcher, mode, m)                   # warm-up
        for _ in range(passes):
            for m in (0, 1):
                res.setdefault(m, []).append(run_dense_init(scene_root, matcher, mode, m))
        for m in (0, 1):
            v = [d for d, _n in res[m]]
            out(f"dense_init {mode:8s} filter {'off' if m == 0 else 'min_support_views = 1'}: median {np.median(v):.3f} s ({min(v):.3f}..{max(v):.3f}), "
                f"{len(refs)} references, {res[m][0][1]} points")


def resources(out):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "lichtfeld-densification-plugin_amd", "csrc"))
    import build as lfd_build
    with tempfile.TemporaryDirectory() as tmp:
        cmd = lfd_build.compile_command("lfd_support.hip", os.path.join(tmp, "c.o"), ["-Rpass-analysis=kernel-resource-usage"])
        err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    cur = None
    for ln in err.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = m.group(1)
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and cur and "lfd_support" in cur:
            out(f"{cur}: {m.group(1)} {m.group(2)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--e2e-passes", type=int, default=3)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--skip-operator", action="store_true")
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it (the second of two chained parts)")
    ap.add_argument("--scene", type=str, default=None)
    ap.add_argument("--out", type=str, default=os.path.join(HERE, "r9", "support_filter.txt"))
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
    out(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; passes {a.passes} (operator), {a.e2e_passes} (end to end); "
        f"support_thresh_px {TAU}, min_support {MIN_SUPPORT}")
    if not a.skip_operator:
        operator_part(a.passes, out)
    if not a.skip_e2e:
        e2e_part(a.e2e_passes, a.scene or os.path.join(tempfile.gettempdir(), "lfd_support_scene"), out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
