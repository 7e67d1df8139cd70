#!/usr/bin/env python3
"""The device distance filter (lfd_voxel_downsample, csrc/lfd_voxel.hip) on one GPU: what profiles/r7/voxel.txt records.

    python profiles/voxel_time.py                       # everything below, printed as text
    python profiles/voxel_time.py --trace               # one call per shape only: the run to put under rocprofv3 --kernel-trace --stats
    python profiles/voxel_time.py --phases STATS.csv    # rocprofv3's kernel_stats.csv -> time per phase (min/max, keys, sort, heads, sums)

- device filter on seeded clouds of 1.2e6, 1.6e7 and 1.27e8 points at voxel_size 0.001 / 0.01 / 0.1, and on a dense-mode survivor cloud of the
  bench's kind (ring cameras, analytic warps at the 'fast' preset, the fused dense kernel): device events around the call after a warm-up call,
  the PLY packing of the voxels timed apart, algorithmic bytes over time as a fraction of the 8 TB/s HBM peak
- the degenerate case: 1e7 points in at most 8 voxels
- the NumPy host path (densify._voxel_downsample) on this machine's host for the two smaller clouds, and the PCIe copy it needs first
- densify.dense_init_from_lfs end to end on the bench's 185-camera scene, with and without voxel_size = 0.01, sampled and dense mode
"""
from __future__ import annotations

import argparse
import csv
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
PHASES = {"lfd_voxel_minmax_kernel": "min/max", "lfd_voxel_final_kernel": "min/max", "lfd_voxel_keys_kernel": "keys",
          "lfd_voxel_hist_kernel": "sort", "lfd_voxel_scan_kernel": "sort/heads scan", "lfd_voxel_scatter_kernel": "sort",
          "lfd_voxel_head_count_kernel": "heads", "lfd_voxel_head_scatter_kernel": "heads", "lfd_voxel_sums_kernel": "sums",
          "lfd_voxel_sums_big_kernel": "sums", "lfd_pack_ply_kernel": "pack"}


def cloud(n, seed, dist="normal"):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if dist == "normal":
        xyz = torch.randn((n, 3), generator=g, device="cuda") * 3.0
    else:                                  # degenerate: every point in one of 8 tiny blobs -> at most 8 voxels at voxel_size 0.1
        c = torch.tensor([[0.02 + 0.3 * (i & 1), 0.02 + 0.3 * ((i >> 1) & 1), 0.02 + 0.3 * (i >> 2)] for i in range(8)], device="cuda")
        xyz = c[torch.randint(0, 8, (n,), generator=g, device="cuda")] + torch.rand((n, 3), generator=g, device="cuda") * 0.01
    return xyz.float().contiguous(), torch.rand((n, 3), generator=g, device="cuda").contiguous()


def sort_passes(xyz, vs):
    lo = xyz.min(0).values.double().cpu().numpy()
    hi = xyz.max(0).values.double().cpu().numpy()
    o = lo - 0.5 * vs
    E = [int(np.floor((hi[c] - o[c]) / vs)) + 1 for c in range(3)]
    bits = (E[0] * E[1] * E[2] - 1).bit_length()
    return (bits + 7) // 8, bits


def algo_bytes(n, nv, passes):
    """minimal traffic of the algorithm as built: min/max reads 24 n; keys read 12 n, write 12 n; a radix pass reads the keys for the
    histogram (8 n) and keys + indices for the scatter (12 n), writes 12 n; heads read the keys twice (16 n), write 4 nv; sums read the sorted
    indices (4 n) and the points (24 n) and the voxel starts (4 nv), write 24 nv"""
    return 24 * n + 24 * n + passes * 32 * n + 16 * n + 4 * nv + 28 * n + 4 * nv + 24 * nv


def time_filter(dens, xyz, rgb, vs, reps=3):
    dens.voxel_downsample(xyz, rgb, vs)                         # warm-up (and the workspace grows here)
    torch.cuda.synchronize()
    f_ms, p_ms = [], []
    for _ in range(reps):
        a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        a.record()
        xv, rv = dens.voxel_downsample(xyz, rgb, vs)
        b.record()
        dens.pack_ply(xv, rv)
        c.record()
        torch.cuda.synchronize()
        f_ms.append(a.elapsed_time(b))
        p_ms.append(b.elapsed_time(c))
    return int(xv.shape[0]), float(np.median(f_ms)), float(np.median(p_ms))


def report_filter(dens, label, xyz, rgb, vs):
    n = int(xyz.shape[0])
    passes, bits = sort_passes(xyz, vs)
    nv, f_ms, p_ms = time_filter(dens, xyz, rgb, vs)
    by = algo_bytes(n, nv, passes)
    print(f"{label:<26} n={n:>11,} vs={vs:<6} voxels={nv:>11,} key bits={bits:>2} passes={passes}  filter {f_ms:9.3f} ms  pack {p_ms:7.3f} ms  "
          f"algorithmic {by / 1e9:6.2f} GB -> {by / (f_ms * 1e-3) / 1e12:5.2f} TB/s = {by / (f_ms * 1e-3) / HBM_PEAK:5.3f} of HBM peak", flush=True)


def dense_survivors(n_refs):
    from lichtfeld_densification_plugin_amd import synthetic
    import lichtfeld_densification_plugin_amd as lfd
    from lichtfeld_densification_plugin_amd.core import hip_backend as hb
    h_lr, w_lr, H, W = synthetic.ROMA_PRESETS["fast"]
    cams = synthetic.ring_cameras(185, seed=0)
    d = hb.HipDensifier(torch.device("cuda:0"))
    try:
        d.upload_cameras(cams)
        xs, cs = [], []
        for g0 in range(0, n_refs, 16):                         # launches of 16 references, as the bench's sampled leg groups them
            refs = []
            for g in range(g0, min(n_refs, g0 + 16)):
                ref = (3 * g) % 185
                nbrs = synthetic.ring_neighbours(185, ref, 3)
                s = synthetic.synth_reference(cams, ref, nbrs, H, W, w_lr, h_lr, noise_px=0.5, outlier_frac=0.05, channels=2, seed=1000 + g,
                                              cert_mode="smooth", device="cuda:0")
                refs.append(hb.ReferenceInputs(ref_cam=ref, nbr_cams=nbrs, cert=list(s.cert), warp=list(s.warp), image=s.image))
            out = d.triangulate_dense(hb.PreparedBatch(refs, w_lr, h_lr), hb.make_params(lfd.DensePipelineConfig(output_path="", triangulation_mode="dense")))
            xs.append(out.xyz.clone())
            cs.append(out.rgb.clone())
        return torch.cat(xs).contiguous(), torch.cat(cs).contiguous()
    finally:
        d.close()


def host_path(xyz, rgb, vs):
    from lichtfeld_densification_plugin_amd import densify
    sys.modules["open3d"] = None                                # the NumPy branch (Open3D is not installed on the box either)
    err = torch.zeros((xyz.shape[0],), device=xyz.device)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    x, c, _ = xyz.cpu().numpy(), rgb.cpu().numpy(), err.cpu().numpy()     # what PipelineResult's arrays cost: 28 B per point
    t1 = time.perf_counter()
    densify._voxel_downsample(x, c, vs)
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3


def gui_runs(reps):
    from bench_pipeline import _SceneNode, _clear_image_caches
    import lichtfeld_densification_plugin_amd as lfd
    from lichtfeld_densification_plugin_amd import densify, synthetic
    from lichtfeld_densification_plugin_amd.core.selection import nearest_neighbors, select_cameras_kcenters
    tmp = tempfile.TemporaryDirectory(prefix="lfd_voxel_scene_")
    synthetic.write_colmap_scene(tmp.name, n_cams=185, width=1297, height=840, images_subdir="images_4", fmt="jpg", seed=0)
    args = densify.build_argparser().parse_args(["--scene_root", tmp.name, "--images_subdir", "images_4", "--num_refs", "0.8", "--nns_per_ref", "3"])
    records, _, _, _ = densify.plan_scene(args)
    nodes = [_SceneNode(r) for r in records]
    recs = densify.extract_cameras_from_lfs(nodes)
    flat = np.stack([c.flat_pose() for c in recs], axis=0)
    refs = select_cameras_kcenters(flat, int(round(0.8 * len(recs))))
    nn_table = nearest_neighbors(flat, 3)
    matcher = synthetic.SyntheticMatcher(recs, setting="fast", device="cuda:0", noise_px=0.5, outlier_frac=0.05, channels=2, seed=0)
    matcher.precompute(refs, nn_table, 3)
    out = os.path.join(tmp.name, "gui.ply")
    for mode in ("sampled", "dense"):
        for vs in (0.0, 0.01):
            cfg = lfd.DensePipelineConfig(output_path=out, roma_setting="fast", num_refs=0.8, nns_per_ref=3, matches_per_ref=10000, viz_interval=0,
                                          device_image_prep=True, triangulation_mode=mode, voxel_size=vs)
            ts = []
            for r in range(reps + 1):                          # the first run is a warm-up
                _clear_image_caches()
                matcher.calls = 0
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                code, info = densify.dense_init_from_lfs(nodes, cfg, matcher=matcher)
                torch.cuda.synchronize()
                if code != 0:
                    raise RuntimeError(info)
                if r:
                    ts.append(time.perf_counter() - t0)
            with open(out, "rb") as fh:
                nvert = int(fh.read(512).split(b"element vertex ")[1].split(b"\n")[0])
            print(f"dense_init_from_lfs {mode:<8} voxel_size={vs:<5} {nvert:>11,} points written  median {np.median(ts):7.3f} s  "
                  f"(runs: {', '.join(f'{t:.3f}' for t in ts)})", flush=True)
    tmp.cleanup()


def phases(path):
    tot = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name") or row.get("KernelName") or ""
            key = next((v for k, v in PHASES.items() if name.startswith(k)), None)
            if key is None:
                continue
            ns = float(row.get("TotalDurationNs") or 0.0)
            calls = int(row.get("Calls") or 0)
            t = tot.setdefault(key, [0.0, 0])
            t[0] += ns
            t[1] += calls
    total = sum(v[0] for v in tot.values())
    print("phase split over the traced calls (rocprofv3 kernel stats, --trace run):")
    for k, (ns, calls) in sorted(tot.items(), key=lambda kv: -kv[1][0]):
        print(f"  {k:<16} {ns / 1e6:9.3f} ms over {calls:>5} launches  {ns / total:6.1%}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--phases", default=None)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    if a.phases:
        phases(a.phases)
        return
    from lichtfeld_densification_plugin_amd.core import hip_backend as hb
    assert torch.cuda.is_available(), "voxel_time.py measures on the GPU"
    dens = hb.HipDensifier(torch.device("cuda:0"))
    print(f"device: {torch.cuda.get_device_name(0)}; times are medians of {a.reps} calls after one warm-up call (device events)")
    if a.trace:
        xyz, rgb = cloud(127_000_000, 0)
        for vs in (0.001, 0.01, 0.1):
            dens.voxel_downsample(xyz, rgb, vs)
            xv, rv = dens.voxel_downsample(xyz, rgb, vs)
            dens.pack_ply(xv, rv)
        torch.cuda.synchronize()
        dens.close()
        return
    for n in (1_200_000, 16_000_000, 127_000_000):
        xyz, rgb = cloud(n, n % 9973)
        for vs in (0.001, 0.01, 0.1):
            report_filter(dens, "normal(0, 3)", xyz, rgb, vs)
        del xyz, rgb
        torch.cuda.empty_cache()
    xyz, rgb = dense_survivors(148)
    for vs in (0.001, 0.01, 0.1):
        report_filter(dens, "dense survivors (148 refs)", xyz, rgb, vs)
    del xyz, rgb
    xyz, rgb = cloud(10_000_000, 1, dist="degenerate")
    report_filter(dens, "degenerate (<= 8 voxels)", xyz, rgb, 0.1)
    del xyz, rgb
    torch.cuda.empty_cache()
    for n, vss in ((1_200_000, (0.001, 0.01, 0.1)), (16_000_000, (0.01,))):
        xyz, rgb = cloud(n, n % 9973)
        for vs in vss:
            copy_ms, host_ms = host_path(xyz, rgb, vs)
            print(f"host path (NumPy branch)   n={n:>11,} vs={vs:<6} PCIe copy of xyz/rgb/err {copy_ms:8.1f} ms  _voxel_downsample {host_ms:9.1f} ms", flush=True)
    xyz, rgb = cloud(127_000_000, 0)
    copy_ms = min(_copy_only(xyz, rgb) for _ in range(3))
    print(f"PCIe copy alone            n={127_000_000:>11,} (28 B per point)            {copy_ms:8.1f} ms", flush=True)
    del xyz, rgb
    torch.cuda.empty_cache()
    dens.close()
    gui_runs(a.reps)


def _copy_only(xyz, rgb):
    err = torch.zeros((xyz.shape[0],), device=xyz.device)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    xyz.cpu(), rgb.cpu(), err.cpu()
    return (time.perf_counter() - t0) * 1e3


if __name__ == "__main__":
    main()
