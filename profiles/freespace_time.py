#!/usr/bin/env python3
"""The free-space filter on one GPU (lfd_freespace_filter, csrc/lfd_freespace.hip): what profiles/r15/freespace.txt records.

    python profiles/freespace_time.py                      # the timings below, printed and written to profiles/r15/freespace.txt
    python profiles/freespace_time.py --no-gui             # the calls only
    python profiles/freespace_time.py --modes sampled      # one mode only

One GPU step each: run them under a time limit of their own (``timeout -k 10 900 python ...``).

- the survivor clouds of the bench's 185-camera scene (ring cameras, analytic warps at the 'fast' preset, 148 references with 3 neighbours),
  sampled mode and dense mode, as run_dense_pipeline returns them: device tensors, the per-reference counts and the matcher's grid
- lfd_freespace_filter at the automatic plane size (densify.freespace_plane), tol = 0.02, min_violations = 2, without and with the count
  arrays: device events around the call, the median of 7 passes after a warm-up call; the work is n * n_refs projections
- lfd_consensus_filter at radius = 2 x the cloud's median nearest-neighbour spacing, min_refs = 2, on the same cloud in the same session - the
  yardstick: the other filter that runs once on the final cloud
- densify.dense_init_from_lfs end to end with the knob off and on, both modes
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "profiles", "r15", "freespace.txt")
TOL, MIN_VIOLATIONS = 0.02, 2
MIN_REFS = 2
_lines = []


def say(text):
    print(text, flush=True)
    _lines.append(text)


def bench_scene():
    from bench_pipeline import _SceneNode
    from lichtfeld_densification_plugin_amd import densify, synthetic
    from lichtfeld_densification_plugin_amd.core.selection import nearest_neighbors, select_cameras_kcenters
    tmp = tempfile.TemporaryDirectory(prefix="lfd_freespace_scene_")
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
    return tmp, nodes, recs, refs, nn_table, matcher


def config(out, mode, exp=None):
    import lichtfeld_densification_plugin_amd as lfd
    return lfd.DensePipelineConfig(output_path=out, roma_setting="fast", num_refs=0.8, nns_per_ref=3, matches_per_ref=10000, viz_interval=0,
                                   device_image_prep=True, triangulation_mode=mode, experimental=exp or {})


def survivors(scene, mode):
    from lichtfeld_densification_plugin_amd import densify
    from lichtfeld_densification_plugin_amd.core import pipeline as pl
    tmp, _nodes, recs, refs, nn_table, matcher = scene
    cfg = config(os.path.join(tmp.name, "cloud.ply"), mode, {"min_freespace_violations": MIN_VIOLATIONS})
    res = pl.run_dense_pipeline(recs, refs, nn_table, cfg, matcher=matcher)
    cams = [recs[int(r)] for r in refs]
    cam_P = np.stack([np.asarray(c.P, np.float64).astype(np.float32).reshape(12) for c in cams])
    cam_wh = np.array([[int(c.width), int(c.height)] for c in cams], np.int32)
    plane = densify.freespace_plane(cfg, cams[0].width, cams[0].height, res.match_grid)
    return tuple(t.contiguous() for t in res.device_points), np.asarray(res.points_per_reference, np.int64), cam_P, cam_wh, plane


def spacing(xyz, queries=512, chunk=2_000_000):
    """median distance to the nearest other point, from `queries` random points against the whole cloud"""
    g = torch.Generator(device="cpu").manual_seed(0)
    pick = torch.randperm(int(xyz.shape[0]), generator=g)[:queries].to(xyz.device)
    q = xyz[pick].double()
    best = torch.full((q.shape[0],), float("inf"), dtype=torch.float64, device=xyz.device)
    for a in range(0, int(xyz.shape[0]), chunk):
        d = torch.cdist(q, xyz[a:a + chunk].double())
        d[d == 0.0] = float("inf")                                   # the point itself (and exact duplicates)
        best = torch.minimum(best, d.min(1).values)
    return float(best.median())


def timed(fn, passes=7):
    fn()                                                            # warm-up (and the workspace grows here)
    torch.cuda.synchronize()
    ms = []
    for _ in range(passes):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def operator_part(dens, label, pts, counts, cam_P, cam_wh, plane):
    xyz, rgb, err = pts
    n, n_refs = int(xyz.shape[0]), int(len(counts))
    s = spacing(xyz)
    say(f"{label}: {n:,} points of {int((counts > 0).sum())} references ({n_refs} cameras in the table), planes of {plane[0]} x {plane[1]} cells, "
        f"{n * n_refs:.3g} projections, median nearest-neighbour spacing {s:.5f}")
    for with_c in (False, True):
        kept = int(dens.freespace_filter(xyz, rgb, err, counts, cam_P, cam_wh, plane, TOL, MIN_VIOLATIONS, with_c)[0].shape[0])
        ms, lo, hi = timed(lambda: dens.freespace_filter(xyz, rgb, err, counts, cam_P, cam_wh, plane, TOL, MIN_VIOLATIONS, with_c))
        say(f"  lfd_freespace_filter  count arrays {'yes' if with_c else 'no ':<3}  kept {kept:>11,} ({kept / n:6.2%})  call {ms:10.3f} ms "
            f"(min {lo:.3f}, max {hi:.3f})  {n * n_refs / ms / 1e6:8.2f} G projections / s")
    radius = 2.0 * s
    kept = int(dens.consensus_filter(xyz, rgb, err, counts, radius, MIN_REFS, False)[0].shape[0])
    c_ms, lo, hi = timed(lambda: dens.consensus_filter(xyz, rgb, err, counts, radius, MIN_REFS, False))
    say(f"  lfd_consensus_filter  radius 2 x spacing = {radius:.5f}, min_refs {MIN_REFS}  kept {kept:>11,} ({kept / n:6.2%})  call {c_ms:10.3f} ms "
        f"(min {lo:.3f}, max {hi:.3f})  free space / consensus {ms / c_ms:6.2f} x")


def gui_runs(scene, mode, reps=3):
    from bench_pipeline import _clear_image_caches
    from lichtfeld_densification_plugin_amd import densify
    tmp, nodes, _recs, _refs, _nn, matcher = scene
    out = os.path.join(tmp.name, "gui.ply")
    for exp in ({}, {"min_freespace_violations": MIN_VIOLATIONS, "freespace_depth_tol_rel": TOL}):
        cfg = config(out, mode, exp)
        ts = []
        for r in range(reps + 1):                                   # the first run is a warm-up
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
        say(f"dense_init_from_lfs {mode:<8} free-space filter {'on ' if exp else 'off'} {nvert:>11,} points written  median {np.median(ts):7.3f} s  "
            f"(runs: {', '.join(f'{t:.3f}' for t in ts)})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-gui", action="store_true")
    ap.add_argument("--modes", default="sampled,dense")
    a = ap.parse_args()
    modes = [m for m in a.modes.split(",") if m]
    from lichtfeld_densification_plugin_amd.core import hip_backend as hb
    assert torch.cuda.is_available(), "freespace_time.py measures on the GPU"
    say(f"device: {torch.cuda.get_device_name(0)}; calls: median of 7 passes after one warm-up call (device events), tol = {TOL}, "
        f"min_violations = {MIN_VIOLATIONS}")
    scene = bench_scene()
    dens = hb.HipDensifier(torch.device("cuda:0"))
    for mode in modes:
        pts, counts, cam_P, cam_wh, plane = survivors(scene, mode)
        operator_part(dens, f"{mode} mode survivors", pts, counts, cam_P, cam_wh, plane)
        del pts
        torch.cuda.empty_cache()
    dens.close()
    if not a.no_gui:
        for mode in modes:
            gui_runs(scene, mode)
    scene[0].cleanup()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a" if a.modes != "sampled,dense" and os.path.exists(OUT) else "w") as fh:
        fh.write("\n".join(_lines) + "\n")


if __name__ == "__main__":
    main()
