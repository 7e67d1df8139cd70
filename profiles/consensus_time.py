#!/usr/bin/env python3
"""The cross-reference consensus filter on one GPU (lfd_consensus_filter, csrc/lfd_consensus.hip): what profiles/r13/consensus.txt records.

    python profiles/consensus_time.py                      # the timings below, printed and written to profiles/r13/consensus.txt
    python profiles/consensus_time.py --trace              # two calls per cloud and radius only: the run to put under rocprofv3 --kernel-trace
    python profiles/consensus_time.py --phases TRACE.csv   # rocprofv3's kernel_trace.csv of that run -> time per phase and call (appended)

One GPU step each: run them under a time limit of their own (``timeout -k 10 600 python ...``).

- the survivor clouds of the bench's 185-camera scene (ring cameras, analytic warps at the 'fast' preset, 148 references with 3 neighbours),
  sampled mode and dense mode, as run_dense_pipeline returns them: device tensors and the per-reference counts
- the call at radius = 1, 2 and 4 times the cloud's median nearest-neighbour spacing (estimated from 512 random points against the whole
  cloud), min_refs = 2, without and with the ``consensus`` array: device events around the call, the median of 7 passes after a warm-up call
- lfd_voxel_downsample at voxel_size = radius on the same cloud in the same run - the yardstick: it shares the min/max, the keys and the sort
- densify.dense_init_from_lfs end to end with the knob off and on (2 x spacing, 2 other references), both modes
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

OUT = os.path.join(ROOT, "profiles", "r13", "consensus.txt")
PHASES = {"lfd_consensus_minmax_kernel": "keys", "lfd_voxel_final_kernel": "keys", "lfd_consensus_keys_kernel": "keys",
          "lfd_voxel_hist_kernel": "sort", "lfd_voxel_scan_kernel": "sort", "lfd_voxel_scatter_kernel": "sort",
          "lfd_consensus_gather_kernel": "gather", "lfd_consensus_count_kernel": "scan", "lfd_consensus_wgcount_kernel": "compaction",
          "lfd_consensus_offsets_kernel": "compaction", "lfd_consensus_scatter_kernel": "compaction"}
MIN_REFS = 2
_lines = []


def say(text):
    print(text, flush=True)
    _lines.append(text)


def bench_scene():
    from bench_pipeline import _SceneNode
    from lichtfeld_densification_plugin_amd import densify, synthetic
    from lichtfeld_densification_plugin_amd.core.selection import nearest_neighbors, select_cameras_kcenters
    tmp = tempfile.TemporaryDirectory(prefix="lfd_consensus_scene_")
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
    from lichtfeld_densification_plugin_amd.core import pipeline as pl
    tmp, _nodes, recs, refs, nn_table, matcher = scene
    res = pl.run_dense_pipeline(recs, refs, nn_table, config(os.path.join(tmp.name, "cloud.ply"), mode), matcher=matcher)
    return tuple(t.contiguous() for t in res.device_points), np.asarray(res.points_per_reference, np.int64)


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


def operator_part(dens, label, pts, counts, trace):
    xyz, rgb, err = pts
    n = int(xyz.shape[0])
    s = spacing(xyz)
    say(f"{label}: {n:,} points of {int((counts > 0).sum())} references, median nearest-neighbour spacing {s:.5f}")
    for mult in (1, 2, 4):
        radius = mult * s
        if trace:
            for with_c in (False, True):
                dens.consensus_filter(xyz, rgb, err, counts, radius, MIN_REFS, with_c)
            continue
        v_ms, _lo, _hi = timed(lambda: dens.voxel_downsample(xyz, rgb, radius))
        for with_c in (False, True):
            kept = int(dens.consensus_filter(xyz, rgb, err, counts, radius, MIN_REFS, with_c)[0].shape[0])
            ms, lo, hi = timed(lambda: dens.consensus_filter(xyz, rgb, err, counts, radius, MIN_REFS, with_c))
            say(f"  radius {mult} x spacing = {radius:.5f}  consensus array {'yes' if with_c else 'no ':<3}  kept {kept:>11,} ({kept / n:5.1%})  "
                f"call {ms:9.3f} ms (min {lo:.3f}, max {hi:.3f})  lfd_voxel_downsample at voxel_size = radius {v_ms:8.3f} ms  ratio {ms / v_ms:5.2f} x")
    return s


def gui_runs(scene, mode, radius, reps=3):
    from bench_pipeline import _clear_image_caches
    from lichtfeld_densification_plugin_amd import densify
    tmp, nodes, _recs, _refs, _nn, matcher = scene
    out = os.path.join(tmp.name, "gui.ply")
    for exp in ({}, {"min_consensus_refs": MIN_REFS, "consensus_radius": float(radius)}):
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
        say(f"dense_init_from_lfs {mode:<8} consensus {'on ' if exp else 'off'} {nvert:>11,} points written  median {np.median(ts):7.3f} s  "
            f"(runs: {', '.join(f'{t:.3f}' for t in ts)})")


def phases(path):
    """kernel_trace.csv of a --trace run: the dispatches of every lfd_consensus_filter call (a call starts at its min/max kernel), per phase"""
    calls = []
    with open(path) as fh:
        rows = sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"]))
    for row in rows:
        name = row["Kernel_Name"]
        if name.startswith("lfd_consensus_minmax_kernel"):
            calls.append({})
        key = next((v for k, v in PHASES.items() if name.startswith(k)), None)
        if key is None or not calls:                                # (the trace run makes no other call that uses the sort's kernels)
            continue
        calls[-1][key] = calls[-1].get(key, 0.0) + (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6
    text = ["phase split per call of the --trace run (rocprofv3 kernel trace; ms of kernel time; the calls in the order the script makes them: per cloud",
            "and radius one without and one with the consensus array):"]
    for i, c in enumerate(calls):
        total = sum(c.values())
        text.append(f"  call {i:>2} ({'with' if i % 2 else 'without'} array)  " + "  ".join(f"{k} {c.get(k, 0.0):8.3f}" for k in ("keys", "sort", "gather", "scan", "compaction"))
                    + f"  total {total:9.3f}")
    print("\n".join(text))
    with open(OUT, "a") as fh:
        fh.write("\n".join(text) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--phases", default=None)
    ap.add_argument("--no-gui", action="store_true")
    a = ap.parse_args()
    if a.phases:
        phases(a.phases)
        return
    from lichtfeld_densification_plugin_amd.core import hip_backend as hb
    assert torch.cuda.is_available(), "consensus_time.py measures on the GPU"
    say(f"device: {torch.cuda.get_device_name(0)}; calls: median of 7 passes after one warm-up call (device events), min_refs = {MIN_REFS}")
    scene = bench_scene()
    dens = hb.HipDensifier(torch.device("cuda:0"))
    radii = {}
    for mode in ("sampled", "dense"):
        pts, counts = survivors(scene, mode)
        radii[mode] = 2.0 * operator_part(dens, f"{mode} mode survivors", pts, counts, a.trace)
        del pts
        torch.cuda.empty_cache()
    dens.close()
    if not a.trace and not a.no_gui:
        for mode in ("sampled", "dense"):
            gui_runs(scene, mode, radii[mode])
    scene[0].cleanup()
    if not a.trace:
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        with open(OUT, "w") as fh:
            fh.write("\n".join(_lines) + "\n")


if __name__ == "__main__":
    main()
