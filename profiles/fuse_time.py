#!/usr/bin/env python3
"""Oriented voxel fusion on one GPU (lfd_fuse_oriented, csrc/lfd_fuse.hip): what profiles/r16/fuse.txt records.

    python profiles/fuse_time.py                      # the timings below, printed and written to profiles/r16/fuse.txt
    python profiles/fuse_time.py --no-gui             # ... without the end-to-end runs
    python profiles/fuse_time.py --trace              # two calls per cloud and voxel size only: the run to put under rocprofv3 --kernel-trace
    python profiles/fuse_time.py --phases TRACE.csv   # rocprofv3's kernel_trace.csv of that run -> time per phase and call (appended)

One GPU step each: run them under a time limit of their own (``timeout -k 10 600 python ...``).

- the survivor clouds WITH NORMALS of the bench's 185-camera scene (profiles/consensus_time.py builds it), sampled mode and dense mode, as
  run_dense_pipeline returns them with experimental['estimate_normals']: device tensors
- the call at voxel_size = 1, 2 and 4 times the cloud's median nearest-neighbour spacing (consensus_time.spacing): device events around the call,
  the median of 7 passes after a warm-up call; rows out over points in, voxels, two-sided voxels
- lfd_voxel_downsample on the same cloud at the same size in the same run - the yardstick: it shares min / max, keys, sort and heads
- densify.dense_init_from_lfs end to end with estimate_normals on and the knob off and on (2 x spacing), both modes
"""
from __future__ import annotations

import argparse
import csv
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "profiles")):
    if p not in sys.path:
        sys.path.insert(0, p)

import consensus_time as ct          # noqa: E402  (the scene, the spacing estimate and the timing loop are that script's)

OUT = os.path.join(ROOT, "profiles", "r16", "fuse.txt")
PHASES = {"lfd_voxel_minmax_kernel": "keys", "lfd_voxel_final_kernel": "keys", "lfd_voxel_keys_kernel": "keys",
          "lfd_voxel_hist_kernel": "sort", "lfd_voxel_scan_kernel": "sort", "lfd_voxel_scatter_kernel": "sort",
          "lfd_voxel_head_count_kernel": "heads", "lfd_voxel_head_scatter_kernel": "heads",
          "lfd_fuse_side_kernel": "sides", "lfd_fuse_side_big_kernel": "sides", "lfd_fuse_rowsum_kernel": "rows", "lfd_fuse_rowstart_kernel": "rows",
          "lfd_fuse_sums_kernel": "sums", "lfd_fuse_sums_big_kernel": "sums", "lfd_voxel_sums_kernel": "sums", "lfd_voxel_sums_big_kernel": "sums"}
NORMALS = {"estimate_normals": True}
say = ct.say


def survivors(scene, mode):
    from lichtfeld_densification_plugin_amd.core import pipeline as pl
    tmp, _nodes, recs, refs, nn_table, matcher = scene
    res = pl.run_dense_pipeline(recs, refs, nn_table, ct.config(os.path.join(tmp.name, "cloud.ply"), mode, dict(NORMALS)), matcher=matcher)
    xyz, rgb, _err = res.device_points
    return xyz.contiguous(), res.device_normals.contiguous(), rgb.contiguous()


def operator_part(dens, label, xyz, nrm, rgb, trace):
    n = int(xyz.shape[0])
    s = ct.spacing(xyz)
    say(f"{label}: {n:,} points with normals, median nearest-neighbour spacing {s:.5f}")
    for mult in (1, 2, 4):
        h = mult * s
        if trace:
            dens.voxel_downsample(xyz, rgb, h)
            dens.fuse_oriented(xyz, nrm, rgb, h)
            continue
        v_ms, _lo, _hi = ct.timed(lambda: dens.voxel_downsample(xyz, rgb, h))
        rows = int(dens.fuse_oriented(xyz, nrm, rgb, h)[0].shape[0])
        vox = int(dens.fuse_voxels)
        ms, lo, hi = ct.timed(lambda: dens.fuse_oriented(xyz, nrm, rgb, h))
        say(f"  voxel_size {mult} x spacing = {h:.5f}  rows {rows:>11,} ({rows / n:6.2%} of the points)  voxels {vox:>11,}  two-sided {rows - vox:>9,}  "
            f"call {ms:9.3f} ms (min {lo:.3f}, max {hi:.3f})  lfd_voxel_downsample {v_ms:8.3f} ms  ratio {ms / v_ms:5.2f} x")
    return s


def gui_runs(scene, mode, h, reps=3):
    from bench_pipeline import _clear_image_caches
    from lichtfeld_densification_plugin_amd import densify
    tmp, nodes, _recs, _refs, _nn, matcher = scene
    out = os.path.join(tmp.name, "gui.ply")
    for exp in (dict(NORMALS), {**NORMALS, "fuse_voxel_size": float(h)}):
        cfg = ct.config(out, mode, exp)
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
        say(f"dense_init_from_lfs {mode:<8} normals on, fusion {'on ' if 'fuse_voxel_size' in exp else 'off'} {nvert:>11,} vertices of 27 bytes written  "
            f"median {np.median(ts):7.3f} s  (runs: {', '.join(f'{t:.3f}' for t in ts)})")


def phases(path):
    """kernel_trace.csv of a --trace run: per call (a call starts at its min / max kernel) the kernel time per phase"""
    calls = []
    with open(path) as fh:
        rows = sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"]))
    for row in rows:
        name = row["Kernel_Name"]
        if name.startswith("lfd_voxel_minmax_kernel"):
            calls.append({})
        key = next((v for k, v in PHASES.items() if name.startswith(k)), None)
        if key is None or not calls:
            continue
        calls[-1][key] = calls[-1].get(key, 0.0) + (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6
    text = ["phase split per call of the --trace run (rocprofv3 kernel trace; ms of kernel time; the calls in the order the script makes them: per cloud",
            "and voxel size lfd_voxel_downsample, then lfd_fuse_oriented):"]
    for i, c in enumerate(calls):
        kind = "fuse " if "sides" in c else "voxel"
        text.append(f"  call {i:>2} {kind}  " + "  ".join(f"{k} {c.get(k, 0.0):8.3f}" for k in ("keys", "sort", "heads", "sides", "rows", "sums"))
                    + f"  total {sum(c.values()):9.3f}")
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
    assert torch.cuda.is_available(), "fuse_time.py measures on the GPU"
    say(f"device: {torch.cuda.get_device_name(0)}; calls: median of 7 passes after one warm-up call (device events)")
    scene = ct.bench_scene()
    dens = hb.HipDensifier(torch.device("cuda:0"))
    sizes = {}
    for mode in ("sampled", "dense"):
        xyz, nrm, rgb = survivors(scene, mode)
        sizes[mode] = 2.0 * operator_part(dens, f"{mode} mode survivors", xyz, nrm, rgb, a.trace)
        del xyz, nrm, rgb
        torch.cuda.empty_cache()
    dens.close()
    if not a.trace and not a.no_gui:
        for mode in ("sampled", "dense"):
            gui_runs(scene, mode, sizes[mode])
    scene[0].cleanup()
    if not a.trace:
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        with open(OUT, "w") as fh:
            fh.write("\n".join(ct._lines) + "\n")


if __name__ == "__main__":
    main()
