#!/usr/bin/env python3
"""The image undistortion on one GPU (lfd_undistort_image, csrc/lfd_undistort.hip): what profiles/r14/undistort.txt records.

    python profiles/undistort_time.py                 # the timings below, printed and written to profiles/r14/undistort.txt
    python profiles/undistort_time.py --skip-e2e      # the operator alone

One GPU step: run it under a time limit of its own (``timeout -k 10 600 python ...``).

- device events around lfd_undistort_image (image + validity plane, asynchronous form) for a 1297 x 840 and a 5187 x 3361 RGB image, per model
  (SIMPLE_RADIAL, RADIAL, OPENCV, FULL_OPENCV): the median of 7 passes after a warm-up call
- the yardstick, timed in the same run: lfd_prepare_image of the same image to 512 x 512, the kernel the undistorted image goes into next
- dense_init end to end on the 185-camera scene written with SIMPLE_RADIAL cameras (k = -0.12), device_image_prep, sampled mode: knob off -
  the comparison - and knob on, alternating, the median of 3 runs each after a warm-up run each; every run decodes its images again
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

OUT = os.path.join(ROOT, "profiles", "r14", "undistort.txt")
MODELS = {"SIMPLE_RADIAL": (-0.12, 0, 0, 0, 0, 0, 0, 0), "RADIAL": (-0.10, 0.03, 0, 0, 0, 0, 0, 0), "OPENCV": (-0.09, 0.02, 0.004, -0.003, 0, 0, 0, 0),
          "FULL_OPENCV": (-0.11, 0.04, 0.002, 0.003, -0.01, 0.05, -0.02, 0.004)}
_lines = []


def say(text):
    print(text, flush=True)
    _lines.append(text)


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


def operator_part(dens):
    g = torch.Generator(device="cpu").manual_seed(0)
    for w, h in ((1297, 840), (5187, 3361)):
        img = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g).to(dens.device)
        f = 0.74 * w                                                # the bench scene's focal length over its width
        y_ms, y_lo, y_hi = timed(lambda: dens.prepare_image(img, (512, 512)))
        say(f"{w} x {h}: lfd_prepare_image to 512 x 512 (the yardstick) {y_ms:8.3f} ms (min {y_lo:.3f}, max {y_hi:.3f})")
        for name, d in MODELS.items():
            params = (f, f * 1.003, w / 2.0 + 3.25, h / 2.0 - 1.75) + d
            n_invalid = dens.undistort_image(img, params, with_valid=True, count=True, workspace="time")[2]
            ms, lo, hi = timed(lambda: dens.undistort_image(img, params, with_valid=True, workspace="time"))
            moved = w * h * (3 + 3 + 1)                             # bytes read once, written, and the validity plane
            say(f"  {name:<14} lfd_undistort_image {ms:8.3f} ms (min {lo:.3f}, max {hi:.3f})  {moved / ms / 1e6:8.1f} GB/s of image bytes  "
                f"{ms / y_ms:5.2f} x the yardstick  invalid pixels {n_invalid}")
        del img
        torch.cuda.empty_cache()


def end_to_end(reps=3):
    from bench_pipeline import _clear_image_caches
    from lichtfeld_densification_plugin_amd import densify, synthetic
    with tempfile.TemporaryDirectory(prefix="lfd_undistort_scene_") as root:
        synthetic.write_colmap_scene(root, n_cams=185, width=1297, height=840, images_subdir="images_4", fmt="jpg", seed=0,
                                     camera_model="SIMPLE_RADIAL", distortion=(-0.12,))
        base = ["--scene_root", root, "--images_subdir", "images_4", "--num_refs", "0.8", "--nns_per_ref", "3", "--matches_per_ref", "10000",
                "--device_image_prep"]
        plan = densify.build_argparser().parse_args(base)
        records, refs, nn_table, _ = densify.plan_scene(plan)
        matcher = synthetic.SyntheticMatcher(records, setting="fast", device="cuda:0", noise_px=0.5, outlier_frac=0.05, channels=2, seed=0)
        matcher.precompute(refs, nn_table, 3)
        times = {False: [], True: []}
        for r in range(reps + 1):                                   # the first run of each is a warm-up
            for on in (False, True):
                args = densify.build_argparser().parse_args(base + ["--out_name", f"knob_{int(on)}.ply"] + (["--undistort_images"] if on else []))
                _clear_image_caches()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rc = densify.dense_init(args, matcher=matcher)
                torch.cuda.synchronize()
                if rc != 0:
                    raise RuntimeError(f"dense_init returned {rc}")
                if r:
                    times[on].append(time.perf_counter() - t0)
        for on in (False, True):
            ts = times[on]
            say(f"dense_init 185 cameras 1297 x 840 SIMPLE_RADIAL, sampled, device_image_prep, undistort_images {'on ' if on else 'off'}  median "
                f"{np.median(ts):7.3f} s  (runs: {', '.join(f'{t:.3f}' for t in ts)})")
        say(f"  knob on - knob off: {np.median(times[True]) - np.median(times[False]):+.3f} s for 185 undistorted images")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-e2e", action="store_true")
    a = ap.parse_args()
    from lichtfeld_densification_plugin_amd.core import hip_backend as hb
    assert torch.cuda.is_available(), "undistort_time.py measures on the GPU"
    say(f"device: {torch.cuda.get_device_name(0)}; calls: median of 7 passes after one warm-up call (device events)")
    dens = hb.HipDensifier(torch.device("cuda:0"))
    operator_part(dens)
    dens.close()
    if a.skip_e2e:
        say("dense_init end to end: NOT MEASURED (--skip-e2e)")
    else:
        end_to_end()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write("\n".join(_lines) + "\n")


if __name__ == "__main__":
    main()
