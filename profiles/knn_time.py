#!/usr/bin/env python3
"""The Gaussian-ready output on one GPU (lfd_knn_dist2 and lfd_pack_gaussians, csrc/lfd_knn.hip): what profiles/r17/knn.txt records.

    python profiles/knn_time.py                        # the timings below, printed and written to profiles/r17/knn.txt
    python profiles/knn_time.py --sizes 100000         # ... at these point counts only (default 1e5, 1e6, 1e7)
    python profiles/knn_time.py --no-twin              # ... without the 16-thread twin beside them
    python profiles/knn_time.py --check                # ... and compare the device's dist2 with the twin's bit for bit (needs the twin)

One GPU step: run it under a time limit of its own (``timeout -k 10 900 python ...``).

- a synthetic multi-plane surface cloud (six planes of random pose in the unit cube, 0.2 % thickness), and the same cloud with 0.1 % of its
  points replaced by far outliers (uniform in a cube 200 times as wide), which inflate the bounding box and exercise the automatic cell size's
  refinement and the brute-force pass
- lfd_knn_dist2 with the automatic cell size and lfd_pack_gaussians: device events around the call, the median of 5 passes after a warm-up
  call; the call's statistics (cell size used, occupied cells, points in the fullest cell, points finished by brute force)
- the 16-thread twin's wall time for the same call, one pass
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "profiles")):
    if p not in sys.path:
        sys.path.insert(0, p)

import consensus_time as ct          # noqa: E402  (say and the timing loop are that script's)

OUT = os.path.join(ROOT, "profiles", "r17", "knn.txt")
say = ct.say


def surface_cloud(n: int, seed: int = 0, outlier_frac: float = 0.0):
    """(xyz, normals, rgb) float32: n points on six planes of random pose through the unit cube, 0.2 % thick; ``outlier_frac`` of them moved far out"""
    rs = np.random.RandomState(seed)
    plane = rs.randint(0, 6, n)
    nrm6 = rs.normal(size=(6, 3))
    nrm6 /= np.linalg.norm(nrm6, axis=1, keepdims=True)
    u6 = np.cross(nrm6, rs.normal(size=(6, 3)))
    u6 /= np.linalg.norm(u6, axis=1, keepdims=True)
    v6 = np.cross(nrm6, u6)
    c6 = rs.uniform(-0.2, 0.2, (6, 3))
    a, b, t = rs.uniform(-0.5, 0.5, n), rs.uniform(-0.5, 0.5, n), rs.normal(0.0, 0.002, n)
    xyz = c6[plane] + a[:, None] * u6[plane] + b[:, None] * v6[plane] + t[:, None] * nrm6[plane]
    k = int(round(outlier_frac * n))
    if k:
        xyz[rs.choice(n, k, replace=False)] = rs.uniform(-100.0, 100.0, (k, 3))
    return xyz.astype(np.float32), nrm6[plane].astype(np.float32), rs.uniform(0, 1, (n, 3)).astype(np.float32)


def one_cloud(dens, twin, label, arrays, check):
    xyz, nrm, rgb = (torch.from_numpy(a).cuda() for a in arrays)
    n = int(xyz.shape[0])
    d2 = dens.knn_dist2(xyz)
    stats = dens.knn_stats
    ms, lo, hi = ct.timed(lambda: dens.knn_dist2(xyz), passes=5)
    p_ms, p_lo, p_hi = ct.timed(lambda: dens.pack_gaussians(xyz, nrm, rgb, d2, flatten=0.3), passes=5)
    line = (f"{label:<28} n {n:>11,}  lfd_knn_dist2 {ms:10.3f} ms (min {lo:.3f}, max {hi:.3f})  {n / ms / 1e3:8.2f} M points/s  "
            f"lfd_pack_gaussians {p_ms:8.3f} ms (min {p_lo:.3f}, max {p_hi:.3f})  "
            f"stats: cell size {stats[0]:.6g}, {stats[1]:,} occupied cells, fullest {stats[2]:,}, {stats[3]:,} by brute force")
    if twin is not None:
        t0 = time.perf_counter()
        w = twin.knn_dist2(torch.from_numpy(arrays[0]))
        t_twin = time.perf_counter() - t0
        line += f"  twin ({twin.n_threads} threads) {t_twin * 1e3:11.1f} ms, stats equal: {twin.knn_stats == stats}"
        if check:
            line += f", dist2 values that differ: {int((w.numpy().view(np.uint32) != d2.cpu().numpy().view(np.uint32)).sum())}"
    say(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[100_000, 1_000_000, 10_000_000])
    ap.add_argument("--no-twin", action="store_true")
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    from lichtfeld_densification_plugin_amd.core import hip_backend as hb
    assert torch.cuda.is_available(), "knn_time.py measures on the GPU"
    say(f"device: {torch.cuda.get_device_name(0)}; calls: median of 5 passes after one warm-up call (device events); twin: one pass, wall time")
    dens = hb.HipDensifier(torch.device("cuda:0"))
    twin = None if a.no_twin else hb.HostDensifier(16)
    for n in a.sizes:
        one_cloud(dens, twin, "surface", surface_cloud(n), a.check)
        one_cloud(dens, twin, "surface + 0.1 % far outliers", surface_cloud(n, outlier_frac=0.001), a.check)
    dens.close()
    if twin is not None:
        twin.close()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write("\n".join(ct._lines) + "\n")


if __name__ == "__main__":
    main()
