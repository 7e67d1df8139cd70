#!/usr/bin/env python3
"""The spatial point cap (lfd_cap_spatial, csrc/lfd_cap.hip) on one GPU: what profiles/r21/cap.txt records.

    python profiles/cap_time.py                       # everything below, printed as text
    python profiles/cap_time.py --trace               # one call per cloud only: the run to put under rocprofv3 --kernel-trace --stats
    python profiles/cap_time.py --phases STATS.csv    # rocprofv3's kernel_stats.csv -> time per phase (min/max, keys, sort, levels, heads, ...)

- clouds of 10^6, 10^7 and 3.45 x 10^7 surface points (a dense and a sparse unit square side by side, 10 : 1, z ~ N(0, 0.002), shuffled, with a
  reprojection error per point), budget 10^6: device events around lfd_cap_spatial, the median of 5 passes after a warm-up call, with the call's
  statistics; then the gather of xyz / rgb / err by the returned index, which stays on the device
- on the same clouds today's random cap on the device route: the draw on the host (densify._cap_index), the upload of its index and the same
  gather - a host clock around work that ends in a device synchronise
- the two are interleaved pass by pass, so that whatever else the machine does meets both alike
- at 10^6 points the budget does not bind: the driver runs neither cap there; the row is what a direct call costs (the sort and the level counts
  for the statistics, then the identity)
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
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = (1_000_000, 10_000_000, 34_500_000)
BUDGET = 1_000_000
PHASES = {"lfd_consensus_minmax_kernel": "min/max", "lfd_voxel_final_kernel": "min/max", "lfd_cap_keys_kernel": "keys",
          "lfd_voxel_hist_kernel": "sort", "lfd_voxel_scan_kernel": "scans (sort, heads, compaction)", "lfd_voxel_scatter_kernel": "sort",
          "lfd_cap_levels_kernel": "levels", "lfd_cap_coarsen_kernel": "coarsen", "lfd_voxel_head_count_kernel": "heads",
          "lfd_voxel_head_scatter_kernel": "heads", "lfd_cap_rep_kernel": "representatives", "lfd_cap_mark_kernel": "mark",
          "lfd_consensus_wgcount_kernel": "compaction", "lfd_cap_index_kernel": "compaction"}


def cloud(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    n_sparse = n // 11
    xy = torch.rand((n, 2), generator=g, device="cuda")
    xy[:n_sparse, 0] += 1.0
    z = torch.randn((n, 1), generator=g, device="cuda") * 0.002
    perm = torch.randperm(n, generator=g, device="cuda")
    xyz = torch.cat([xy, z], 1)[perm].float().contiguous()
    rgb = torch.rand((n, 3), generator=g, device="cuda").contiguous()
    err = (torch.rand((n,), generator=g, device="cuda") * 2.0).contiguous()
    return xyz, rgb, err


def gather(tensors, keep):
    return tuple(t[keep] for t in tensors)


def spatial_pass(dens, pts):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    keep = dens.cap_spatial(pts[0], pts[2], BUDGET)
    b.record()
    out = gather(pts, keep)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    return a.elapsed_time(b), (t1 - t0) * 1e3, int(out[0].shape[0])


def random_pass(pts, seed):
    from lichtfeld_densification_plugin_amd import densify
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    keep = densify._cap_index(int(pts[0].shape[0]), BUDGET, seed)
    t1 = time.perf_counter()
    out = pts if keep is None else gather(pts, torch.from_numpy(keep).to(pts[0].device))
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t0) * 1e3, int(out[0].shape[0])


def phases(path):
    tot = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name") or row.get("KernelName") or ""
            key = next((v for k, v in PHASES.items() if name.startswith(k)), None)
            if key is None:
                continue
            t = tot.setdefault(key, [0.0, 0])
            t[0] += float(row.get("TotalDurationNs") or 0.0)
            t[1] += int(row.get("Calls") or 0)
    total = sum(v[0] for v in tot.values())
    print("phase split over the traced calls (rocprofv3 kernel stats, --trace run):")
    for k, (ns, calls) in sorted(tot.items(), key=lambda kv: -kv[1][0]):
        print(f"  {k:<32} {ns / 1e6:9.3f} ms over {calls:>5} launches  {ns / total:6.1%}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--phases", default=None)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.phases:
        phases(a.phases)
        return
    from lichtfeld_densification_plugin_amd.core import hip_backend as hb
    assert torch.cuda.is_available(), "cap_time.py measures on the GPU"
    dens = hb.HipDensifier(torch.device("cuda:0"))
    if a.trace:
        for n in SIZES[1:]:
            pts = cloud(n, n % 9973)
            dens.cap_spatial(pts[0], pts[2], BUDGET)
            del pts
            torch.cuda.empty_cache()
        torch.cuda.synchronize()
        dens.close()
        return
    print(f"device: {torch.cuda.get_device_name(0)}; budget {BUDGET:,}; medians of {a.reps} interleaved passes after one warm-up pass of each")
    for n in SIZES:
        pts = cloud(n, n % 9973)
        spatial_pass(dens, pts)
        random_pass(pts, 0)
        sp, rn = [], []
        for r in range(a.reps):
            sp.append(spatial_pass(dens, pts))
            rn.append(random_pass(pts, r))
        lev, cells, above, side = dens.cap_stats
        call_ms, total_ms = np.median([s[0] for s in sp]), np.median([s[1] for s in sp])
        draw_ms, rnd_ms = np.median([s[0] for s in rn]), np.median([s[1] for s in rn])
        print(f"n={n:>11,}  spatial: call {call_ms:9.3f} ms (device events), call + gather {total_ms:9.3f} ms, kept {sp[-1][2]:,}, level {lev}, "
              f"cells {cells:,}, one level up {above:,}, L {side:.4f}  |  random: draw {draw_ms:9.3f} ms, draw + upload + gather {rnd_ms:9.3f} ms, "
              f"kept {rn[-1][2]:,}", flush=True)
        del pts
        torch.cuda.empty_cache()
    dens.close()


if __name__ == "__main__":
    main()
