#!/usr/bin/env python3
"""The connected-component filter (lfd_component_filter, csrc/lfd_component.hip) on one GPU: what profiles/r33/component.txt
records.

    python profiles/component_timing.py                      # everything below, printed as text
    python profiles/component_timing.py --trace component    # the filter alone, one call per cloud and radius: the run to put under
                                                             # rocprofv3 --kernel-trace --stats; --trace consensus: the yardstick alone;
                                                             # --trace sheet / sheet_plain: the single-sheet cloud with the size kernel's
                                                             # aggregation and without it
    python profiles/component_timing.py --phases STATS.csv   # rocprofv3's kernel_stats.csv -> time per kernel of the library

One GPU step each: run them under a time limit of their own (``timeout -k 10 600 python ...``).

- the survivor cloud of the 64 x 3 x 512^2 dense workload (as profiles/thin_timing.py builds it) at two radii at which a point has about 10 and
  about 30 neighbours - found by bisection on the 256 nearest distances of 512 sampled points, the measured mean is printed -, and the
  1 052 673-point cloud of tests/test_gpu_thin.py at about 10
- lfd_component_filter (sizes and labels asked for) beside lfd_consensus_filter with counts at the same radius on the same cloud - the existing
  call that walks the same 27 cells: the same process, alternating call by call, device events around each call (both are synchronous), the
  median and lowest .. highest of ``--reps`` calls after two warm-up calls of each
- a single sheet (a 2048 x 2048 lattice at 0.7 radius: ONE component of 4.2 M points): the whole call with the size kernel's in-wave and LDS
  aggregation and with the plain one-atomic-per-point form (LFD_COMPONENT_PLAIN_SIZE=1, read when a context is made); the kernel's own time
  is the --trace sheet / sheet_plain runs'
"""
from __future__ import annotations

import argparse
import csv
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "profiles")):
    if p not in sys.path:
        sys.path.insert(0, p)

MIN_POINTS = 50
KERNELS = ("lfd_consensus_minmax_kernel", "lfd_voxel_final_kernel", "lfd_consensus_keys_kernel", "lfd_voxel_hist_kernel", "lfd_voxel_scan_kernel",
           "lfd_voxel_scatter_kernel", "lfd_consensus_gather_kernel", "lfd_consensus_count_kernel", "lfd_component_gather_kernel",
           "lfd_component_link_kernel", "lfd_component_flatten_kernel", "lfd_component_size_kernel", "lfd_component_mark_kernel",
           "lfd_consensus_wgcount_kernel", "lfd_consensus_offsets_kernel", "lfd_consensus_scatter_kernel")


def nearest_distances(xyz, sample=512, k=256, seed=0):
    """(sample, k) ascending distances from `sample` random points of the cloud to their k nearest other points (all pairs, in chunks)"""
    n = int(xyz.shape[0])
    idx = torch.from_numpy(np.random.default_rng(seed).choice(n, sample, replace=False)).to(xyz.device)
    out = []
    for a in range(0, sample, 32):
        q = xyz[idx[a:a + 32]]
        d2 = ((q[:, None, :] - xyz[None, :, :]) ** 2).sum(-1)
        out.append(torch.topk(d2, k + 1, dim=1, largest=False).values[:, 1:].sqrt())        # without the point itself
    return torch.cat(out).cpu().numpy()


def radius_for(dist, neighbours):
    """the radius at which the sampled points have `neighbours` neighbours on average, and that average as measured"""
    lo, hi = float(dist.min()), float(dist[:, -1].min())                   # below hi no row is cut off at k
    for _ in range(50):
        mid = 0.5 * (lo + hi)
        if (dist <= mid).sum(1).mean() < neighbours:
            lo = mid
        else:
            hi = mid
    return hi, float((dist <= hi).sum(1).mean())


def sheet_cloud(dev, side=2048, radius=0.01):
    a = torch.arange(side, device=dev, dtype=torch.float32) * (0.7 * radius)
    u, v = torch.meshgrid(a, a, indexing="ij")
    xyz = torch.stack([u.reshape(-1), v.reshape(-1), torch.zeros(side * side, device=dev)], 1).contiguous()
    xyz = xyz[torch.randperm(side * side, device=dev, generator=torch.Generator(device=dev).manual_seed(1))].contiguous()
    return xyz, np.asarray([side * side], np.int64), radius


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def cases(dens, dev, say):
    """[(label, xyz, counts, radius)] of the timed runs"""
    import thin_timing
    out = []
    xyz, _err, counts, _rows = thin_timing.workload_cloud(dens, dev)
    dist = nearest_distances(xyz)
    for want in (10, 30):
        r, mean = radius_for(dist, want)
        out.append((f"64 x 3 x 512^2 dense survivors, radius {r:.5f} (measured mean {mean:.1f} neighbours over 512 sampled points)", xyz, counts, r))
    xyz, _err, counts, _rows = thin_timing.test_cloud(dev)
    r, mean = radius_for(nearest_distances(xyz), 10)
    out.append((f"test cloud, radius {r:.5f} (measured mean {mean:.1f} neighbours over 512 sampled points)", xyz, counts, r))
    return out


def measure(dens, label, xyz, counts, radius, reps, say):
    n = int(xyz.shape[0])
    comp = lambda: dens.component_filter(xyz, None, None, counts, radius, MIN_POINTS, True, True)      # noqa: E731
    cons = lambda: dens.consensus_filter(xyz, None, None, counts, radius, 1, True)      # noqa: E731
    got = comp()
    s = got[6]
    say(f"{label}: {n:,} points of {int((np.asarray(counts) > 0).sum())} references")
    say(f"  {int(s[0]):,} components, largest {int(s[1]):,}; {int(got[0].shape[0]):,} points kept at min_points {MIN_POINTS}")
    for _ in range(2):
        comp()
        cons()
    t, c = [], []
    for _ in range(reps):
        t.append(event_ms(comp))
        c.append(event_ms(cons))
    tm, cm = float(np.median(t)), float(np.median(c))
    say(f"    lfd_component_filter (sizes, labels, summary) {tm:9.3f} ms (lowest {min(t):.3f}, highest {max(t):.3f}; {reps} calls)")
    say(f"    lfd_consensus_filter (counts, min_refs 1)     {cm:9.3f} ms (lowest {min(c):.3f}, highest {max(c):.3f})")
    say(f"    component / consensus {tm / cm:.3f}")


def measure_sheet(hb, dev, reps, say):
    xyz, counts, radius = sheet_cloud(dev)
    times = {}
    for plain in (0, 1):
        os.environ["LFD_COMPONENT_PLAIN_SIZE"] = str(plain)
        d = hb.HipDensifier(dev)                                           # the switch is read when the context is made
        call = lambda: d.component_filter(xyz, None, None, counts, radius, MIN_POINTS, True, True)      # noqa: E731
        s = call()[6]
        assert int(s[0]) == 1 and int(s[1]) == int(xyz.shape[0])
        call()
        times[plain] = [event_ms(call) for _ in range(reps)]
        d.close()
    os.environ.pop("LFD_COMPONENT_PLAIN_SIZE", None)
    say(f"single sheet: {int(xyz.shape[0]):,} points, one component (every point adds to ONE root)")
    for plain, name in ((0, "size kernel with in-wave + LDS aggregation"), (1, "size kernel, one atomic add and one atomic min per point")):
        t = times[plain]
        say(f"    whole call, {name:<58} {float(np.median(t)):9.3f} ms (lowest {min(t):.3f}, highest {max(t):.3f}; {reps} calls)")


def phases(path, say):
    tot = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name") or row.get("KernelName") or ""
            key = next((k for k in KERNELS if name.startswith(k)), None)
            if key is not None:
                t = tot.setdefault(key, [0.0, 0])
                t[0] += float(row.get("TotalDurationNs") or 0.0)
                t[1] += int(row.get("Calls") or 0)
    total = sum(v[0] for v in tot.values())
    say(f"kernels of the library over the traced calls (rocprofv3 kernel stats of a --trace run, {os.path.basename(os.path.dirname(path)) or path}):")
    for k, (ns, calls) in sorted(tot.items(), key=lambda kv: -kv[1][0]):
        say(f"  {k:<32} {ns / 1e6:9.3f} ms over {calls:>5} launches  {ns / total:6.1%}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", choices=("component", "consensus", "sheet", "sheet_plain"), default=None)
    ap.add_argument("--phases", default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None, help="also write the text to this file")
    a = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    if a.phases:
        phases(a.phases, say)
    else:
        from lichtfeld_densification_plugin_amd.core import hip_backend as hb
        assert torch.cuda.is_available(), "component_timing.py measures on the GPU"
        dev = torch.device("cuda:0")
        if a.trace in ("sheet", "sheet_plain"):
            os.environ["LFD_COMPONENT_PLAIN_SIZE"] = "1" if a.trace == "sheet_plain" else "0"
            dens = hb.HipDensifier(dev)
            xyz, counts, radius = sheet_cloud(dev)
            for _ in range(3):
                s = dens.component_filter(xyz, None, None, counts, radius, MIN_POINTS, True, True)[6]
            say(f"{a.trace}: {int(s[0])} component(s), largest {int(s[1]):,}")
        else:
            dens = hb.HipDensifier(dev)
            runs = cases(dens, dev, say)
            if a.trace:
                for label, xyz, counts, radius in runs:
                    if a.trace == "component":
                        s = dens.component_filter(xyz, None, None, counts, radius, MIN_POINTS, True, True)[6]
                        say(f"{label}: {int(s[0]):,} components, largest {int(s[1]):,}")
                    else:
                        say(f"{label}: {int(dens.consensus_filter(xyz, None, None, counts, radius, 1, True)[0].shape[0]):,} kept")
                torch.cuda.synchronize()
            else:
                say(f"device: {torch.cuda.get_device_name(0)}; medians of {a.reps} alternating calls after two warm-up calls of each; device events")
                for label, xyz, counts, radius in runs:
                    measure(dens, label, xyz, counts, radius, a.reps, say)
                measure_sheet(hb, dev, a.reps, say)
        dens.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
