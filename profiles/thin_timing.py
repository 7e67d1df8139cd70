#!/usr/bin/env python3
"""The footprint-adaptive thinning (lfd_thin_footprint, csrc/lfd_thin.hip) on one GPU: what profiles/r26/thin.txt records.

    python profiles/thin_timing.py                      # everything below, printed as text
    python profiles/thin_timing.py --trace thin         # the thinning alone, one call per knob value on the workload cloud (--cloud test: on the
                                                        # test cloud): the run to put under rocprofv3 --kernel-trace --stats; --trace cap: the cap
                                                        # alone at the same kept counts
    python profiles/thin_timing.py --phases STATS.csv   # rocprofv3's kernel_stats.csv -> time per kernel of the library

One GPU step each: run them under a time limit of their own (``timeout -k 10 600 python ...``).

- the survivor cloud of the 64 x 3 x 512^2 dense workload (the ring scene's cameras, analytic warps, as profiles/support_filter_time.py builds
  it), with its per-reference offsets and the five values per reference from the cameras and the 512 x 512 grid; and the 1 052 673-point cloud
  of tests/test_gpu_thin.py (three references)
- lfd_thin_footprint at footprint_thin_cells = 2, 1 and 0.5 and, as the yardstick, lfd_cap_spatial at a budget equal to the thinning's kept
  count: the same process, alternating call by call, device events around each call (both are synchronous), the median and lowest .. highest of
  ``--reps`` calls after two warm-up calls of each
- the kept fraction and the points and cells of every level in use
"""
from __future__ import annotations

import argparse
import csv
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

CELLS = (2.0, 1.0, 0.5)
KERNELS = ("lfd_consensus_minmax_kernel", "lfd_voxel_final_kernel", "lfd_thin_keys_kernel", "lfd_thin_cells_kernel", "lfd_cap_keys_kernel",
           "lfd_cap_levels_kernel", "lfd_cap_coarsen_kernel", "lfd_voxel_hist_kernel", "lfd_voxel_scan_kernel", "lfd_voxel_scatter_kernel",
           "lfd_voxel_head_count_kernel", "lfd_voxel_head_scatter_kernel", "lfd_cap_rep_kernel", "lfd_cap_mark_kernel", "lfd_consensus_wgcount_kernel",
           "lfd_consensus_offsets_kernel", "lfd_cap_index_kernel")


def workload_cloud(dens, dev, R=64, k=3, side=512):
    """(xyz, err, counts, rows) of the 64 x 3 x 512^2 dense workload's survivors"""
    import lichtfeld_densification_plugin_amd as lfd
    from lichtfeld_densification_plugin_amd import densify, synthetic as syn
    from lichtfeld_densification_plugin_amd.core import hip_backend as hb
    cams = syn.ring_cameras(185)
    dens.upload_cameras(cams)
    refs, ref_ids = [], []
    for i in range(R):
        r = (10 + 2 * i) % 185
        nbrs = syn.ring_neighbours(185, r, k)
        s = syn.synth_reference(cams, r, nbrs, side, side, side, side, noise_px=0.5, outlier_frac=0.05, cert_mode="tiefree", device=dev)
        refs.append(hb.ReferenceInputs(ref_cam=r, nbr_cams=nbrs, cert=[s.cert[j].clone() for j in range(k)], warp=[s.warp[j].clone() for j in range(k)],
                                       image=s.image))
        ref_ids.append(r)
    batch = hb.PreparedBatch(refs, side, side)
    params = hb.make_params(lfd.DensePipelineConfig(output_path="", matches_per_ref=10000))
    src = hb.OutputBuffers(R * side * side, R, k, dev)
    dens.launch_dense(batch, params, src)
    dens.check_launches()
    res = src.collect(indexed=False)
    counts = np.diff(np.asarray(res.ref_offsets, np.int64))
    rows = densify.footprint_rows(cams, ref_ids, (side, side))
    return res.xyz.contiguous().clone(), res.err.contiguous().clone(), counts, rows


def test_cloud(dev):
    import thin_ref as tr
    counts = [400000, 252673, 400000]
    xyz, err, rows = tr.random_case(1052673, counts, 8)
    return torch.from_numpy(xyz).to(dev), torch.from_numpy(err).to(dev), np.asarray(counts, np.int64), rows


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def measure(dens, label, cloud, reps, say):
    xyz, err, counts, rows = cloud
    n = int(xyz.shape[0])
    say(f"{label}: {n:,} points of {int((counts > 0).sum())} references")
    for cells in CELLS:
        thin = lambda: dens.thin_footprint(xyz, err, counts, rows, cells)
        keep, _ = thin()
        kept = int(keep.shape[0])
        points, in_cells, side = dens.thin_stats
        cap = lambda: dens.cap_spatial(xyz, err, kept)
        for _ in range(2):
            thin()
            cap()
        t, c = [], []
        for _ in range(reps):
            t.append(event_ms(thin))
            c.append(event_ms(cap))
        tm, cm = float(np.median(t)), float(np.median(c))
        say(f"  footprint_thin_cells {cells:g}: kept {kept:,} ({kept / n:.2%}), L {side:.4f}")
        say(f"    lfd_thin_footprint              {tm:9.3f} ms (lowest {min(t):.3f}, highest {max(t):.3f}; {reps} calls)")
        say(f"    lfd_cap_spatial, budget {kept:>10,} {cm:9.3f} ms (lowest {min(c):.3f}, highest {max(c):.3f}; level {dens.cap_stats[0]})")
        say(f"    thin / cap {tm / cm:.3f}; the cap's own spread (highest - lowest) / median {(max(c) - min(c)) / cm:.3f}; "
            f"thin slower beyond that spread: {'yes' if tm - cm > max(c) - min(c) else 'no'}")
        say("    level: points / cells  " + "  ".join(f"{l}: {int(points[l]):,} / {int(in_cells[l]):,}" for l in np.flatnonzero(points)))


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
    ap.add_argument("--trace", choices=("thin", "cap"), default=None)
    ap.add_argument("--cloud", choices=("workload", "test"), default="workload", help="the cloud of a --trace run")
    ap.add_argument("--phases", default=None)
    ap.add_argument("--reps", type=int, default=25)
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
        assert torch.cuda.is_available(), "thin_timing.py measures on the GPU"
        dev = torch.device("cuda:0")
        dens = hb.HipDensifier(dev)
        if a.trace:
            # one function per traced run, so that the shared kernels' time is that function's; the cap's budgets are the thinning's kept
            # counts, taken from the CPU twin here so that no thinning kernel enters the cap's trace
            xyz, err, counts, rows = workload_cloud(dens, dev) if a.cloud == "workload" else test_cloud(dev)
            if a.trace == "cap":
                twin = hb.HostDensifier(16)
                hx, he = xyz.cpu(), err.cpu()
                budgets = [int(twin.thin_footprint(hx, he, counts, rows, cells)[0].shape[0]) for cells in CELLS]
                twin.close()
            for i, cells in enumerate(CELLS):
                if a.trace == "thin":
                    say(f"thin {cells:g}: kept {int(dens.thin_footprint(xyz, err, counts, rows, cells)[0].shape[0]):,}")
                else:
                    say(f"cap {budgets[i]:,}: kept {int(dens.cap_spatial(xyz, err, budgets[i]).shape[0]):,}")
            torch.cuda.synchronize()
        else:
            clouds = (("64 x 3 x 512^2 dense survivors", workload_cloud(dens, dev)), ("test cloud", test_cloud(dev)))
            say(f"device: {torch.cuda.get_device_name(0)}; medians of {a.reps} alternating calls after two warm-up calls of each; device events")
            for label, cloud in clouds:
                measure(dens, label, cloud, a.reps, say)
        dens.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
