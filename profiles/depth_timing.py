#!/usr/bin/env python3
"""The depth-map renderer on one GPU (lfd_render_depth, csrc/lfd_depth.hip): the call's time on the survivors of the dense launch at the bench's
shape - 64 references x 3 neighbours x 512^2, match 512^2, ring of 185 cameras - into 64 (the references) and 185 (all) cameras on planes of 256^2
and 512^2 cells at the default knobs, beside two yardsticks that are not the code under test - the CPU twin on 16 threads and the same rule written
with torch on the same GPU - and beside the dense kernel's own time.  What DESIGN.md 4.22 records.  (The "every atomic" lines of
profiles/r24/depth.txt are the same run with a second splat kernel that issued every atomic without reading the word first; it lost by
2.9 .. 5.0 x and was not kept, so this script no longer produces them.)

    python profiles/depth_timing.py                    # needs the GPU; writes profiles/r24/depth.txt
    python profiles/depth_timing.py --trace            # six calls at 185 cameras x 512^2 only: the run to put under
                                                       #   rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/depth_timing.py --trace
    python profiles/depth_timing.py --shares DIR       # that run's kernel_stats.csv -> the three kernels' shares (appended to the file)
    python profiles/depth_timing.py --resources        # registers / scratch / LDS of the kernels from the compiler (needs hipcc only)

One GPU step each: run them under a time limit of their own (``timeout -k 10 900 python ...``).

Method: every call warmed first, then ``--passes`` passes; a pass times one call between two device events.
Reported: the median pass, the lowest and highest one as the spread.  The torch form (``torch_render``): per camera the projection term by term
in f64, ``scatter_reduce_(amin)`` of int64 keys into the plane, ``max_pool2d`` on the negated depths for both min-filters; its depths are
compared with the HIP path's bit for bit, its indices are not produced (a pooled f64 cannot hold a 63-bit key).  The twin is timed once per
shape - it takes seconds - and its three outputs are compared with the HIP path's at the size that is timed."""
from __future__ import annotations

import argparse
import csv
import glob
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N_REFS, SIDE, MATCH, K = 64, 512, 512, 3
THR = 0.8
SPLAT, WINDOW, TOL = 1, 3, 0.02
OUT = os.path.join(HERE, "r24", "depth.txt")


def event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def dense_cloud(dev):
    """(dens, cams, ref indices, xyz of the dense launch's survivors, the launch as a callable)"""
    import torch
    import lichtfeld_densification_plugin_amd as lfd
    from lichtfeld_densification_plugin_amd import synthetic as syn
    from lichtfeld_densification_plugin_amd.core import hip_backend as hb
    dens = hb.HipDensifier(dev)
    cams = syn.ring_cameras(185)
    dens.upload_cameras(cams)
    params = hb.make_params(lfd.DensePipelineConfig(output_path="", reproj_thresh=THR))
    refs, which = [], []
    for i in range(N_REFS):
        r = (10 + 2 * i) % 185
        nbrs = syn.ring_neighbours(185, r, K)
        s = syn.synth_reference(cams, r, nbrs, SIDE, SIDE, MATCH, MATCH, noise_px=0.5, outlier_frac=0.05, cert_mode="tiefree", device=dev)
        refs.append(hb.ReferenceInputs(ref_cam=r, nbr_cams=nbrs, cert=[s.cert[j].clone() for j in range(K)], warp=[s.warp[j].clone() for j in range(K)],
                                       image=s.image))
        which.append(r)
    batch = hb.PreparedBatch(refs, MATCH, MATCH)
    src = hb.OutputBuffers(N_REFS * SIDE * SIDE, N_REFS, K, dev)
    tri = lambda: dens.launch_dense(batch, params, src)      # noqa: E731
    tri()
    dens.check_launches()
    n = int(src.ref_offsets[-1].item())
    return dens, cams, which, src.xyz[:n].contiguous(), tri, (batch, src)


def camera_arrays(cams, idx):
    P = np.stack([np.asarray(cams[i].P, np.float64).astype(np.float32).reshape(12) for i in idx])
    wh = np.array([[cams[i].width, cams[i].height] for i in idx], np.int32)
    return P, wh


def torch_render(xyz, P, wh, pw, ph, r, R, tol):
    """depth (n_cams, ph, pw) f32 by the rule, with torch operators only"""
    import torch
    import torch.nn.functional as F
    dev = xyz.device
    X, Y, Z = (xyz[:, k].double() for k in range(3))
    idx = torch.arange(xyz.shape[0], device=dev, dtype=torch.int64)
    empty = (0x7F800000 << 32) | 0xFFFFFFFF
    out = torch.empty((P.shape[0], ph, pw), dtype=torch.float32, device=dev)
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    for c in range(P.shape[0]):
        p = [float(v) for v in P[c]]
        w, h = float(wh[c, 0]), float(wh[c, 1])
        p0 = ((p[0] * X + p[1] * Y) + p[2] * Z) + p[3]
        p1 = ((p[4] * X + p[5] * Y) + p[6] * Z) + p[7]
        p2 = ((p[8] * X + p[9] * Y) + p[10] * Z) + p[11]
        u, v = p0 / p2, p1 / p2
        d = p2.float()
        ok = torch.isfinite(p0) & torch.isfinite(p1) & torch.isfinite(p2) & (p2 > 0) & (u >= 0) & (u < w) & (v >= 0) & (v < h) & (d > 0) & torch.isfinite(d)
        cx = torch.clamp(torch.floor((u * pw) / w), max=pw - 1.0)
        cy = torch.clamp(torch.floor((v * ph) / h), max=ph - 1.0)
        cell = (cy * pw + cx)[ok].long()
        key = (d[ok].view(torch.int32).long() << 32) | idx[ok]
        plane = torch.full((ph * pw,), empty, dtype=torch.int64, device=dev)
        plane.scatter_reduce_(0, cell, key, "amin", include_self=True)
        raw = (plane >> 32).int().view(torch.float32).view(1, 1, ph, pw)                 # +inf where nobody is
        D = -F.max_pool2d(-raw, 2 * r + 1, 1, r) if r else raw
        m = -F.max_pool2d(-raw, 2 * (R + r) + 1, 1, R + r) if R + r else raw
        keep = torch.isfinite(D) & (D <= m + tol * m)
        out[c] = torch.where(keep, D, zero)[0, 0]
    return out


def timings(passes, out):
    import torch
    from lichtfeld_densification_plugin_amd.core import hip_backend as hb
    dev = torch.device("cuda:0")
    dens, cams, which, xyz, tri, _hold = dense_cloud(dev)
    n = int(xyz.shape[0])
    out(f"# {N_REFS} references x {K} neighbours x {SIDE}^2, match {MATCH}^2: {n:,} dense survivors; splat {SPLAT}, window {WINDOW}, tol {TOL}")
    tri()
    t_dense = [event_ms(tri) for _ in range(passes)]
    out(f"dense kernel (lfd_triangulate_dense): {np.median(t_dense):9.3f} ms per launch of {N_REFS} references ({min(t_dense):.3f}..{max(t_dense):.3f})")
    twin = hb.HostDensifier(16)
    host_xyz = xyz.cpu()
    tol32 = torch.tensor(TOL, dtype=torch.float32, device=dev)
    for n_cams, idx in ((64, which), (185, list(range(185)))):
        P, wh = camera_arrays(cams, idx)
        for side in (256, 512):
            plane = (side, side)
            hip = lambda: dens.render_depth(xyz, None, P, wh, plane, SPLAT, WINDOW, TOL, True)      # noqa: E731
            a = hip()
            torch.cuda.synchronize()
            tr = lambda: torch_render(xyz, P, wh, side, side, SPLAT, WINDOW, tol32)      # noqa: E731
            t_depth = tr()
            same_torch = torch.equal(t_depth.view(torch.int32), a[0].view(torch.int32))
            t_hip, t_torch = [], []
            for p in range(passes):
                t_hip.append(event_ms(hip))
                if p < 3:
                    t_torch.append(event_ms(tr))
            del t_depth
            t0 = time.perf_counter()
            h = twin.render_depth(host_xyz, None, P, wh, plane, SPLAT, WINDOW, TOL, True)
            t_twin = (time.perf_counter() - t0) * 1e3
            same_twin = torch.equal(h[0].view(torch.int32), a[0].cpu().view(torch.int32)) and torch.equal(h[1], a[1].cpu())
            valid = float((a[1] >= 0).float().mean().item())
            out(f"{n_cams:3d} cameras, plane {side}^2: {n * n_cams:.3g} projections, {valid:6.2%} of the cells hold data; "
                f"HIP == twin (depth, index): {same_twin}; HIP == torch (depth): {same_torch}")
            med = float(np.median(t_hip))
            out(f"    lfd_render_depth               {med:10.3f} ms ({min(t_hip):.3f}..{max(t_hip):.3f})   x dense kernel {med / np.median(t_dense):7.3f}   "
                f"{n * n_cams / med / 1e6:8.2f} G projections / s")
            out(f"    torch on the same GPU          {np.median(t_torch):10.3f} ms ({min(t_torch):.3f}..{max(t_torch):.3f})   x HIP {np.median(t_torch) / med:7.1f}")
            out(f"    CPU twin, 16 threads           {t_twin:10.1f} ms (one call)               x HIP {t_twin / med:7.1f}")
            del a, h
            torch.cuda.empty_cache()
    twin.close()
    dens.close()


def trace_calls():
    import torch
    dev = torch.device("cuda:0")
    dens, cams, _which, xyz, _tri, _hold = dense_cloud(dev)
    P, wh = camera_arrays(cams, list(range(185)))
    for _ in range(6):                                    # the first three are the warm-up
        dens.render_depth(xyz, None, P, wh, (512, 512), SPLAT, WINDOW, TOL, True)
    torch.cuda.synchronize()
    dens.close()


def shares(root, out):
    hits = glob.glob(os.path.join(root, "**", "*kernel_stats.csv"), recursive=True)
    if not hits:
        raise SystemExit(f"no kernel_stats.csv under {root}")
    rows = {}
    with open(hits[0]) as fh:
        for row in csv.DictReader(fh):
            if row["Name"].startswith("lfd_depth_"):
                total = float(row["TotalDurationNs"]) if "TotalDurationNs" in row else float(row["AverageNs"]) * int(row["Calls"])
                rows[re.sub(r"\.kd$", "", row["Name"].split("(")[0])] = (int(row["Calls"]), total)
    out("kernel shares of the --trace run (rocprofv3 --kernel-trace --stats; 185 cameras, plane 512^2, 6 calls in 2 batches each):")
    part = {k: rows[f"lfd_depth_{k}_kernel"] for k in ("fill", "splat", "resolve")}
    total = sum(v[1] for v in part.values())
    out("    " + "  ".join(f"{k} {v[1] / v[0] / 1e3:9.1f} us per launch = {v[1] / total:6.2%}" for k, v in part.items()))


def resources(out):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "lichtfeld-densification-plugin_amd", "csrc"))
    import build as lfd_build
    with tempfile.TemporaryDirectory() as tmp:
        cmd = lfd_build.compile_command("lfd_depth.hip", os.path.join(tmp, "d.o"), ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"])
        err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    cur = None
    for ln in err.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = m.group(1)
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and cur:
            out(f"{cur}: {m.group(1)} {m.group(2)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--shares", type=str, default="")
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--out", type=str, default=OUT)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(HERE))
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    if a.trace:
        trace_calls()
        return
    if a.resources or a.shares:
        resources(out) if a.resources else shares(a.shares, out)
    else:
        import torch
        out(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; passes {a.passes} (torch: 3), one call per pass between device events")
        timings(a.passes, out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a" if (a.resources or a.shares) else "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
