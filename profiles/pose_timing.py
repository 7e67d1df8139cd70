#!/usr/bin/env python3
"""The pose refinement's statistics on one GPU (lfd_pose_accumulate, csrc/lfd_pose.hip): one launch at the bench's dense shape - 64 references
x 3 neighbours x 512^2, match 512^2 - and at k = 8, beside lfd_epipolar_audit on the same batch (the same 12 bytes read per cell and slot,
the same confidence test) and the dense kernel's own launch, all in the same process and session.  What DESIGN.md 4.28 records.

The batch is the noisy probe scene of the other timing profiles (ring of 185 cameras, 0.5 px iid matching noise, 5 % outliers).

    python profiles/pose_timing.py                   # needs the GPU; writes profiles/r30/pose.txt
    python profiles/pose_timing.py --resources       # registers / scratch / LDS of the kernels from the compiler (needs hipcc only)

One GPU step: run it under a time limit of its own (``timeout -k 10 600 python ...``).

Method: every launch warmed first, then ``--passes`` passes that alternate the pose launch, the audit's launch and the dense launch; a pass
times a group of back-to-back calls through the C entry point (arguments built once; the table is added to, which costs the same every
time - at most 2^62 per launch and column, and the table is cleared between groups) between two device events and divides by the group's
size.  Reported: the median pass, the lowest and highest one as the spread."""
from __future__ import annotations

import argparse
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from colour_timing import MATCH, N_REFS, SIDE, THR, references, timed       # noqa: E402  (the same workload, built by the same code)

CERT, INLIER_PX = 0.5, 8.0


def one_shape(k, passes, out):
    import torch
    import lichtfeld_densification_plugin_amd as lfd
    from lichtfeld_densification_plugin_amd import synthetic as syn
    from lichtfeld_densification_plugin_amd.core import hip_backend as hb
    dev = torch.device("cuda:0")
    dens = hb.HipDensifier(dev)
    lib = hb.load_library()
    cams = syn.ring_cameras(185)
    dens.upload_cameras(cams)
    params = hb.make_params(lfd.DensePipelineConfig(output_path="", reproj_thresh=THR))
    batch = hb.PreparedBatch(references(cams, dev, k), MATCH, MATCH)
    cap = N_REFS * SIDE * SIDE
    src = hb.OutputBuffers(cap, N_REFS, k, dev)
    tri = lambda: dens.launch_dense(batch, params, src)
    tri()
    dens.check_launches()
    out(f"# {N_REFS} references x {k} neighbours x {SIDE}^2, match {MATCH}^2: {int(src.ref_offsets[-1].item())} dense survivors")
    table = hb.pose_table(N_REFS, k, dev)
    audit_table = hb.audit_table(N_REFS, k, dev)
    pose_args = (dens._ctx, C.byref(batch.c), C.c_float(CERT), C.c_float(INLIER_PX), table.data_ptr())
    pose = lambda: lib.lfd_pose_accumulate(*pose_args)
    audit_args = (dens._ctx, C.byref(batch.c), C.c_float(CERT), audit_table.data_ptr(), None)
    audit = lambda: lib.lfd_epipolar_audit(*audit_args)
    assert pose() == 0 and audit() == 0
    dens.check_launches()
    t = table.clone()
    n_in, n_out, n_deg = (int(t[:, c].sum().item()) for c in range(3))
    out(f"# {n_in} inliers, {n_out} outliers and {n_deg} degenerate samples of {cap * k} (cell, slot) pairs ({(n_in + n_out + n_deg) / (cap * k):.3f} "
        f"confident); rms distance of the inliers {float(np.sqrt(t[:, 3].sum().item() / 1048576.0 / max(n_in, 1))):.3f} px; the audit counts "
        f"{int(audit_table[:, 0].sum().item()) + int(audit_table[:, 1].sum().item())} confident samples")
    t_pose, t_audit, t_dense, group = [], [], [], 5
    timed(pose, 2)
    timed(audit, 2)
    timed(tri, 2)
    for _ in range(passes):
        table.zero_()
        t_pose.append(timed(pose, group))
        t_audit.append(timed(audit, group))
        t_dense.append(timed(tri, group))
    med = lambda v: float(np.median(v))
    out(f"dense kernel (lfd_triangulate_dense):  {med(t_dense):9.1f} us per launch of {N_REFS} references ({min(t_dense):.1f}..{max(t_dense):.1f})")
    out(f"lfd_epipolar_audit, no cell map:       {med(t_audit):9.1f} us per launch ({min(t_audit):.1f}..{max(t_audit):.1f})")
    out(f"lfd_pose_accumulate:                   {med(t_pose):9.1f} us per launch ({min(t_pose):.1f}..{max(t_pose):.1f}): "
        f"{med(t_pose) / med(t_audit):.3f} x the audit's launch, {med(t_pose) / med(t_dense):.3f} x the dense kernel's")
    dens.close()


def resources(out):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "lichtfeld-densification-plugin_amd", "csrc"))
    import build as lfd_build
    with tempfile.TemporaryDirectory() as tmp:
        cmd = lfd_build.compile_command("lfd_pose.hip", os.path.join(tmp, "c.o"), ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"])
        err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    cur = None
    for ln in err.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = m.group(1)
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and cur and "lfd_pose" in cur:
            out(f"{cur}: {m.group(1)} {m.group(2)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--out", type=str, default=os.path.join(HERE, "r30", "pose.txt"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(HERE))
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    if a.resources:
        resources(out)
        return
    import torch
    out(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; passes {a.passes}; pose_certainty {CERT}, pose_inlier_px {INLIER_PX}")
    for k in (3, 8):
        one_shape(k, a.passes, out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
