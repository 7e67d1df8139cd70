#!/usr/bin/env python3
"""The epipolar audit on one GPU (lfd_epipolar_audit, csrc/lfd_audit.hip): one launch at the bench's dense shape - 64 references x 3
neighbours x 512^2, match 512^2 - and at k = 8, with the in-wave aggregation and as the per-lane variant (LFD_AUDIT_NO_AGGREGATE=1: every
confident lane issues its own LDS adds), with and without the cell map, beside lfd_far_accumulate on the same batch (no far cell: it reads
the same 12 bytes per cell and slot) and the dense kernel's own launch, all in the same process and session.  What DESIGN.md 4.27 records.

The batch is the noisy probe scene of the other timing profiles (ring of 185 cameras, 0.5 px iid matching noise, 5 % outliers).

    python profiles/audit_timing.py                   # needs the GPU; writes profiles/r29/audit.txt
    python profiles/audit_timing.py --resources       # registers / scratch / LDS of the kernels from the compiler (needs hipcc only)

One GPU step: run it under a time limit of its own (``timeout -k 10 600 python ...``).

Method: every launch warmed first, then ``--passes`` passes that alternate all variants, the far launch and the dense launch; a pass times a
group of back-to-back calls through the C entry point (arguments built once; the table is added to, which costs the same every time) between
two device events and divides by the group's size.  Reported: the median pass, the lowest and highest one as the spread."""
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

CERT = 0.5


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
    table = hb.audit_table(N_REFS, k, dev)
    best = torch.empty((N_REFS, SIDE * SIDE), dtype=torch.uint8, device=dev)
    far_table = hb.far_table(256, dev)

    def audit(with_best):
        args = (dens._ctx, C.byref(batch.c), C.c_float(CERT), table.data_ptr(), best.data_ptr() if with_best else None)
        return lambda: lib.lfd_epipolar_audit(*args)

    far_args = (dens._ctx, C.byref(batch.c), C.c_float(THR), C.c_float(CERT), 2, 256, far_table.data_ptr(), None)
    far = lambda: lib.lfd_far_accumulate(*far_args)
    tables = {}
    for aggregate in (True, False):
        os.environ["LFD_AUDIT_NO_AGGREGATE"] = "0" if aggregate else "1"
        table.zero_()
        assert audit(True)() == 0
        dens.check_launches()
        tables[aggregate] = table.clone()
    assert torch.equal(tables[True], tables[False]), "the two forms disagree"
    t = tables[True]
    n, deg = int(t[:, 0].sum().item()), int(t[:, 1].sum().item())
    hist = t[:, 2:].sum(dim=0)
    out(f"# {n} usable and {deg} degenerate samples of {cap * k} (cell, slot) pairs ({n / (cap * k):.3f}); bins occupied {int((hist > 0).sum().item())} of 64, "
        f"below 1 px {int(hist[:8].sum().item()) / max(n, 1):.3f}; the per-lane variant's table equals the aggregated one's, element for element")
    far_table.zero_()
    assert far() == 0
    dens.check_launches()
    out(f"# lfd_far_accumulate on the same batch: {int(far_table[:, 6].sum().item())} far cells")
    variants = [(aggregate, with_best) for aggregate in (True, False) for with_best in (True, False)]
    times = {v: [] for v in variants}
    t_far, t_dense, group = [], [], 5
    for aggregate, with_best in variants:
        os.environ["LFD_AUDIT_NO_AGGREGATE"] = "0" if aggregate else "1"
        timed(audit(with_best), 2)
    timed(far, 2)
    timed(tri, 2)
    for _ in range(passes):
        for aggregate, with_best in variants:
            os.environ["LFD_AUDIT_NO_AGGREGATE"] = "0" if aggregate else "1"
            times[(aggregate, with_best)].append(timed(audit(with_best), group))
        t_far.append(timed(far, group))
        t_dense.append(timed(tri, group))
    os.environ["LFD_AUDIT_NO_AGGREGATE"] = "0"
    med = lambda v: float(np.median(v))
    out(f"dense kernel (lfd_triangulate_dense):  {med(t_dense):9.1f} us per launch of {N_REFS} references ({min(t_dense):.1f}..{max(t_dense):.1f})")
    out(f"lfd_far_accumulate, no far cell:       {med(t_far):9.1f} us per launch ({min(t_far):.1f}..{max(t_far):.1f})")
    out("lfd_epipolar_audit   cell map   us per call (lo..hi)          x far launch   x dense kernel")
    for (aggregate, with_best), v in times.items():
        name = "in-wave aggregation" if aggregate else "per-lane LDS adds  "
        out(f"{name}  {'yes' if with_best else 'no ':>6} {med(v):9.1f} ({min(v):.1f}..{max(v):.1f})   {med(v) / med(t_far):12.3f} {med(v) / med(t_dense):14.3f}")
    dens.close()


def resources(out):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "lichtfeld-densification-plugin_amd", "csrc"))
    import build as lfd_build
    with tempfile.TemporaryDirectory() as tmp:
        cmd = lfd_build.compile_command("lfd_audit.hip", os.path.join(tmp, "c.o"), ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"])
        err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    cur = None
    for ln in err.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = m.group(1)
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and cur and "lfd_audit" in cur:
            out(f"{cur}: {m.group(1)} {m.group(2)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--out", type=str, default=os.path.join(HERE, "r29", "audit.txt"))
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
    out(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; passes {a.passes}; audit_certainty {CERT}")
    for k in (3, 8):
        one_shape(k, a.passes, out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
