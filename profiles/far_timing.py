#!/usr/bin/env python3
"""The far-field shell on one GPU (lfd_far_accumulate / lfd_far_emit, csrc/lfd_far.hip): the accumulate launch at the bench's dense shape
- 64 references x 3 neighbours x 512^2, match 512^2 - with 0, 0.3 and 1.0 of the grid's rows far, with and without the in-wave reduction
over runs of equal keys (LFD_FAR_NO_REDUCE=1: every far lane issues its own seven atomic adds), beside the dense kernel's own launch on the
same batch in the same session (device events around a group, and the kernel's own duration through lfd_kernel_timing); then lfd_far_emit
at S = 256 and 512 on the table of the all-far batch.  What DESIGN.md 4.26 records.

The batch is the noisy probe scene of the other timing profiles (ring of 185 cameras, 0.5 px iid matching noise, 5 % outliers).  The top
``fraction`` of every reference's grid rows is rewritten: observation = the rotation-only transfer of the cell into the neighbour, computed in
f64 with torch, certainty 0.9 - those cells are far unless the transfer leaves the neighbour's image; the rest keeps the scene's parallax.

    python profiles/far_timing.py                   # needs the GPU; writes profiles/r28/far.txt
    python profiles/far_timing.py --resources       # registers / scratch / LDS of the kernels from the compiler (needs hipcc only)

One GPU step: run it under a time limit of its own (``timeout -k 10 600 python ...``).

Method: every launch warmed first, then ``--passes`` passes that alternate all variants and the dense launch; a pass times a group of
back-to-back calls through the C entry point (arguments built once; the table is added to, which costs the same every time) between two
device events and divides by the group's size.  Reported: the median pass, the lowest and highest one as the spread."""
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

CERT, VIEWS, S_DEFAULT = 0.5, 2, 256
FRACTIONS = (0.0, 0.3, 1.0)


def with_far_rows(refs, cams, fraction, dev):
    """The references with the top ``fraction`` of their rows looking at infinity."""
    import torch
    from lichtfeld_densification_plugin_amd import synthetic as syn
    from lichtfeld_densification_plugin_amd.core import hip_backend as hb
    rows = int(round(fraction * SIDE))
    if rows == 0:
        return refs
    ax = syn.identity_axis_torch(SIDE, dev).double()
    yy, xx = torch.meshgrid(ax[:rows], ax, indexing="ij")
    out = []
    for ri in refs:
        a = cams[int(ri.ref_cam)]
        u = (xx + 1.0) * 0.5 * (MATCH - 1) * (a.width / float(MATCH))
        v = (yy + 1.0) * 0.5 * (MATCH - 1) * (a.height / float(MATCH))
        Ka, Ra = torch.from_numpy(np.asarray(a.K, np.float64)).to(dev), torch.from_numpy(np.asarray(a.R, np.float64)).to(dev)
        d = torch.stack([(u - Ka[0, 2]) / Ka[0, 0], (v - Ka[1, 2]) / Ka[1, 1], torch.ones_like(u)], dim=-1) @ Ra
        cert, warp = [], []
        for j, n in enumerate(ri.nbr_cams):
            b = cams[int(n)]
            Kb, Rb = torch.from_numpy(np.asarray(b.K, np.float64)).to(dev), torch.from_numpy(np.asarray(b.R, np.float64)).to(dev)
            p = (d @ Rb.T) @ Kb.T
            ub, vb = p[..., 0] / p[..., 2], p[..., 1] / p[..., 2]
            w = ri.warp[j].clone()
            w[:rows, :, -2] = (ub / (b.width / float(MATCH)) / (0.5 * (MATCH - 1)) - 1.0).float()
            w[:rows, :, -1] = (vb / (b.height / float(MATCH)) / (0.5 * (MATCH - 1)) - 1.0).float()
            c = ri.cert[j].clone()
            c[:rows] = 0.9
            cert.append(c)
            warp.append(w)
        out.append(hb.ReferenceInputs(ref_cam=ri.ref_cam, nbr_cams=ri.nbr_cams, cert=cert, warp=warp, image=ri.image))
    return out


def run(passes, out):
    import torch
    import lichtfeld_densification_plugin_amd as lfd
    from lichtfeld_densification_plugin_amd import synthetic as syn
    from lichtfeld_densification_plugin_amd.core import hip_backend as hb
    k = 3
    dev = torch.device("cuda:0")
    dens = hb.HipDensifier(dev)
    lib = hb.load_library()
    cams = syn.ring_cameras(185)
    dens.upload_cameras(cams)
    params = hb.make_params(lfd.DensePipelineConfig(output_path="", reproj_thresh=THR))
    base = references(cams, dev, k)
    cap = N_REFS * SIDE * SIDE
    src = hb.OutputBuffers(cap, N_REFS, k, dev)
    batches = {f: hb.PreparedBatch(with_far_rows(base, cams, f, dev), MATCH, MATCH) for f in FRACTIONS}
    tri = lambda: dens.launch_dense(batches[0.0], params, src)
    tri()
    dens.check_launches()
    out(f"# {N_REFS} references x {k} neighbours x {SIDE}^2, match {MATCH}^2: {int(src.ref_offsets[-1].item())} dense survivors of the plain batch")
    table = hb.far_table(S_DEFAULT, dev)
    counters = torch.zeros(N_REFS, dtype=torch.int64, device=dev)

    def acc(f, cnt):
        args = (dens._ctx, C.byref(batches[f].c), C.c_float(THR), C.c_float(CERT), VIEWS, S_DEFAULT, table.data_ptr(), cnt)
        return lambda: lib.lfd_far_accumulate(*args)

    tables = {}
    for reduce in (True, False):
        os.environ["LFD_FAR_NO_REDUCE"] = "0" if reduce else "1"
        for f in FRACTIONS:
            table.zero_()
            counters.zero_()
            assert acc(f, counters.data_ptr())() == 0
            dens.check_launches()
            tables[(f, reduce)] = table.clone()
            if reduce:
                runs = int((table[:, 6] > 0).sum().item())
                out(f"# far rows {f:.1f}: {int(counters.sum().item())} far cells of {cap} ({int(counters.sum().item()) / cap:.3f}) in {runs} direction cells")
    for f in FRACTIONS:
        assert torch.equal(tables[(f, True)], tables[(f, False)]), "the two forms disagree"
    out("# the table of the form without the reduction equals the reduced form's, element for element, at every fraction")
    variants = [(f, reduce) for reduce in (True, False) for f in FRACTIONS]
    times = {v: [] for v in variants}
    t_dense, group = [], 5
    for f, reduce in variants:
        os.environ["LFD_FAR_NO_REDUCE"] = "0" if reduce else "1"
        timed(acc(f, None), 2)
    timed(tri, 2)
    for _ in range(passes):
        for f, reduce in variants:
            os.environ["LFD_FAR_NO_REDUCE"] = "0" if reduce else "1"
            times[(f, reduce)].append(timed(acc(f, None), group))
        t_dense.append(timed(tri, group))
    os.environ["LFD_FAR_NO_REDUCE"] = "0"
    dens.time_dense_kernels(10)
    for _ in range(10):
        tri()
    own = dens.dense_kernel_times_ms() * 1e3
    dens.time_dense_kernels(0)
    med = lambda v: float(np.median(v))
    out(f"dense kernel (lfd_triangulate_dense): {med(t_dense):9.1f} us per launch of {N_REFS} references ({min(t_dense):.1f}..{max(t_dense):.1f}); "
        f"its own duration (lfd_kernel_timing, 10 launches): {med(own):.1f} us ({own.min():.1f}..{own.max():.1f})")
    out("accumulate        far rows   us per call (lo..hi)          x dense kernel")
    for (f, reduce), v in times.items():
        name = "run reduction" if reduce else "lane per add "
        out(f"{name}     {f:8.1f} {med(v):9.1f} ({min(v):.1f}..{max(v):.1f})   {med(v) / med(t_dense):14.3f}")
    # emit, on the all-far table (synchronous: the call's wall time, read-back of the count included)
    import time
    for S in (256, 512):
        tab = hb.far_table(S, dev)
        os.environ["LFD_FAR_NO_REDUCE"] = "0"
        dens.far_accumulate(batches[1.0], THR, CERT, VIEWS, S, table=tab)
        torch.cuda.synchronize()
        centre = np.zeros(3)
        n = int(dens.far_emit(tab, S, 2, centre, 100.0, with_normals=True)[0].shape[0])
        xyz, rgb, nrm = (torch.empty((max(n, 1), 3), device=dev) for _ in range(3))
        smp = torch.empty((max(n, 1),), dtype=torch.int32, device=dev)
        c3, n_out = (C.c_double * 3)(0.0, 0.0, 0.0), C.c_int64(0)
        call = lambda: lib.lfd_far_emit(dens._ctx, tab.data_ptr(), S, 2, c3, C.c_double(100.0), xyz.data_ptr(), rgb.data_ptr(), nrm.data_ptr(),
                                        smp.data_ptr(), n, C.byref(n_out))
        for _ in range(3):
            assert call() == 0
        t = []
        for _ in range(passes * 3):
            t0 = time.perf_counter()
            call()
            t.append((time.perf_counter() - t0) * 1e6)
        out(f"emit S = {S}: {6 * S * S} direction cells, {n} points: {med(t):9.1f} us per call, synchronous ({min(t):.1f}..{max(t):.1f})")
    dens.close()


def resources(out):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "lichtfeld-densification-plugin_amd", "csrc"))
    import build as lfd_build
    with tempfile.TemporaryDirectory() as tmp:
        cmd = lfd_build.compile_command("lfd_far.hip", os.path.join(tmp, "c.o"), ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"])
        err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    cur = None
    for ln in err.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = m.group(1)
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and cur and "lfd_far" in cur:
            out(f"{cur}: {m.group(1)} {m.group(2)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--out", type=str, default=os.path.join(HERE, "r28", "far.txt"))
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
    out(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; passes {a.passes}; far_thresh_px {THR}, far_certainty {CERT}, "
        f"far_min_views {VIEWS}, S {S_DEFAULT}")
    run(a.passes, out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
