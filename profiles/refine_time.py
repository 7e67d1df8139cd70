#!/usr/bin/env python3
"""The multi-view re-triangulation on one GPU (lfd_refine_multiview, csrc/lfd_refine.hip) against the same operation written in torch - gathers of
the other neighbours' certainty and warp at the points' cells, the candidate test, the DLT rows of every view, M = sum row row^T in f64,
torch.linalg.eigh, the acceptance tests, a select - at the survivor counts of the bench shapes, beside the lfd_triangulate_dense call it follows.
What profiles/r10/refine.txt records.

    python profiles/refine_time.py                   # the operator part (needs the GPU)
    python profiles/refine_time.py --resources       # registers / occupancy of the kernels from the compiler (needs hipcc only)

One GPU step: run it under a time limit of its own (``timeout -k 10 600 python ...``).

Method: both forms in this one process, every shape warmed first, then ``--passes`` passes that ALTERNATE kernel, torch form and the dense launch;
a pass times a group of back-to-back calls between two device events and divides by the group's size.  The kernel is timed through the C entry
point with its arguments built once, out of place (a launch in place would refine its own result the next time).  Reported: the median pass, the
lowest and highest one as the spread; the algorithmic bytes - per input point 21 (cell, slot, xyz, err) + 8 (the winner's warp pair) + 12 (k - 1)
(certainty, warp pair of every other neighbour) read and 17 written - over the kernel's time as a share of 8 TB/s; and the kernel's time as a
share of the dense launch's.  The torch form is given its best case outside the timed region: the planes of all references stacked, the
projection matrices and pixel scales as tensors, every point's reference and the reference's own observation already known."""
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
HBM_PEAK = 8.0e12
# (label, references, neighbours, grid side, match side)
SHAPES = (("64 x 3 x 512^2 dense", 64, 3, 512, 512), ("16 x 8 x 512^2 dense", 16, 8, 512, 512), ("16 x 3 x 640^2 dense (high, 960^2 match)", 16, 3, 640, 960))
TAU, THR = 1.6, 0.8


def timed(fn, group):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(group):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / group          # microseconds


def torch_refine(cert, warp, P, sxy, Pa, sa, obs_a, wm1, hm1, xyz, err, cell, slot, ref, tau, thr):
    """cert (R, k, HW), warp (R, k, HW, 2), P (R, k, 3, 4), sxy (R, k, 2), Pa (R, 3, 4), sa (R, 2), obs_a (n, 2): the reference's normalised
    observation of every point's cell; the points' arrays and their reference index."""
    import torch
    k = cert.shape[1]
    c = cert[ref, :, cell]                                           # (n, k)
    w = warp[ref, :, cell]                                           # (n, k, 2)
    Pp = P[ref]                                                      # (n, k, 3, 4)
    s = sxy[ref]
    ub = (w[..., 0] + 1.0) * 0.5 * wm1 * s[..., 0]
    vb = (w[..., 1] + 1.0) * 0.5 * hm1 * s[..., 1]

    def residual(X):
        p = (Pp[..., :3] * X[:, None, None, :]).sum(-1) + Pp[..., 3]
        pz = p[..., 2]
        du, dv = p[..., 0] - ub * pz, p[..., 1] - vb * pz
        return pz, du * du + dv * dv

    pz, d2 = residual(xyz)
    t = tau * pz
    winner = torch.arange(k, device=c.device)[None, :] == slot[:, None]
    cand = (pz > 0) & (d2 <= t * t) & (c > 0) & ~winner
    use = (cand | winner).to(torch.float64)
    rows = torch.stack([ub[..., None] * Pp[..., 2, :] - Pp[..., 0, :], vb[..., None] * Pp[..., 2, :] - Pp[..., 1, :]], dim=2).to(torch.float64)   # (n, k, 2, 4)
    M = torch.einsum("nk,nkri,nkrj->nij", use, rows, rows)
    Pr, sr = Pa[ref], sa[ref]
    ua = (obs_a[:, 0] + 1.0) * 0.5 * wm1 * sr[:, 0]
    va = (obs_a[:, 1] + 1.0) * 0.5 * hm1 * sr[:, 1]
    ra = torch.stack([ua[:, None] * Pr[:, 2] - Pr[:, 0], va[:, None] * Pr[:, 2] - Pr[:, 1]], dim=1).to(torch.float64)
    M = M + torch.einsum("nri,nrj->nij", ra, ra)
    v = torch.linalg.eigh(M)[1][:, :, 0]
    Xn = (v[:, :3] / v[:, 3:4]).to(torch.float32)
    pz2, d22 = residual(Xn)
    t2 = tau * pz2
    still = ((pz2 > 0) & (d22 <= t2 * t2)) | ~cand
    pa = (Pr[:, :, :3] * Xn[:, None, :]).sum(-1) + Pr[:, :, 3]
    ea = torch.hypot(pa[:, 0] / pa[:, 2] - ua, pa[:, 1] / pa[:, 2] - va)
    win = winner.to(torch.float32)
    pzw, d2w = (pz2 * win).sum(1), (d22 * win).sum(1)
    eb = torch.sqrt(d2w) / pzw
    e2 = torch.maximum(ea, eb)
    ok = cand.any(1) & still.all(1) & (pa[:, 2] > 0) & (pzw > 0) & (e2 <= thr) & torch.isfinite(Xn).all(1)
    return torch.where(ok[:, None], Xn, xyz), torch.where(ok, e2, err), ok


def operator_part(passes, out):
    import torch
    import lichtfeld_densification_plugin_amd as lfd
    from lichtfeld_densification_plugin_amd import synthetic as syn
    from lichtfeld_densification_plugin_amd.core import hip_backend as hb
    dev = torch.device("cuda:0")
    dens = hb.HipDensifier(dev)
    lib = hb.load_library()
    cams = syn.ring_cameras(185)
    dens.upload_cameras(cams)
    out("shape                                         points in   refined    kernel us (lo..hi)     HBM share   torch us (lo..hi)    torch / kernel   "
        "triangulation us   kernel / triangulation")
    verdict = True
    for label, R, k, side, wm in SHAPES:
        refs = []
        for i in range(R):
            r = (10 + 2 * i) % 185
            nbrs = syn.ring_neighbours(185, r, k)
            s = syn.synth_reference(cams, r, nbrs, side, side, wm, wm, noise_px=0.5, outlier_frac=0.05, cert_mode="tiefree", device=dev)
            refs.append(hb.ReferenceInputs(ref_cam=r, nbr_cams=nbrs, cert=[s.cert[j].clone() for j in range(k)], warp=[s.warp[j].clone() for j in range(k)],
                                           image=s.image))
        batch = hb.PreparedBatch(refs, wm, wm)
        params = hb.make_params(lfd.DensePipelineConfig(output_path="", reproj_thresh=THR))
        cap = R * side * side
        src = hb.OutputBuffers(cap, R, k, dev)
        tri = lambda: dens.launch_dense(batch, params, src)
        tri()
        dens.check_launches()
        res = src.collect()
        n_in = res.count
        xyz_out, err_out = torch.empty((cap, 3), device=dev), torch.empty((cap,), device=dev)
        status, counters = torch.zeros((cap,), dtype=torch.uint8, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
        args = (dens._ctx, C.byref(batch.c), C.byref(src.c), src.ref_offsets.data_ptr(), C.c_float(TAU), C.c_float(THR), xyz_out.data_ptr(),
                err_out.data_ptr(), status.data_ptr(), None)
        launch = lambda: lib.lfd_refine_multiview(*args)
        assert lib.lfd_refine_multiview(*(args[:-1] + (counters.data_ptr(),))) == 0
        torch.cuda.synchronize()
        n_ref = int(counters[0])
        # the torch form's inputs, prepared outside the timed region
        cert = torch.stack([torch.stack([c.reshape(-1) for c in r.cert]) for r in refs])
        warp = torch.stack([torch.stack([w.reshape(side * side, 2) for w in r.warp]) for r in refs])
        P = torch.tensor(np.stack([np.stack([np.asarray(cams[n].P, np.float32) for n in r.nbr_cams]) for r in refs]), device=dev)
        sxy = torch.tensor(np.stack([np.stack([[np.float32(cams[n].width / wm), np.float32(cams[n].height / wm)] for n in r.nbr_cams]) for r in refs]), device=dev)
        Pa = torch.tensor(np.stack([np.asarray(cams[r.ref_cam].P, np.float32) for r in refs]), device=dev)
        sa = torch.tensor(np.stack([[np.float32(cams[r.ref_cam].width / wm), np.float32(cams[r.ref_cam].height / wm)] for r in refs]), device=dev)
        off = torch.from_numpy(np.asarray(res.ref_offsets)).to(dev)
        ref_of = torch.repeat_interleave(torch.arange(R, device=dev), off[1:] - off[:-1])
        cell_l, slot_l = res.cell.long(), res.slot.long()
        axis = syn.identity_axis_torch(side, dev)
        obs_a = torch.stack([axis[cell_l % side], axis[cell_l // side]], dim=1)
        form = lambda: torch_refine(cert, warp, P, sxy, Pa, sa, obs_a, float(wm - 1), float(wm - 1), res.xyz, res.err, cell_l, slot_l, ref_of, TAU, THR)
        same = int(form()[2].sum())
        group = 10 if n_in > 1000000 else 50
        for fn in (launch, form, tri):
            timed(fn, max(2, group // 4))
        t_l, t_t, t_d = [], [], []
        for _ in range(passes):
            t_l.append(timed(launch, group))
            t_t.append(timed(form, max(2, group // 4)))
            t_d.append(timed(tri, max(2, group // 4)))
        med = lambda v: float(np.median(v))
        nbytes = n_in * (21 + 8 + 12 * (k - 1) + 17)
        clear = max(t_l) < min(t_t)
        verdict &= clear
        out(f"{label:44s} {n_in:9d} {n_ref:9d}   {med(t_l):8.1f} ({min(t_l):.1f}..{max(t_l):.1f})   {100 * nbytes / (med(t_l) * 1e-6) / HBM_PEAK:6.1f} %   "
            f"{med(t_t):8.1f} ({min(t_t):.1f}..{max(t_t):.1f})   {med(t_t) / med(t_l):6.1f} x   {med(t_d):10.1f}   {100 * med(t_l) / med(t_d):6.1f} %"
            f"      (torch refines {same}: differs by {same - n_ref}; faster beyond the spread: {'yes' if clear else 'NO'})")
        del refs, batch, src, cert, warp, res, xyz_out, err_out, status
        torch.cuda.empty_cache()
    out(f"kernel faster than the torch form at every shape by more than the spread of the passes: {'yes' if verdict else 'NO'}")
    dens.close()


def resources(out):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "lichtfeld-densification-plugin_amd", "csrc"))
    import build as lfd_build
    with tempfile.TemporaryDirectory() as tmp:
        cmd = lfd_build.compile_command("lfd_refine.hip", os.path.join(tmp, "c.o"), ["-Rpass-analysis=kernel-resource-usage"])
        err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    cur = None
    for ln in err.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = m.group(1)
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and cur and "lfd_refine" in cur:
            out(f"{cur}: {m.group(1)} {m.group(2)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--out", type=str, default=os.path.join(HERE, "r10", "refine.txt"))
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
    out(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; passes {a.passes}; support_thresh_px {TAU}, reproj_thresh {THR}")
    operator_part(a.passes, out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
