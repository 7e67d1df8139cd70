#!/usr/bin/env python3
"""The depth-uncertainty gate on one GPU (lfd_depth_sigma_filter, csrc/lfd_sigma.hip: three launches) in the winner-only form and in the
candidate form (with the status of lfd_refine_multiview_weighted over the same points), against the same operation written in torch, at the
survivor counts of profiles/refine_time.py's shapes.  What profiles/r12/depth_sigma.txt records.

    python profiles/depth_sigma_time.py                   # the operator part (needs the GPU)
    python profiles/depth_sigma_time.py --resources       # registers / occupancy of the kernels from the compiler (needs hipcc only)

One GPU step: run it under a time limit of its own (``timeout -k 10 600 python ...``).

Method: profiles/refine_time.py's - all forms in one process, every shape warmed first, ``--passes`` passes that ALTERNATE the arms, device
events around a group of back-to-back calls, the median pass with the lowest and highest as the spread.  The calls go through the C entry
point with their arguments built once; the gate sits at the median sigma, so half of the points are moved.  Algorithmic bytes per input point:
17 of its own fields read (cell 4, slot 1, xyz 12), 12 of the winner's precision, 4 + 1 written (sigma, keep byte), 1 + 4 read again by the
scatter, and per KEPT point 33 read + 33 written + 4 of sigma_rel_out; the candidate form adds the status byte and, per accepted point, 24
(certainty 4, warp 8, precision 12) per other neighbour.  Over the three launches' time as a share of 8 TB/s, and the time as a share of the
lfd_triangulate_dense call that made the points, timed in the same run."""
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
from refine_time import HBM_PEAK, SHAPES, TAU, THR, timed  # noqa: E402


def torch_sigma(cert, warp, prec, P, sxy, CA, wm1, hm1, xyz, cell, slot, ref, accepted, tau):
    """sigma_rel of DESIGN 4.11 in torch, f64 behind the f32 inputs.  cert (R, k, HW), warp (R, k, HW, 2), prec (R, k, HW, 3), P (R, k, 3, 4),
    sxy (R, k, 2), CA (R, 3); accepted: None (winner only) or (n,) bool."""
    import torch
    k = cert.shape[1]
    Pp = P[ref].to(torch.float64)                                    # (n, k, 3, 4)
    X = xyz.to(torch.float64)
    D = X - CA[ref].to(torch.float64)
    p = (Pp[..., :3] * X[:, None, None, :]).sum(-1) + Pp[..., 3]
    h = (Pp[..., :3] * D[:, None, None, :]).sum(-1)
    pz = p[..., 2]
    gx = h[..., 0] / pz - p[..., 0] * h[..., 2] / (pz * pz)
    gy = h[..., 1] / pz - p[..., 1] * h[..., 2] / (pz * pz)
    q = prec[ref, :, cell].to(torch.float64)
    s = sxy[ref].to(torch.float64)
    p00, p01, p11 = q[..., 0] / (s[..., 0] ** 2), q[..., 1] / (s[..., 0] * s[..., 1]), q[..., 2] / (s[..., 1] ** 2)
    info = p00 * gx * gx + 2.0 * p01 * gx * gy + p11 * gy * gy
    valid = torch.isfinite(q).all(-1) & (q[..., 0] > 0) & (q[..., 2] > 0) & (q[..., 0] * q[..., 2] - q[..., 1] * q[..., 1] > 0)
    use = torch.arange(k, device=cell.device)[None, :] == slot[:, None]
    if accepted is not None:
        c = cert[ref, :, cell]
        w = warp[ref, :, cell]
        s32 = sxy[ref]
        ub = (w[..., 0] + 1.0) * 0.5 * wm1 * s32[..., 0]
        vb = (w[..., 1] + 1.0) * 0.5 * hm1 * s32[..., 1]
        P32 = P[ref]
        p32 = (P32[..., :3] * xyz[:, None, None, :]).sum(-1) + P32[..., 3]
        z = p32[..., 2]
        du, dv = p32[..., 0] - ub * z, p32[..., 1] - vb * z
        t = tau * z
        use = use | ((z > 0) & (du * du + dv * dv <= t * t) & (c > 0) & ~use & accepted[:, None])
    total = torch.where(use & valid & (pz > 0) & torch.isfinite(info), info, torch.zeros_like(info)).sum(1)
    return torch.where(total > 0, 1.0 / torch.sqrt(total), torch.full_like(total, float("inf"))).to(torch.float32)


def torch_gate(sigma, mx, xyz, rgb, err, cell, slot):
    keep = sigma <= mx
    return xyz[keep], rgb[keep], err[keep], cell[keep], slot[keep], sigma[keep]


def operator_part(passes, out, shapes):
    import torch
    import lichtfeld_densification_plugin_amd as lfd
    from lichtfeld_densification_plugin_amd import synthetic as syn
    from lichtfeld_densification_plugin_amd.core import hip_backend as hb
    dev = torch.device("cuda:0")
    dens = hb.HipDensifier(dev)
    lib = hb.load_library()
    cams = syn.ring_cameras(185)
    dens.upload_cameras(cams)
    out("shape / form                                            points in      kept   accepted   gate us (lo..hi)   HBM share   share of dense call   "
        "torch us (lo..hi)   torch / gate")
    verdict = True
    for label, R, k, side, wm in SHAPES[:shapes]:
        refs = []
        for i in range(R):
            r = (10 + 2 * i) % 185
            nbrs = syn.ring_neighbours(185, r, k)
            s = syn.synth_reference(cams, r, nbrs, side, side, wm, wm, noise_px=0.5, outlier_frac=0.05, cert_mode="tiefree", device=dev,
                                    noise_model="hetero")
            refs.append(hb.ReferenceInputs(ref_cam=r, nbr_cams=nbrs, cert=[s.cert[j].clone() for j in range(k)], warp=[s.warp[j].clone() for j in range(k)],
                                           image=s.image, precision=[s.precision[j].clone() for j in range(k)]))
        batch = hb.PreparedBatch(refs, wm, wm)
        params = hb.make_params(lfd.DensePipelineConfig(output_path="", reproj_thresh=THR))
        cap = R * side * side
        src, dst = hb.OutputBuffers(cap, R, k, dev), hb.OutputBuffers(cap, R, k, dev)
        dense = lambda: dens.launch_dense(batch, params, src)
        dense()
        dens.check_launches()
        # the refined points and their status (the candidate form's input), in place
        status = torch.zeros((cap,), dtype=torch.uint8, device=dev)
        table = C.cast(batch.precision, C.c_void_p)
        assert lib.lfd_refine_multiview_weighted(dens._ctx, C.byref(batch.c), C.byref(src.c), src.ref_offsets.data_ptr(), C.c_float(TAU), C.c_float(THR),
                                                 src.c.xyz, src.c.err, status.data_ptr(), None, table) == 0
        res = src.collect()
        n_in = res.count
        sigma, sigma_out = torch.empty((cap,), device=dev), torch.empty((cap,), device=dev)

        def gate(st, mx):
            return lambda: lib.lfd_depth_sigma_filter(dens._ctx, C.byref(batch.c), C.byref(src.c), src.ref_offsets.data_ptr(), table, C.c_float(0.0),
                                                      st.data_ptr() if st is not None else None, C.c_float(TAU if st is not None else 0.0),
                                                      C.c_float(mx), C.byref(dst.c), dst.ref_offsets.data_ptr(), dst.seg_counts.data_ptr(),
                                                      sigma.data_ptr(), sigma_out.data_ptr())

        cert = torch.stack([torch.stack([c.reshape(-1) for c in r.cert]) for r in refs])
        warp = torch.stack([torch.stack([w.reshape(side * side, 2) for w in r.warp]) for r in refs])
        prec = torch.stack([torch.stack([q.reshape(side * side, 3) for q in r.precision]) for r in refs])
        P = torch.tensor(np.stack([np.stack([np.asarray(cams[n].P, np.float32) for n in r.nbr_cams]) for r in refs]), device=dev)
        sxy = torch.tensor(np.stack([np.stack([[np.float32(cams[n].width / wm), np.float32(cams[n].height / wm)] for n in r.nbr_cams]) for r in refs]), device=dev)
        CA = torch.tensor(np.stack([np.asarray(cams[r.ref_cam].C, np.float32) for r in refs]), device=dev)
        off = torch.from_numpy(np.asarray(res.ref_offsets)).to(dev)
        ref_of = torch.repeat_interleave(torch.arange(R, device=dev), off[1:] - off[:-1])
        cell_l, slot_l = res.cell.long(), res.slot.long()
        acc = (status[:n_in] & 0x80) != 0
        group = 10 if n_in > 1000000 else 50
        t_dense = float(np.median([timed(dense, max(2, group // 4)) for _ in range(3)]))
        # (the timed dense launches overwrote the refined points with the two-view ones: the gate's traffic does not depend on which they are)
        for form, st, accepted in (("winner only", None, None), ("with candidates", status, acc)):
            assert gate(st, 0.0)() == 0
            torch.cuda.synchronize()
            fin = sigma[:n_in][torch.isfinite(sigma[:n_in])]
            mx = float(fin.median())
            fn = gate(st, mx)
            assert fn() == 0
            torch.cuda.synchronize()
            kept = int(dst.ref_offsets[-1])
            form_t = lambda: torch_gate(torch_sigma(cert, warp, prec, P, sxy, CA, float(wm - 1), float(wm - 1), res.xyz, cell_l, slot_l, ref_of,
                                                    accepted, TAU), mx, res.xyz, res.rgb, res.err, res.cell, res.slot)
            same = int(form_t()[0].shape[0])
            for f in (fn, form_t):
                timed(f, max(2, group // 4))
            t_g, t_t = [], []
            for _ in range(passes):
                t_g.append(timed(fn, group))
                t_t.append(timed(form_t, max(2, group // 4)))
            med = lambda v: float(np.median(v))
            n_acc = int(acc.sum()) if accepted is not None else 0
            nbytes = n_in * (17 + 12 + 5 + 5) + kept * 70 + (n_in + n_acc * 24 * (k - 1) if accepted is not None else 0)
            clear = max(t_g) < min(t_t)
            verdict &= clear
            out(f"{label + ', ' + form:54s} {n_in:9d} {kept:9d} {n_acc:9d}   {med(t_g):8.1f} ({min(t_g):.1f}..{max(t_g):.1f})   "
                f"{100 * nbytes / (med(t_g) * 1e-6) / HBM_PEAK:6.1f} %   {100 * med(t_g) / t_dense:6.1f} % of {t_dense:.1f} us   "
                f"{med(t_t):8.1f} ({min(t_t):.1f}..{max(t_t):.1f})   {med(t_t) / med(t_g):6.1f} x"
                f"      (torch keeps {same}: differs by {same - kept}; faster than torch beyond the spread: {'yes' if clear else 'NO'})")
        del refs, batch, src, dst, cert, warp, prec, res, sigma, sigma_out, status
        torch.cuda.empty_cache()
    out(f"gate faster than the torch form at every shape and form by more than the spread of the passes: {'yes' if verdict else 'NO'}")
    dens.close()


def resources(out):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "lichtfeld-densification-plugin_amd", "csrc"))
    import build as lfd_build
    with tempfile.TemporaryDirectory() as tmp:
        cmd = lfd_build.compile_command("lfd_sigma.hip", os.path.join(tmp, "c.o"), ["-Rpass-analysis=kernel-resource-usage"])
        err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    cur = None
    for ln in err.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = m.group(1)
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and cur and "lfd_sigma" in cur:
            out(f"{cur}: {m.group(1)} {m.group(2)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--shapes", type=int, default=len(SHAPES), help="the first N shapes only")
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--out", type=str, default=os.path.join(HERE, "r12", "depth_sigma.txt"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(HERE))
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    if a.resources:
        resources(out)
    else:
        import torch
        out(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; passes {a.passes}; support_thresh_px {TAU}, reproj_thresh {THR}")
        operator_part(a.passes, out, a.shapes)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out if not a.resources else os.path.join(os.path.dirname(a.out), "depth_sigma_resources.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
