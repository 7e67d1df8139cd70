#!/usr/bin/env python3
"""The precision-weighted re-triangulation on one GPU (lfd_refine_multiview_weighted, csrc/lfd_refine.hip) against the unweighted launch
(lfd_refine_multiview) on the same points and against the same operation written in torch - the form of profiles/refine_time.py with the
precision gathers, the validity test, the camera-pixel scaling, the depth weights and the weighted M - at the same survivor counts.  What
profiles/r11/refine_weighted.txt records.

    python profiles/refine_weighted_time.py                   # the operator part (needs the GPU)
    python profiles/refine_weighted_time.py --resources       # registers / occupancy of the kernels from the compiler (needs hipcc only)

One GPU step: run it under a time limit of its own (``timeout -k 10 600 python ...``).

Method: profiles/refine_time.py's - all forms in one process, every shape warmed first, ``--passes`` passes that ALTERNATE the weighted launch,
the unweighted launch and the torch form, device events around a group of back-to-back calls, the median pass with the lowest and highest as
the spread.  Both launches go through the C entry points with their arguments built once, out of place.  Algorithmic bytes of the weighted
launch: the unweighted launch's - per input point 21 + 8 + 12 (k - 1) read, 17 written - plus 12 per view whose precision is gathered (the
winner and the k - 1 others: 12 k), over the kernel's time as a share of 8 TB/s.  The planes are the scene's TRUE precision
(synth_reference(noise_model="hetero")), valid everywhere: every point with a candidate takes the weighted rows."""
from __future__ import annotations

import argparse
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from refine_time import HBM_PEAK, SHAPES, TAU, THR, resources, timed  # noqa: E402


def torch_refine_weighted(cert, warp, prec, P, sxy, Pa, sa, obs_a, wm1, hm1, xyz, err, cell, slot, ref, tau, thr):
    """refine_time.torch_refine with prec (R, k, HW, 3): the weights of DESIGN 4.10, everything behind the f32 rows in f64."""
    import torch
    k = cert.shape[1]
    c = cert[ref, :, cell]
    w = warp[ref, :, cell]
    q = prec[ref, :, cell].to(torch.float64)                         # (n, k, 3)
    Pp = P[ref]
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
    use = cand | winner
    valid = torch.isfinite(q).all(-1) & (q[..., 0] > 0) & (q[..., 2] > 0) & (q[..., 0] * q[..., 2] - q[..., 1] * q[..., 1] > 0)
    weighted = (valid | ~use).all(1)
    s64 = s.to(torch.float64)
    w2 = 1.0 / (pz.to(torch.float64) ** 2)
    p00, p01, p11 = q[..., 0] / (s64[..., 0] ** 2), q[..., 1] / (s64[..., 0] * s64[..., 1]), q[..., 2] / (s64[..., 1] ** 2)
    ru = (ub[..., None] * Pp[..., 2, :] - Pp[..., 0, :]).to(torch.float64)      # (n, k, 4)
    rv = (vb[..., None] * Pp[..., 2, :] - Pp[..., 1, :]).to(torch.float64)
    usef = use.to(torch.float64)
    a, b, d = usef * w2 * p00, usef * w2 * p01, usef * w2 * p11
    Mw = (torch.einsum("nk,nki,nkj->nij", a, ru, ru) + torch.einsum("nk,nki,nkj->nij", b, ru, rv) + torch.einsum("nk,nki,nkj->nij", b, rv, ru)
          + torch.einsum("nk,nki,nkj->nij", d, rv, rv))
    Mu = torch.einsum("nk,nki,nkj->nij", usef, ru, ru) + torch.einsum("nk,nki,nkj->nij", usef, rv, rv)
    Pr, sr = Pa[ref], sa[ref]
    ua = (obs_a[:, 0] + 1.0) * 0.5 * wm1 * sr[:, 0]
    va = (obs_a[:, 1] + 1.0) * 0.5 * hm1 * sr[:, 1]
    ra = torch.stack([ua[:, None] * Pr[:, 2] - Pr[:, 0], va[:, None] * Pr[:, 2] - Pr[:, 1]], dim=1).to(torch.float64)
    Ma = torch.einsum("nri,nrj->nij", ra, ra)
    za = ((Pr[:, 2, :3] * xyz).sum(-1) + Pr[:, 2, 3]).to(torch.float64)
    lam = (usef * 0.5 * (p00 + p11)).sum(1)
    M = torch.where(weighted[:, None, None], Mw + (lam / (za * za))[:, None, None] * Ma, Mu + Ma)
    M = torch.where(torch.isfinite(M).all((1, 2))[:, None, None], M, torch.eye(4, dtype=torch.float64, device=M.device))
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
    out("shape                                         points in   refined  weighted   weighted us (lo..hi)   HBM share   unweighted us (lo..hi)   "
        "weighted / unweighted   torch us (lo..hi)    torch / weighted")
    verdict = True
    for label, R, k, side, wm in SHAPES:
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
        src = hb.OutputBuffers(cap, R, k, dev)
        dens.launch_dense(batch, params, src)
        dens.check_launches()
        res = src.collect()
        n_in = res.count
        xyz_out, err_out = torch.empty((cap, 3), device=dev), torch.empty((cap,), device=dev)
        status, counters = torch.zeros((cap,), dtype=torch.uint8, device=dev), torch.zeros(3, dtype=torch.int64, device=dev)
        args = (dens._ctx, C.byref(batch.c), C.byref(src.c), src.ref_offsets.data_ptr(), C.c_float(TAU), C.c_float(THR), xyz_out.data_ptr(),
                err_out.data_ptr(), status.data_ptr(), None)
        table = C.cast(batch.precision, C.c_void_p)
        weighted = lambda: lib.lfd_refine_multiview_weighted(*args, table)
        plain = lambda: lib.lfd_refine_multiview(*args)
        assert lib.lfd_refine_multiview_weighted(*(args[:-1] + (counters.data_ptr(), table))) == 0
        torch.cuda.synchronize()
        n_ref, n_w = int(counters[0]), int(counters[2])
        cert = torch.stack([torch.stack([c.reshape(-1) for c in r.cert]) for r in refs])
        warp = torch.stack([torch.stack([w.reshape(side * side, 2) for w in r.warp]) for r in refs])
        prec = torch.stack([torch.stack([q.reshape(side * side, 3) for q in r.precision]) for r in refs])
        P = torch.tensor(np.stack([np.stack([np.asarray(cams[n].P, np.float32) for n in r.nbr_cams]) for r in refs]), device=dev)
        sxy = torch.tensor(np.stack([np.stack([[np.float32(cams[n].width / wm), np.float32(cams[n].height / wm)] for n in r.nbr_cams]) for r in refs]), device=dev)
        Pa = torch.tensor(np.stack([np.asarray(cams[r.ref_cam].P, np.float32) for r in refs]), device=dev)
        sa = torch.tensor(np.stack([[np.float32(cams[r.ref_cam].width / wm), np.float32(cams[r.ref_cam].height / wm)] for r in refs]), device=dev)
        off = torch.from_numpy(np.asarray(res.ref_offsets)).to(dev)
        ref_of = torch.repeat_interleave(torch.arange(R, device=dev), off[1:] - off[:-1])
        cell_l, slot_l = res.cell.long(), res.slot.long()
        axis = syn.identity_axis_torch(side, dev)
        obs_a = torch.stack([axis[cell_l % side], axis[cell_l // side]], dim=1)
        form = lambda: torch_refine_weighted(cert, warp, prec, P, sxy, Pa, sa, obs_a, float(wm - 1), float(wm - 1), res.xyz, res.err, cell_l, slot_l,
                                             ref_of, TAU, THR)
        same = int(form()[2].sum())
        group = 10 if n_in > 1000000 else 50
        for fn in (weighted, plain, form):
            timed(fn, max(2, group // 4))
        t_w, t_u, t_t = [], [], []
        for _ in range(passes):
            t_w.append(timed(weighted, group))
            t_u.append(timed(plain, group))
            t_t.append(timed(form, max(2, group // 4)))
        med = lambda v: float(np.median(v))
        nbytes = n_in * (21 + 8 + 12 * (k - 1) + 17 + 12 * k)
        clear = max(t_w) < min(t_t)
        verdict &= clear
        out(f"{label:44s} {n_in:9d} {n_ref:9d} {n_w:9d}   {med(t_w):8.1f} ({min(t_w):.1f}..{max(t_w):.1f})   "
            f"{100 * nbytes / (med(t_w) * 1e-6) / HBM_PEAK:6.1f} %   {med(t_u):8.1f} ({min(t_u):.1f}..{max(t_u):.1f})   {med(t_w) / med(t_u):6.2f} x   "
            f"{med(t_t):8.1f} ({min(t_t):.1f}..{max(t_t):.1f})   {med(t_t) / med(t_w):6.1f} x"
            f"      (torch refines {same}: differs by {same - n_ref}; faster than torch beyond the spread: {'yes' if clear else 'NO'})")
        del refs, batch, src, cert, warp, prec, res, xyz_out, err_out, status
        torch.cuda.empty_cache()
    out(f"weighted kernel faster than the torch form at every shape by more than the spread of the passes: {'yes' if verdict else 'NO'}")
    dens.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--out", type=str, default=os.path.join(HERE, "r11", "refine_weighted.txt"))
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
