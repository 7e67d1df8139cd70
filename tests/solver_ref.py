"""The rules the triangulation solver (csrc/lfd_geometry.hpp::lfd_null_vector_rows) is judged by against the exact answers of
tests/golden/g19_solver_exact.npz (made by tests/golden/make_solver_exact_fixture.py), for the host and the GPU tests alike - and the
re-triangulation's solver (csrc/lfd_refine.hpp::lfd_null_vector_sym) by the same rules, on the same matrices and on those of
tests/golden/g21_refine_solver_exact.npz, through lfd_refine_multiview[_weighted] (run_refine / check_refine at the end of this file).

    r    sigma4 / sigma3 of the exact singular values (its class is stored: the sigmas are f32)
    v    the exact unit null vector
    d    the unit direction under test: c/|c| on the host; (x, y, z, 1) normalised on the device, (x, y, z, 0) normalised where the
         guard branch (|v3|/|v| < 1e-12: X = c / (1e-12 |c|)) is expected

Direction, min(|d - v|, |d + v|): 1e-8 for r < 0.1, 2e-6 for 0.1 <= r < 0.9 (tests/test_host_helpers.py's bounds), and
2e-6 * 0.19 / (1 - r^2) for 0.9 <= r <= 0.999: the same bound continued with the eigenvector gap mu3 - mu4 ~ 1 - r^2, continuous at 0.9.
Residual, every finite case: |A d| <= sigma4 (1 + 1e-6) + 1e-9 sigma1 (tests/test_properties.py's rule); for r > 0.999, where no
direction is asked for, sigma3 instead of sigma4: the result lies in the two-dimensional near-null space.
The device adds 2^-23 (direction) and 2^-23 sigma1 (residual) for the f32 rounding of the three output coordinates.
Cases with |v3|/|v| within a factor 2 of the guard's 1e-12 may take either branch: finiteness only.
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
F32_EPS = 2.0 ** -23
GUARD = 1e-12
MAX_SOLVES = 3 + 8 * 4            # LFD_NULLVEC_MAXIT solves in each of LFD_NULLVEC_PASSES passes, on top of pass 0's first three


def load_fixture():
    """g19 as a dict, with family M's matrices put together (those taken from g13 are stored there only)."""
    g19 = dict(np.load(os.path.join(GOLDEN, "g19_solver_exact.npz")))
    g13 = np.load(os.path.join(GOLDEN, "g13_null_vector.npz"))
    src = g19["M_g13"]
    A = np.empty((src.size, 4, 4), np.float32)
    A[src >= 0] = g13["A"][src[src >= 0]]
    A[src < 0] = g19.pop("M_A7")
    assert ((src < 0) == (g19["M_kind"] == 7)).all()
    g19["M_A"] = A
    g19["G_idx"] = np.nonzero(g13["kind"] <= 4)[0]
    g19["G_A"] = g13["A"][g19["G_idx"]]
    assert g19["G_idx"].size == int(g19["G_n"])
    return g19


def w_fraction(v):
    return abs(float(v[3])) / float(np.linalg.norm(v))


def in_guard_band(v):
    return GUARD / 2.0 <= w_fraction(v) <= GUARD * 2.0


def guard_expected(v):
    return w_fraction(v) < GUARD / 2.0


def direction_bound(cls, sigma):
    """None where no direction is asked for (r > 0.999, or no finite answer)."""
    if cls == 0:
        return 1e-8
    if cls == 1:
        return 2e-6
    if cls == 2:
        r = float(sigma[3]) / float(sigma[2])
        return 2e-6 * 0.19 / (1.0 - r * r)
    return None


def judge(A, sigma, cls, v, d, device=False):
    """The rules for one finite case (cls >= 0); ``d``: the direction under test (any length).  Returns (what failed or None, direction error or
    None, residual / bound)."""
    d = np.asarray(d, np.float64)
    if not np.isfinite(d).all() or not np.any(d):
        return "not finite", None, None
    if in_guard_band(v):
        return None, None, None
    d = d / np.abs(d).max()                # (first: the solver's c may be too large to square)
    d = d / np.linalg.norm(d)
    s = sigma.astype(np.float64)
    err, fail = None, None
    bound = direction_bound(int(cls), sigma)
    if bound is not None:
        err = float(min(np.linalg.norm(d - v), np.linalg.norm(d + v)))
        if not err <= bound + (F32_EPS if device else 0.0):
            fail = f"direction {err:.3e} > {bound:.3e} (r = {s[3] / s[2]:.6f})"
    res = float(np.linalg.norm(A.astype(np.float64) @ d))
    rb = (s[3] if cls <= 2 else s[2]) * (1.0 + 1e-6) + 1e-9 * s[0] + (F32_EPS * s[0] if device else 0.0)
    if not res <= rb:
        fail = (fail + "; " if fail else "") + f"residual {res:.6e} > {rb:.6e} (sigma {s.tolist()})"
    return fail, err, res / rb if rb > 0 else 0.0


def device_direction(xyz, v, cls):
    """(x, y, z, 1), or (x, y, z, 0) where the guard branch is expected.  Where no unique v exists (r > 0.999, rank <= 2: class 3) the exact answer
    cannot say which branch is due; the point itself does - the guard branch returns |X| = 1e12, and a common-branch X that long has a w of
    1e-12 |X| or less, which (x, y, z, 1) and (x, y, z, 0) agree on far below the f32 rounding."""
    if cls == 3:
        w = 0.0 if float(np.linalg.norm(np.asarray(xyz, np.float64))) > 1e11 else 1.0
    else:
        w = 0.0 if guard_expected(v) else 1.0
    return np.array([float(xyz[0]), float(xyz[1]), float(xyz[2]), w])


def host_guard_branch(c):
    """lfd_eval_correspondence's test on the solver's c: c3^2 < 1e-24 |c|^2."""
    c = np.asarray(c, np.float64)
    with np.errstate(all="ignore"):        # (evaluated as the code does: squares that overflow give Inf < Inf, the common branch)
        return bool(c[3] * c[3] < 1e-24 * (c[0] * c[0] + c[1] * c[1] + c[2] * c[2] + c[3] * c[3]))


def ulp_distance(a, b):
    """Distance in representable f32 values between two finite arrays."""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


# ---- feeding the cases to the entry points ---------------------------------------------------------------------------------------------
S_GRID = 32                      # family S: H = W = w_match = h_match
M_GRID, M_MATCH = 1, 2           # family M: one cell, the smallest match image the entry points accept


def scene_s(fx):
    """(cams, ref index, neighbour indices, cert planes [3 x (H,W)], warp plane (H,W,4)) of family S.  The same warp plane serves every slot; the
    slot that the fixture names wins the cell through its certainty."""
    from lichtfeld_densification_plugin_amd import synthetic
    cams = synthetic.ring_cameras(60, seed=0)
    ids = [int(i) for i in fx["S_cams"]]
    slot = fx["S_slot"].reshape(S_GRID, S_GRID)
    cert = [np.where(slot == j, 0.9, 0.3).astype(np.float32) for j in range(3)]
    warp = np.ascontiguousarray(fx["S_corr"].reshape(S_GRID, S_GRID, 4))
    return cams, ids[0], ids[1:], cert, warp


def injected_cameras(A, uid=0, ref_scale=1.0):
    """Reference and neighbour cameras whose DLT rows at pixel 0 (warp value -1 on all four channels) are the rows of A exactly, a pair per
    camera (A: 2n x 4, n cameras, the reference first): rows of -A as the first two rows of P, third row (0, 0, 0, 1) - the depth of X is
    X[3].  ``ref_scale``: a power of two that the reference's two rows are multiplied by (the weighted re-triangulation, see run_refine)."""
    import lichtfeld_densification_plugin_amd as lfd
    A = np.asarray(A, np.float32).reshape(-1, 4)
    assert A.shape[0] % 2 == 0 and A.shape[0] >= 2
    out = []
    for h in range(A.shape[0] // 2):
        P = np.zeros((3, 4), np.float32)
        with np.errstate(all="ignore"):
            P[0], P[1], P[2, 3] = -A[2 * h], -A[2 * h + 1], 1.0
            if h == 0 and ref_scale != 1.0:
                P[:2] *= np.float32(ref_scale)
        out.append(lfd.CameraRecord(uid=uid + h, image_path="", width=M_MATCH, height=M_MATCH, K=np.eye(3, dtype=np.float32),
                                    R=np.eye(3, dtype=np.float32), t=np.zeros((3, 1), np.float32), P=P, C=np.zeros(3, np.float32)))
    return out


def no_filter_params():
    import lichtfeld_densification_plugin_amd as lfd
    from lichtfeld_densification_plugin_amd.core import hip_backend as hb
    return hb.make_params(lfd.DensePipelineConfig(output_path="", no_filter=True))


def run_family_s(dens, fx, torch, device):
    """(dense, indexed with every cell selected) of family S on ``dens`` (HipDensifier or its CPU twin)."""
    from lichtfeld_densification_plugin_amd.core import hip_backend as hb
    cams, ref, nbrs, cert, warp = scene_s(fx)
    dens.upload_cameras(cams)
    w = torch.from_numpy(warp).to(device)
    r = hb.ReferenceInputs(ref_cam=ref, nbr_cams=nbrs, cert=[torch.from_numpy(c).to(device) for c in cert], warp=[w, w, w],
                           image=torch.zeros((S_GRID, S_GRID, 3), dtype=torch.uint8, device=device))
    batch = hb.PreparedBatch([r], S_GRID, S_GRID)
    params = no_filter_params()
    dense = dens.triangulate_dense(batch, params)
    sel = torch.arange(S_GRID * S_GRID, dtype=torch.int64)
    idx = dens.triangulate_indexed(batch, params, sel if device.type == "cpu" else sel.to(device), [0, S_GRID * S_GRID])
    return dense, idx


def run_family_m(dens, fx, torch, device, batch_refs=102):
    """Family M through triangulate_indexed, ``batch_refs`` references (one matrix, one cell, one neighbour each) per launch.
    Returns (emitted[n] bool, xyz[n,3] f32 - rows of cases that were not emitted are NaN)."""
    from lichtfeld_densification_plugin_amd.core import hip_backend as hb
    A = fx["M_A"]
    n = A.shape[0]
    cams = []
    for i in range(n):
        cams += injected_cameras(A[i], uid=2 * i)
    dens.upload_cameras(cams)
    cert = torch.full((M_GRID, M_GRID), 0.9, dtype=torch.float32, device=device)
    warp = torch.full((M_GRID, M_GRID, 4), -1.0, dtype=torch.float32, device=device)
    image = torch.zeros((M_MATCH, M_MATCH, 3), dtype=torch.uint8, device=device)
    params = no_filter_params()
    emitted, xyz = np.zeros(n, bool), np.full((n, 3), np.nan, np.float32)
    for lo in range(0, n, batch_refs):
        hi = min(n, lo + batch_refs)
        refs = [hb.ReferenceInputs(ref_cam=2 * i, nbr_cams=[2 * i + 1], cert=[cert], warp=[warp], image=image) for i in range(lo, hi)]
        batch = hb.PreparedBatch(refs, M_MATCH, M_MATCH)
        sel = torch.zeros(hi - lo, dtype=torch.int64)
        out = dens.triangulate_indexed(batch, params, sel if device.type == "cpu" else sel.to(device), list(range(hi - lo + 1)))
        offs = np.asarray(out.ref_offsets, np.int64)
        got = out.xyz.cpu().numpy()
        for i in range(lo, hi):
            a, b = int(offs[i - lo]), int(offs[i - lo + 1])
            assert b - a in (0, 1)
            if b > a:
                emitted[i], xyz[i] = True, got[a]
    return emitted, xyz


# ---- feeding chosen matrices to the multi-view re-triangulation (lfd_refine_multiview[_weighted], csrc/lfd_refine.hpp) -------------------------
# Gates wide open but finite: with them every finite case away from the w -> 0 guard has to come back accepted, so no gate can hide a wrong vector.
REFINE_TAU, REFINE_THR = 1e15, 1e30
REFINE_LAM = 4.0                 # the weighted variant's lam (the sum of the neighbours' mean precisions): a power of four
ACCEPTED, WEIGHTED = 0x80, 0x40


def refine_cases():
    """The cases of the re-triangulation tests, family -> dict(A[N, 2n, 4], sigma, cls, v, nopivot, names): ``G`` every g13 matrix of
    kinds 0..4 and ``M`` g19's family M (two views), ``V3`` and ``V4`` the three- and four-view matrices of g21_refine_solver_exact.npz.
    ``names``: what a failure is reported under (G: the g13 index)."""
    fx = load_fixture()
    g21 = np.load(os.path.join(GOLDEN, "g21_refine_solver_exact.npz"))
    out = {}
    for fam in "GM":
        n = fx[fam + "_A"].shape[0]
        out[fam] = dict(A=fx[fam + "_A"], sigma=fx[fam + "_sigma"], cls=fx[fam + "_cls"], v=fx[fam + "_v"],
                        nopivot=fx["M_nopivot"] if fam == "M" else np.zeros(n, bool), names=fx["G_idx"] if fam == "G" else np.arange(n))
    for fam in ("V3", "V4"):
        n = g21[fam + "_A"].shape[0]
        out[fam] = dict(A=g21[fam + "_A"], sigma=g21[fam + "_sigma"], cls=g21[fam + "_cls"], v=g21[fam + "_v"], nopivot=g21[fam + "_nopivot"],
                        names=np.arange(n))
    return out


def refine_subset(cases):
    """What the wider kernels (k = 5, 9) are given: g13's classes 1..3, family M and g21 whole."""
    keep = np.isin(cases["G"]["cls"], (1, 2, 3))
    out = dict(cases)
    out["G"] = {key: val[keep] for key, val in cases["G"].items()}
    return out


def refine_slots(n_views, k, winner):
    """Slots of the live neighbours besides the winner, ascending: the n_views - 2 candidates that carry rows of A, then the null view.  They are
    spread over the free slots, so that with k = 9 slots beyond the eighth are live."""
    free = [j for j in range(k) if j != winner]
    others = n_views - 1
    assert len(free) >= others >= 1
    pick = [free[-1]] if others == 1 else [free[int(round(t))] for t in np.linspace(0, len(free) - 1, others)]
    assert len(set(pick)) == others and pick == sorted(pick)
    return pick


def refine_winner(i, k):
    """The winning slot of case i: first, middle and last slot in turn."""
    return (0, k // 2, k - 1)[i % 3]


def run_refine(dens, A, torch, device, precision, k=None, batch_refs=100):
    """The matrices A[N, 2n, 4] (n = 2, 3 or 4 views) through ``dens.refine_multiview`` (HipDensifier or its CPU twin), one reference with one
    cell and one hand-made input point (xyz = 0, err = 0) each, ``batch_refs`` references per launch, gates REFINE_TAU / REFINE_THR.

    The reference carries rows 0-1, the winning slot rows 2-3, n - 2 further live slots the other row pairs (the routine's view order: reference,
    winner, candidates by ascending slot) and one more live slot - the null view - has zero rows: it makes every point a candidate and adds
    exact zeros, so M = A^T A.  The other slots of the ``k`` (default n) are dead (certainty 0).  Every view sees pixel 0 with depth exactly 1, and
    the input point (0, 0, 0) is within REFINE_TAU of every view.

    ``precision``: the weighted variant on the same M.  Every view that carries rows has the plane (1, 0, 1), the null view (p, 0, p) with
    p = REFINE_LAM - (n - 1), so lam = REFINE_LAM = 4, and the reference is injected with its rows halved (exact in f32): it enters with weight
    lam, 4 (A[0:2] / 2)^T (A[0:2] / 2).  A case whose halved rows would not be exact (underflow) is flagged ``skipped``.  Dead slots carry NaN
    planes.

    Returns dict(status[N] u8, xyz[N, 3] f32, err[N] f32, skipped[N] bool, n_extra: n - 1)."""
    import lichtfeld_densification_plugin_amd as lfd
    from lichtfeld_densification_plugin_amd.core import hip_backend as hb
    A = np.asarray(A, np.float32)
    N, n_views = A.shape[0], A.shape[1] // 2
    k = n_views if k is None else k
    scale = 1.0 / np.sqrt(REFINE_LAM) if precision else 1.0
    with np.errstate(all="ignore"):
        ref_rows = A[:, :2].astype(np.float32)
        back = (ref_rows * np.float32(scale)) / np.float32(scale)
    skipped = ~((back == ref_rows) | ~np.isfinite(ref_rows)).all(axis=(1, 2))
    t32 = lambda v, shape: torch.full(shape, v, dtype=torch.float32, device=device)
    live, dead, warp = t32(0.9, (M_GRID, M_GRID)), t32(0.0, (M_GRID, M_GRID)), t32(-1.0, (M_GRID, M_GRID, 4))
    image = torch.zeros((M_MATCH, M_MATCH, 3), dtype=torch.uint8, device=device)
    plane = lambda p: torch.tensor([p, 0.0, p], dtype=torch.float32, device=device).reshape(M_GRID, M_GRID, 3).contiguous()
    one, null_plane, nan_plane = plane(1.0), plane(REFINE_LAM - (n_views - 1)), plane(float("nan"))
    status, xyz, err = np.zeros(N, np.uint8), np.zeros((N, 3), np.float32), np.zeros(N, np.float32)
    for lo in range(0, N, batch_refs):
        hi = min(N, lo + batch_refs)
        cams = injected_cameras(np.zeros((2, 4), np.float32))          # camera 0: zero rows - the null view and every dead slot
        refs, slots = [], []
        for i in range(lo, hi):
            s = refine_winner(i, k)
            others = refine_slots(n_views, k, s)
            mine = injected_cameras(A[i], uid=len(cams), ref_scale=scale)
            base = len(cams)
            cams += mine
            nbr, cert, prec = [0] * k, [dead] * k, [nan_plane] * k
            nbr[s], cert[s], prec[s] = base + 1, live, one
            for c, j in enumerate(others[:-1]):
                nbr[j], cert[j], prec[j] = base + 2 + c, live, one
            cert[others[-1]], prec[others[-1]] = live, null_plane
            refs.append(hb.ReferenceInputs(ref_cam=base, nbr_cams=nbr, cert=cert, warp=[warp] * k, image=image, precision=prec if precision else None))
            slots.append(s)
        dens.upload_cameras(cams)
        batch = hb.PreparedBatch(refs, M_MATCH, M_MATCH)
        m = hi - lo
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=device)
        pts = hb.TriangulationOutput(xyz=z((m, 3), torch.float32), rgb=z((m, 3), torch.float32), err=z((m,), torch.float32), cell=z((m,), torch.int32),
                                     slot=torch.tensor(slots, dtype=torch.uint8, device=device), ref_offsets=np.arange(m + 1, dtype=np.int64),
                                     seg_counts=np.zeros((m, k), np.int32))
        res, st = dens.refine_multiview(batch, pts, REFINE_TAU, REFINE_THR, with_status=True, precision=precision)
        status[lo:hi], xyz[lo:hi], err[lo:hi] = st.cpu().numpy(), res.xyz.cpu().numpy(), res.err.cpu().numpy()
    return dict(status=status, xyz=xyz, err=err, skipped=skipped, n_extra=n_views - 1)


def check_refine(out, A, sigma, cls, v, nopivot, weighted, names=None):
    """The rules for what run_refine returned for the cases (A, sigma, cls, v; ``nopivot``: bool per case, see the fixture's M_nopivot).

      every case            a point that is not accepted keeps the bits of its xyz and err (here: zeros)
      non-finite A          not accepted
      finite A              the status carries n_extra (and WEIGHTED when ``weighted``): the candidates are counted before the solve
      ... guard expected    (|v3|/|v| < 1e-12 / 2) not accepted
      ... guard band        finite
      ... ``nopivot``       may come back unaccepted; an accepted one is judged
      ... every other       ACCEPTED, and judge(..., device=True) on (x, y, z, 1): the output is f32 on the host as well
    Returns (failed [(name, what)], counts dict)."""
    failed, counts = [], dict(judged=0, guard=0, band=0, nonfinite=0, nopivot_unaccepted=0, skipped=int(out["skipped"].sum()))
    want = out["n_extra"] | (WEIGHTED if weighted else 0)
    for i in range(A.shape[0]):
        if out["skipped"][i]:
            continue
        name = int(names[i]) if names is not None else i
        st, xyz, err = int(out["status"][i]), out["xyz"][i], out["err"][i]
        accepted = bool(st & ACCEPTED)
        if not accepted and (xyz.view(np.uint32).any() or err.view(np.uint32).any()):
            failed.append((name, f"not accepted (status {st:#x}) but moved: {xyz} {err}"))
            continue
        if cls[i] < 0:
            counts["nonfinite"] += 1
            if accepted:
                failed.append((name, f"non-finite matrix accepted (status {st:#x})"))
            continue
        if (st & 0x7f) != want:
            failed.append((name, f"status {st:#x}, expected {want:#x} beside ACCEPTED"))
            continue
        unique = cls[i] != 3          # (class 3 - r > 0.999, rank <= 2 - has no unique v that could say whether the guard is due: it has to be accepted)
        if unique and guard_expected(v[i]):
            counts["guard"] += 1
            if accepted:
                failed.append((name, f"guard expected but accepted: {xyz}"))
            continue
        if unique and in_guard_band(v[i]):
            counts["band"] += 1
            if not (np.isfinite(xyz).all() and np.isfinite(err)):
                failed.append((name, f"guard band, not finite: {xyz} {err}"))
            continue
        if not accepted:
            if nopivot[i]:
                counts["nopivot_unaccepted"] += 1
            else:
                failed.append((name, f"finite, away from the guard, not accepted (status {st:#x})"))
            continue
        fail, _, _ = judge(A[i], sigma[i], cls[i], v[i], np.array([float(xyz[0]), float(xyz[1]), float(xyz[2]), 1.0]), device=True)
        counts["judged"] += 1
        if fail:
            failed.append((name, fail))
    return failed, counts
