"""The rules the triangulation solver (csrc/lfd_geometry.hpp::lfd_null_vector_rows) is judged by against the exact answers of
tests/golden/g19_solver_exact.npz (made by tests/golden/make_solver_exact_fixture.py), for the host and the GPU tests alike.

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


def injected_cameras(A, uid=0):
    """Reference and neighbour camera whose DLT matrix at pixel 0 (warp value -1 on all four channels) is A exactly: rows of -A as the first two
    rows of P, third row (0, 0, 0, 1) - the depth of X is X[3]."""
    import lichtfeld_densification_plugin_amd as lfd
    A = np.asarray(A, np.float32).reshape(4, 4)
    out = []
    for h in range(2):
        P = np.zeros((3, 4), np.float32)
        P[0], P[1], P[2, 3] = -A[2 * h], -A[2 * h + 1], 1.0
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
