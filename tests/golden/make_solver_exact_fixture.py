"""Exact answers for the triangulation solver (csrc/lfd_geometry.hpp::lfd_null_vector_rows): g19_solver_exact.npz.

    python tests/golden/make_solver_exact_fixture.py [out.npz]

Needs mpmath (development machines only; no test imports it).  For every stored f32 4x4 matrix A the eigen-decomposition
of A^T A is taken at 80 digits (mp.eigsy; the entries of A^T A are formed exactly from the f32 values): the four singular
values (stored as f32, with the class of r = sigma4/sigma3 taken from the exact values beside them: ``*_cls``, see ratio_class) and
the unit null vector, rounded to f64.  tests/solver_ref.py holds the rules the solver's output is judged by,
tests/test_solver_exact_host.py and tests/test_gpu_solver_exact.py apply them to the host and the device build.

Family S (arrays ``S_*``), scene cells: ONE reference of synthetic.ring_cameras with three neighbours on a 32x32 grid, four-channel
warps [xA yA xB yB].  Every cell has its own correspondence, drawn as g13's kinds 0..3 are (noise-free, 0.1-2 px, 10-60 px, point at
infinity), the kinds interleaved along the raster so that the 64 lanes of a wave need different numbers of solves, plus a few
cells with NaN / Inf coordinates.  A cell's matrix is built with the kernel's own f32 sequence in np.float32 scalar arithmetic.
Stored: the correspondence of every cell and the neighbour slot that wins it (the tests give that slot the highest certainty and
put the same warp plane in every slot), kind, A, sigma, v.

Family M (arrays ``M_*``), injected matrices: with warp value -1 on all four channels the pixel is 0 and the DLT rows
u P[2] - P[0], v P[2] - P[1] are -P[0], -P[1] exactly, so a reference camera and one neighbour with the rows of -A as the first two
rows of their P make the kernels solve A (``injected_cameras`` of tests/solver_ref.py; third rows (0, 0, 0, 1): depth X[3] = 1).
g13's 150 kind-4 spectra, 12 of its kind-5 (NaN / Inf) and its kind-6 matrices (``M_g13`` = their g13 index), and new matrices
for the w -> 0 guard branch (kind 7): exactly singular, rows exactly representable in f32, exact null vector with
|v3|/|v| = ``M_w`` in {0, 1e-14, 1e-13, 4e-13, 5e-13, 2e-12, 2.5e-12, 1e-11}.

``M_nopivot``: a leading principal minor of A^T A is exactly zero (see no_pivot): the zero matrix, rank-one matrices, a zero first column and
every matrix with v3 = 0 exactly.  For these a non-finite result is accepted; a finite one obeys the rules like any other.

g13 (arrays ``G_*``): sigma and v of every g13 matrix of kinds 0..4, in the order of their g13 indices.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

SEED = 20250119
DIGITS = 80
GRID = 32                      # family S: H = W = w_match = h_match
S_REF, S_CAMS = 7, 60          # reference camera of synthetic.ring_cameras(60, seed=0); its ring neighbours +1, -1, +2
# kinds along the raster (period 8 against the 64 lanes of a wave: every wave holds every kind)
S_PATTERN = (0, 2, 1, 0, 3, 2, 0, 2)
S_BAD = {37: (2, np.nan), 38: (3, np.inf), 500: (2, -np.inf), 501: (3, np.nan), 1023: (2, np.inf)}     # cell: (channel, value), kind 5
GUARD_W = (0.0, 1e-14, 1e-13, 4e-13, 5e-13, 2e-12, 2.5e-12, 1e-11)


def exact(A):
    """(sigma[4] descending, unit v[4]) of a finite f32 m x 4 matrix, f64-rounded from an 80-digit eigen-decomposition of A^T A."""
    import mpmath as mp
    mp.mp.dps = DIGITS
    A = np.asarray(A, np.float32).reshape(-1, 4)
    if not np.isfinite(A).all():
        return np.full(4, np.nan), np.full(4, np.nan)
    a = mp.matrix([[mp.mpf(float(A[i, j])) for j in range(4)] for i in range(A.shape[0])])
    M = a.T * a
    if max(abs(M[i, j]) for i in range(4) for j in range(4)) == 0:
        return np.zeros(4), np.array([0.0, 0.0, 0.0, 1.0])
    E, Q = mp.eigsy(M)                       # ascending
    order = sorted(range(4), key=lambda i: E[i])
    sig = [mp.sqrt(E[i]) if E[i] > 0 else mp.mpf(0) for i in order[::-1]]
    v = [Q[i, order[0]] for i in range(4)]
    n = mp.sqrt(sum(x * x for x in v))
    return np.array([float(s) for s in sig]), np.array([float(x / n) for x in v])


def no_pivot(A):
    """Is a leading principal minor (1x1 .. 3x3) of A^T A exactly zero, i.e. are the first k <= 3 columns of A linearly dependent?  The
    solver's unpivoted L D L^T then does not exist (a pivot that divides is 0): it survives on rounding noise where there is any, and
    returns NaN - the cell is dropped - where the arithmetic happens to be exact.  Every matrix whose exact null vector has v3 = 0
    is of this kind (its first three columns are dependent)."""
    import mpmath as mp
    mp.mp.dps = DIGITS
    A = np.asarray(A, np.float32).reshape(-1, 4)
    if not np.isfinite(A).all():
        return False
    a = mp.matrix([[mp.mpf(float(A[i, j])) for j in range(4)] for i in range(A.shape[0])])
    M = a.T * a
    scale = max(abs(M[i, i]) for i in range(4))
    if scale == 0:
        return True
    return any(abs(mp.det(M[:k, :k])) <= scale ** k * mp.mpf(10) ** -60 for k in (1, 2, 3))


def kernel_rows(Pa, Pb, corr, wm1, hm1, sa, sb):
    """The DLT matrix of lfd_eval_correspondence in np.float32 scalar arithmetic: xa = ((xan + 1) * 0.5) * wm1, ua = xa * sx,
    rows u * P[2] - P[0] (multiply, then subtract)."""
    f = np.float32
    one, half = f(1.0), f(0.5)
    with np.errstate(all="ignore"):
        px = [((f(corr[0]) + one) * half) * f(wm1), ((f(corr[1]) + one) * half) * f(hm1),
              ((f(corr[2]) + one) * half) * f(wm1), ((f(corr[3]) + one) * half) * f(hm1)]
        u = [px[0] * f(sa[0]), px[1] * f(sa[1]), px[2] * f(sb[0]), px[3] * f(sb[1])]
        A = np.empty((4, 4), np.float32)
        for c in range(4):
            A[0, c] = u[0] * f(Pa[2, c]) - f(Pa[0, c])
            A[1, c] = u[1] * f(Pa[2, c]) - f(Pa[1, c])
            A[2, c] = u[2] * f(Pb[2, c]) - f(Pb[0, c])
            A[3, c] = u[3] * f(Pb[2, c]) - f(Pb[1, c])
    return A


def pair_scales(cam, w_match, h_match):
    return np.float32(float(cam.width) / float(w_match)), np.float32(float(cam.height) / float(h_match))


def family_s(rng):
    from lichtfeld_densification_plugin_amd import synthetic
    cams = synthetic.ring_cameras(S_CAMS, seed=0)
    nbrs = synthetic.ring_neighbours(S_CAMS, S_REF, 3)
    ca = cams[S_REF]
    Pa = np.asarray(ca.P, np.float64)
    sa = pair_scales(ca, GRID, GRID)
    n = GRID * GRID
    corr, slot, kind, A = np.zeros((n, 4), np.float32), np.zeros(n, np.uint8), np.zeros(n, np.int8), np.zeros((n, 4, 4), np.float32)
    for cell in range(n):
        k = S_PATTERN[cell % len(S_PATTERN)]
        j = int(rng.randint(3))
        cb = cams[nbrs[j]]
        Pb = np.asarray(cb.P, np.float64)
        sb = pair_scales(cb, GRID, GRID)
        noise = {0: rng.choice([0.1, 0.5, 1.0, 2.0]), 1: 0.0, 2: rng.choice([10.0, 30.0, 60.0]), 3: rng.choice([0.0, 0.3])}[k]
        while True:          # the reference pixel stays inside its image (a matcher's xA, yA lie in [-1, 1])
            if k == 3:
                d = rng.normal(size=3)
                d[2] = -abs(d[2]) * 0.2
                X = np.array([d[0], d[1], d[2], rng.choice([1e-3, 1e-6, 1e-9, 1e-12, 1e-20, 0.0])])
            else:
                X = np.array([rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(-0.3, 0.5), 1.0])
            qa, qb = Pa @ X, Pb @ X
            if qa[2] == 0.0 or qb[2] == 0.0:
                continue
            ua = qa[:2] / qa[2] + rng.normal(0, noise, 2)
            ub = qb[:2] / qb[2] + rng.normal(0, noise, 2)
            na = np.array([ua[0] / float(sa[0]), ua[1] / float(sa[1])]) / (GRID - 1) * 2.0 - 1.0
            nb = np.array([ub[0] / float(sb[0]), ub[1] / float(sb[1])]) / (GRID - 1) * 2.0 - 1.0
            if np.abs(na).max() <= 1.0 and np.abs(nb).max() <= 4.0:
                break
        corr[cell] = np.concatenate([na, nb]).astype(np.float32)
        slot[cell], kind[cell] = j, k
        if cell in S_BAD:
            ch, val = S_BAD[cell]
            corr[cell, ch] = val
            kind[cell] = 5
        A[cell] = kernel_rows(np.asarray(ca.P, np.float32), np.asarray(cb.P, np.float32), corr[cell], GRID - 1, GRID - 1, sa, sb)
    return dict(S_corr=corr, S_slot=slot, S_kind=kind, S_A=A, S_cams=np.array([S_REF] + list(nbrs), np.int32))


def guard_matrices(rng):
    """Exactly singular matrices whose exact null vector has |v3|/|v| = w (kind 7), scaled by 2^-8 (exact) so that the f32
    reprojection error of the guard branch's X ~ 1e12 v stays far from overflow."""
    out = []
    basis = [np.array(b, np.float64) for b in ((2, -1, 0, 0), (1, 0, 1, 0), (0, 1, 2, 0), (0, 0, 0, 1), (2, -1, 0, 3), (1, 0, 1, -2), (0, 1, 2, 1))]
    for w in GUARD_W:
        for _ in range(4):
            if w == 0.0:          # rows of small integers orthogonal to (1, 2, -1, 0): v3 = 0 exactly
                while True:
                    R = np.stack([sum(int(rng.randint(-2, 3)) * b for b in basis) for _ in range(4)])
                    if np.linalg.matrix_rank(R) == 3 and np.abs(R @ np.array([1.0, 2.0, -1.0, 0.0])).max() == 0:
                        break
                wv = 0.0
            else:                 # rows (-d t, b, c, d), d a power of two: v = (1, 0, 0, t) exactly, t the f32 next to w
                t = np.float32(w)
                while True:
                    dd = rng.choice([1.0, 2.0, 4.0, -1.0, -2.0], 4) * np.array([1.0, 1.0, 1.0, rng.choice([0.0, 1.0])])
                    R = np.stack([np.array([float(np.float32(-d) * t), float(rng.randint(-3, 4)), float(rng.randint(-3, 4)), d]) for d in dd])
                    if np.linalg.matrix_rank(R[:, 1:]) == 3:
                        break
                wv = float(t) / np.sqrt(1.0 + float(t) ** 2)
            R32 = (R / 256.0).astype(np.float32)
            assert (R32.astype(np.float64) == R / 256.0).all()
            out.append((R32, wv))
    return out


def family_m(rng, g13):
    A13, kind13 = g13["A"], g13["kind"]
    A, kind, src, w = [], [], [], []
    for i in np.nonzero(kind13 == 4)[0]:
        A.append(A13[i]); kind.append(4); src.append(i); w.append(np.nan)
    for R, wv in guard_matrices(rng):
        A.append(R); kind.append(7); src.append(-1); w.append(wv)
    for i in np.nonzero(kind13 == 6)[0]:
        A.append(A13[i]); kind.append(6); src.append(i); w.append(np.nan)
    k5 = np.nonzero(kind13 == 5)[0]
    for i in list(k5[::5][:10]) + list(k5[-2:]):          # one entry NaN / Inf at several positions, all-NaN, all-Inf
        A.append(A13[i]); kind.append(5); src.append(i); w.append(np.nan)
    return dict(M_A=np.stack(A).astype(np.float32), M_kind=np.asarray(kind, np.int8), M_g13=np.asarray(src, np.int32), M_w=np.asarray(w, np.float64))


def ratio_class(sig):
    """-1: non-finite matrix; 0: r < 0.1; 1: 0.1 <= r < 0.9; 2: 0.9 <= r <= 0.999; 3: r > 0.999 or sigma3 = 0 (r = sigma4/sigma3 from the
    f64-rounded exact values: the class is stored because the sigmas themselves are stored as f32)."""
    if not np.isfinite(sig).all():
        return -1
    if sig[2] <= 1e-30 * sig[0]:          # rank <= 2 (an exact zero comes out of the 80 digits as ~1e-40 sigma1): no unique v
        return 3
    r = sig[3] / sig[2]
    return 0 if r < 0.1 else (1 if r < 0.9 else (2 if r <= 0.999 else 3))


def solve_all(A):
    sig, v, cls = np.empty((A.shape[0], 4)), np.empty((A.shape[0], 4)), np.empty(A.shape[0], np.int8)
    for i in range(A.shape[0]):
        sig[i], v[i] = exact(A[i])
        cls[i] = ratio_class(sig[i])
    return sig.astype(np.float32), v, cls


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "g19_solver_exact.npz")
    g13 = np.load(os.path.join(HERE, "g13_null_vector.npz"))
    rng = np.random.RandomState(SEED)
    d = family_s(rng)
    d["S_sigma"], d["S_v"], d["S_cls"] = solve_all(d["S_A"])
    d.update(family_m(rng, g13))
    d["M_sigma"], d["M_v"], d["M_cls"] = solve_all(d["M_A"])
    d["M_nopivot"] = np.array([no_pivot(a) for a in d["M_A"]])
    idx = np.nonzero(g13["kind"] <= 4)[0]
    d["G_sigma"], d["G_v"], d["G_cls"] = solve_all(g13["A"][idx])
    d["G_n"] = np.array(idx.size, np.int32)
    # the matrices taken from g13 are not stored twice: M_A7 holds the new (kind 7) ones, load_fixture of tests/solver_ref.py puts M_A together
    d["M_A7"] = d.pop("M_A")[d["M_kind"] == 7]
    np.savez_compressed(out, **d)
    print(out, os.path.getsize(out), "bytes;", {k: v.shape for k, v in d.items()})


if __name__ == "__main__":
    main()
