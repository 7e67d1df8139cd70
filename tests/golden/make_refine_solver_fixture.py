"""Exact answers for the re-triangulation's solver (csrc/lfd_refine.hpp::lfd_null_vector_sym) on THREE and FOUR views: g21_refine_solver_exact.npz.

    python tests/golden/make_refine_solver_fixture.py [out.npz]

Needs mpmath (development machines only; no test imports it).  The two-view matrices the same solver is tested with are g19's
(make_solver_exact_fixture.py); here the f32 6x4 and 8x4 matrices a reference, a winning slot and one or two candidates stack, with the
80-digit eigen-decomposition of A^T A of that fixture's ``exact``: sigma (f32), the unit null vector v (f64) and the class of
r = sigma4/sigma3 (``ratio_class``), stored exactly as g19 stores them, per family ``V3_*`` (6x4) and ``V4_*`` (8x4), beside
``*_kind``, ``*_w`` and ``*_nopivot`` (``no_pivot``).  tests/solver_ref.py::run_refine feeds them to the entry points.

kind 4  prescribed singular values: A = U diag(sigma) V^T rounded to f32, U with orthonormal columns, V orthogonal.  r = sigma4/sigma3 from 1e-6
        to 0.9999, dense around 0.9, 0.99 and 0.999 (the class boundaries, and where the shifted passes and their search for the shift
        work); sigma1/sigma4 from 1/r up to 1e4 beside every r.  Three V per r: a random one, and two whose v4 is nearly orthogonal to e4
        - the solver's start - with v4[3] = 1e-1 and 1e-2 while v3 carries e4: pass 0 then hands the first shifted pass a vector that v3
        dominates, the case in which the shift lands between mu4 and mu3.  And WIDE: sigma1/sigma4 of 1e5, 1e6 and 1e7 with r small enough
        that sigma1/sigma3 <= 5e3 - M = A^T A is rounded to f64, which alone turns v4 by ~2^-53 (sigma1/sigma3)^2, and beyond
        1e4 that exceeds the 1e-8 the rules ask of r < 0.1, whatever the solver does.
kind 8  as kind 4 with v4[3] = 1e-4 and r >= 0.95.  Pass 0 then sits next to v3, x = v3 + eps v4 with eps ~ 1e-4 growing by 1 / r^2 per solve:
        the direction changes by eps (1 - r^2) per solve, less than LFD_NULLVEC_TOL, which lfd_nullvec_settled alone takes for convergence:
        what lfd_null_vector_sym's inertia check behind a pass-0 settle is for.
kind 7  the w -> 0 guard: exactly singular, rows exactly representable in f32, exact null vector with |v3|/|v| = ``w`` in GUARD_W
        (make_solver_exact_fixture.py), built as that fixture's guard matrices are.
kind 5  one entry NaN / Inf in the reference's or the winner's rows (a candidate with such an entry fails the candidate test and never
        reaches the solver); all NaN; all Inf.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_solver_exact_fixture as g19            # noqa: E402

SEED = 20250121
RATIOS = (1e-6, 1e-4, 1e-2, 0.1, 0.5, 0.8,
          0.89, 0.895, 0.899, 0.8999, 0.9001, 0.901, 0.905, 0.91, 0.95,
          0.985, 0.989, 0.9899, 0.9901, 0.991, 0.995,
          0.998, 0.9985, 0.9989, 0.99899, 0.99901, 0.9991, 0.9995, 0.9999)
CONDS = (1e1, 1e2, 1e3, 1e4)                       # sigma1/sigma4 beside every r (those >= 2/r), in turn
WIDE = ((1e5, 1e-3), (1e5, 0.05), (1e6, 1e-5), (1e6, 1e-3), (1e7, 1e-6), (1e7, 1e-4))      # (sigma1/sigma4, r): badly conditioned
SMALL_W = (None, 1e-1, 1e-2)                       # v4[3] of the three V per r
DRIFT_W, DRIFT_R = 1e-4, (0.95, 0.985, 0.989, 0.991, 0.995, 0.998, 0.9985, 0.9989)      # kind 8


def orthonormal(rng, rows, cols):
    q, _ = np.linalg.qr(rng.normal(size=(rows, cols)))
    return q


def right_vectors(rng, w):
    """Orthogonal V (columns v1 .. v4).  ``w``: v4 = (u sqrt(1 - w^2), w) with u a random unit 3-vector and v3 = (-u w, sqrt(1 - w^2)) - v3
    carries e4, v4 nearly none of it."""
    if w is None:
        return orthonormal(rng, 4, 4)
    u = rng.normal(size=3)
    u /= np.linalg.norm(u)
    c = np.sqrt(1.0 - w * w)
    v4, v3 = np.append(u * c, w), np.append(-u * w, c)
    rest = orthonormal(rng, 4, 4)
    basis = [v4, v3]
    for col in rest.T:                              # Gram-Schmidt of two more
        for b in basis:
            col = col - b * (b @ col)
        if np.linalg.norm(col) > 0.3:
            basis.append(col / np.linalg.norm(col))
        if len(basis) == 4:
            break
    return np.stack([basis[2], basis[3], v3, v4], axis=1)


def prescribed(rng, n_views, cond, r, w, scale):
    s4 = 1.0
    s3 = s4 / r
    s1 = max(cond * s4, 2.0 * s3)
    s2 = np.sqrt(s1 * s3)
    U, V = orthonormal(rng, 2 * n_views, 4), right_vectors(rng, w)
    return ((U * np.array([s1, s2, s3, s4])) @ V.T * scale).astype(np.float32)


def guard_matrix(rng, n_views, w):
    """make_solver_exact_fixture.guard_matrices' construction on 2 n_views rows."""
    m = 2 * n_views
    basis = [np.array(b, np.float64) for b in ((2, -1, 0, 0), (1, 0, 1, 0), (0, 1, 2, 0), (0, 0, 0, 1), (2, -1, 0, 3), (1, 0, 1, -2), (0, 1, 2, 1))]
    if w == 0.0:
        while True:
            R = np.stack([sum(int(rng.randint(-2, 3)) * b for b in basis) for _ in range(m)])
            if np.linalg.matrix_rank(R) == 3 and np.abs(R @ np.array([1.0, 2.0, -1.0, 0.0])).max() == 0:
                break
        wv = 0.0
    else:
        t = np.float32(w)
        while True:
            dd = rng.choice([1.0, 2.0, 4.0, -1.0, -2.0], m) * np.append(np.ones(m - 1), rng.choice([0.0, 1.0]))
            R = np.stack([np.array([float(np.float32(-d) * t), float(rng.randint(-3, 4)), float(rng.randint(-3, 4)), d]) for d in dd])
            if np.linalg.matrix_rank(R[:, 1:]) == 3:
                break
        wv = float(t) / np.sqrt(1.0 + float(t) ** 2)
    R32 = (R / 256.0).astype(np.float32)
    assert (R32.astype(np.float64) == R / 256.0).all()
    return R32, wv


def family(rng, n_views):
    A, kind, w = [], [], []
    turn = 0
    for r in RATIOS:
        for sw in SMALL_W:
            ok = [c for c in CONDS if c >= 2.0 / r] or [2.0 / r]
            cond = ok[turn % len(ok)]
            turn += 1
            A.append(prescribed(rng, n_views, cond, r, sw, rng.choice([1.0, 40.0, 3000.0])))
            kind.append(4); w.append(np.nan)
    for cond, r in WIDE:
        A.append(prescribed(rng, n_views, cond, r, None, rng.choice([1e-2, 1.0])))
        kind.append(4); w.append(np.nan)
    for i, r in enumerate(DRIFT_R):
        A.append(prescribed(rng, n_views, (1e1, 1e2, 1e3)[i % 3], r, DRIFT_W, 1.0))
        kind.append(8); w.append(np.nan)
    for gw in g19.GUARD_W:
        for _ in range(3):
            R, wv = guard_matrix(rng, n_views, gw)
            A.append(R); kind.append(7); w.append(wv)
    m = 2 * n_views
    for row, col, val in ((0, 0, np.nan), (1, 3, np.inf), (2, 1, -np.inf), (3, 2, np.nan), (0, 3, np.nan), (3, 0, np.inf)):
        B = prescribed(rng, n_views, 100.0, 0.01, None, 1.0)
        B[row, col] = val
        A.append(B); kind.append(5); w.append(np.nan)
    A.append(np.full((m, 4), np.nan, np.float32)); kind.append(5); w.append(np.nan)
    A.append(np.full((m, 4), np.inf, np.float32)); kind.append(5); w.append(np.nan)
    A = np.stack(A).astype(np.float32)
    sig, v, cls = np.empty((A.shape[0], 4)), np.empty((A.shape[0], 4)), np.empty(A.shape[0], np.int8)
    for i in range(A.shape[0]):
        sig[i], v[i] = g19.exact(A[i])
        cls[i] = g19.ratio_class(sig[i])
    p = f"V{n_views}_"
    return {p + "A": A, p + "kind": np.asarray(kind, np.int8), p + "w": np.asarray(w, np.float64), p + "sigma": sig.astype(np.float32), p + "v": v,
            p + "cls": cls, p + "nopivot": np.array([g19.no_pivot(a) for a in A])}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "g21_refine_solver_exact.npz")
    rng = np.random.RandomState(SEED)
    d = {}
    for n_views in (3, 4):
        d.update(family(rng, n_views))
    np.savez_compressed(out, **d)
    print(out, os.path.getsize(out), "bytes;", {k: v.shape for k, v in d.items()})
    for n_views in (3, 4):
        cls = d[f"V{n_views}_cls"]
        print(n_views, "views: classes", {int(c): int((cls == c).sum()) for c in sorted(set(cls.tolist()))})


if __name__ == "__main__":
    main()
