"""The host build of the re-triangulation's solver (csrc/lfd_refine.hpp::lfd_null_vector_sym) against EXACT answers, directly and through the
entry points that write the project's final coordinates (HostDensifier.refine_multiview, ``precision`` False and True), under the rules of
tests/solver_ref.py.  No GPU needed.

The cases: every g13 matrix of kinds 0..4 and g19's family M (tests/golden/g19_solver_exact.npz: sigma4/sigma3 up to 1, the w -> 0 guard,
degenerate, NaN / Inf, ``M_nopivot``) as two views, and the 6x4 and 8x4 matrices of tests/golden/g21_refine_solver_exact.npz (generator beside
it) as three and four views.  tests/solver_ref.py::run_refine injects a matrix as cameras whose DLT rows at pixel 0 are its rows, with the gates
wide open (support_thresh_px 1e15, reproj_thresh 1e30): every finite case away from the w -> 0 guard has to come back ACCEPTED and is judged, so
no gate can hide a wrong vector; a non-finite or guard case has to keep the bits of its input.  The weighted variant is fed the same M = A^T A
(lam = 4, the reference's rows halved).

Before the shifted passes of lfd_null_vector_sym were brought to lfd_null_vector_rows' scheme (negative-pivot test, step-down and bisection of
the shift, restart from e4, rescaling of a large iterate) these tests failed, in both variants and in the direct call, on the g13 matrices 2949,
2969 (r = 0.9), 2977, 2979, 2993 (r = 0.99), 3008 and 3013 (r just below 0.999) and on no other of the 3070 - direction error 1.414, residual
sigma3: the vector of sigma3 was accepted and replaced the two-view point - on the ten guard matrices of family M with |v3|/|v| of 1e-14 and
1e-13 (accepted with |X| of 1e12 .. 1e14: the squares of lfd_refine_dehomogenise's guard test overflowed, Inf < Inf) and on 35 to 40 of the 133
matrices of either family of g21.

g21's kind 8 (v4[3] = 1e-4, r >= 0.95) found a second way to the same wrong vector, in the fixed scheme as well: pass 0 sits next to v3 and drifts
away from it by less than LFD_NULLVEC_TOL per solve, lfd_nullvec_settled takes that for convergence and the routine left after three solves with
the vector of sigma3 - V3 95, 97, 99, 100 and V4 97, 98, 99, 100, class 2, direction error 1.414 - before any shifted pass.  lfd_null_vector_sym now
checks the inertia of M just below the eigenvalue a pass-0 settle found; a negative pivot hands the point to the shifted passes."""
import numpy as np
import pytest
import torch

from lichtfeld_densification_plugin_amd.core import hip_backend as hb
import solver_ref as sr

WIDE_K = (5, 9)               # the kernels' other two instantiations of KMAX (k <= 8, larger); the host twin has one, LFD_MAX_SLOTS


@pytest.fixture(scope="module")
def cases():
    return sr.refine_cases()


@pytest.fixture(scope="module")
def twin():
    t = hb.HostDensifier()
    yield t
    t.close()


@pytest.mark.parametrize("precision", [False, True], ids=["unweighted", "weighted"])
def test_every_case_through_refine_multiview(cases, twin, precision):
    """k = the number of views (2, 3, 4): all cases.  Nothing is skipped; every finite case that is neither a guard case nor flagged nopivot is
    accepted and judged (check_refine fails it otherwise)."""
    cpu = torch.device("cpu")
    for name, c in cases.items():
        out = sr.run_refine(twin, c["A"], torch, cpu, precision)
        failed, counts = sr.check_refine(out, c["A"], c["sigma"], c["cls"], c["v"], c["nopivot"], precision, c["names"])
        print(f"[refine solver exact, host, {'weighted' if precision else 'unweighted'}] {name}: {c['A'].shape[0]} cases, {counts}")
        assert counts["skipped"] == 0
        assert not failed, (name, failed)
        finite = int((c["cls"] >= 0).sum())
        assert counts["judged"] + counts["guard"] + counts["band"] + counts["nopivot_unaccepted"] == finite and counts["nonfinite"] == c["A"].shape[0] - finite
        if name == "G":
            assert counts["judged"] == 3070 == c["A"].shape[0]
        if name == "M":
            assert counts["guard"] >= 12 and counts["nopivot_unaccepted"] <= int(c["nopivot"].sum())


@pytest.mark.parametrize("precision", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("k", WIDE_K)
def test_more_slots_than_views(cases, twin, k, precision):
    """k = 5 and 9 with the surplus slots dead, the winner at the first, a middle and the last slot: g13's classes 1..3, family M and g21."""
    cpu = torch.device("cpu")
    sub = sr.refine_subset(cases)
    assert sub["G"]["A"].shape[0] == 533
    for name, c in sub.items():
        out = sr.run_refine(twin, c["A"], torch, cpu, precision, k=k)
        failed, counts = sr.check_refine(out, c["A"], c["sigma"], c["cls"], c["v"], c["nopivot"], precision, c["names"])
        assert counts["skipped"] == 0
        assert not failed, (name, k, failed)


def test_the_solver_called_directly(cases):
    """lfd_null_vector_sym on M = A^T A (f64 products of the f32 entries, summed in numpy): the rules on c itself, and the solve count - every
    call ends within the limits, the NaN / Inf matrices included, and the shifted passes and their search are reached."""
    solves = []
    for name, c in cases.items():
        failed = []
        for i in range(c["A"].shape[0]):
            A = c["A"][i].astype(np.float64)
            with np.errstate(all="ignore"):
                x, it = hb.host_null_vector_sym(A.T @ A)
            assert 3 <= it <= sr.MAX_SOLVES, (name, i, it)
            if c["cls"][i] < 0:
                assert not np.isfinite(x).all(), (name, i, x)
                continue
            solves.append(it)
            fail, _, _ = sr.judge(c["A"][i], c["sigma"][i], c["cls"][i], c["v"][i], x)
            if fail and not (fail == "not finite" and c["nopivot"][i]):
                failed.append((int(c["names"][i]), fail, it))
        assert not failed, (name, failed)
    solves = np.asarray(solves)
    for lo, hi, least in ((3, 3, 1000), (4, 5, 100), (6, 9, 50), (10, 17, 50), (18, sr.MAX_SOLVES, 10)):
        assert ((solves >= lo) & (solves <= hi)).sum() >= least, (lo, hi, int(((solves >= lo) & (solves <= hi)).sum()))


def test_injection_is_exact(cases, twin):
    """What run_refine relies on: a case whose answer is far from the input comes back with X = v[:3] / v[3] to f32 - the rows the routine solved
    ARE the fixture's - and the status counts the views beside reference and winner (the null view included)."""
    cpu = torch.device("cpu")
    for name, n_views in (("G", 2), ("V3", 3), ("V4", 4)):
        c = cases[name]
        easy = np.array([i for i in np.nonzero(c["cls"] == 0)[0] if sr.w_fraction(c["v"][i]) > 1e-6][:40])          # (not the guard's cases)
        for precision in (False, True):
            out = sr.run_refine(twin, c["A"][easy], torch, cpu, precision)
            assert (out["status"] == (n_views - 1) | sr.ACCEPTED | (sr.WEIGHTED if precision else 0)).all()
            want = c["v"][easy][:, :3] / c["v"][easy][:, 3:4]
            # a direction error e of the unit vector moves X = v[:3] / v[3] by about e (1 + |X|^2); e <= 1e-8 + 2^-23 for class 0
            bound = 2.0 * (1e-8 + sr.F32_EPS) * (1.0 + (want * want).sum(axis=1))
            assert (np.linalg.norm(out["xyz"] - want, axis=1) <= bound).all()
    assert sr.refine_slots(2, 9, 0) == [8] and sr.refine_slots(4, 9, 8) == [0, 4, 7] and sr.refine_winner(4, 9) == 4
