"""The host build of csrc/lfd_geometry.hpp::lfd_null_vector_rows against EXACT answers (tests/golden/g19_solver_exact.npz: 80-digit
eigen-decompositions, made by tests/golden/make_solver_exact_fixture.py) under the rules of tests/solver_ref.py, over the solver's whole
domain: scene cells of every kind (family S), injected matrices with sigma4/sigma3 up to 1, the w -> 0 guard branch, degenerate and
non-finite matrices (family M), and every g13 matrix of kinds 0..4.  No GPU needed.

Before the shifted passes tested the sign of their pivots the solver returned the singular vector of sigma3 instead of sigma4
(|v3 . d| = 1) for g13's kind-4 matrices 2949, 2969 (r = 0.9), 2977, 2979, 2993 (r = 0.99), 3008 and 3013 (r just below 0.999): those,
and only those, failed here (3002, 3004 and 3010, the other wrong vectors of g13, have r just above 0.999, where only the residual
against sigma3 is asked for)."""
import numpy as np
import pytest

import lichtfeld_densification_plugin_amd as lfd
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
import solver_ref as sr


@pytest.fixture(scope="module")
def fx():
    return sr.load_fixture()


@pytest.fixture(scope="module")
def solved(fx):
    """host_null_vector of every matrix of the fixture, once: family -> (c[n,4], solves[n])."""
    out = {}
    for fam in "SMG":
        A = fx[fam + "_A"]
        c, it = np.empty((A.shape[0], 4)), np.empty(A.shape[0], int)
        for i in range(A.shape[0]):
            c[i], it[i] = hb.host_null_vector(A[i])
        out[fam] = (c, it)
    return out


def _judge_family(fx, solved, fam):
    A, sigma, cls, v = fx[fam + "_A"], fx[fam + "_sigma"], fx[fam + "_cls"], fx[fam + "_v"]
    c, it = solved[fam]
    failed, worst, banded = [], {0: 0.0, 1: 0.0, 2: 0.0}, 0
    for i in range(A.shape[0]):
        assert 3 <= it[i] <= sr.MAX_SOLVES, (fam, i, it[i])
        if cls[i] < 0:
            continue
        banded += sr.in_guard_band(v[i])
        fail, err, _ = sr.judge(A[i], sigma[i], cls[i], v[i], c[i])
        if fail:
            failed.append((int(fx["G_idx"][i]) if fam == "G" else i, fail, int(it[i])))
        elif err is not None:
            worst[int(cls[i])] = max(worst[int(cls[i])], err)
    print(f"[solver exact, host] family {fam}: {A.shape[0]} matrices, worst direction error by class of r {worst}, {banded} in the guard's band")
    return failed, banded


def test_scene_cells_family_s(fx, solved):
    kind = fx["S_kind"]
    assert kind.size == sr.S_GRID ** 2 and sorted(set(kind.tolist())) == [0, 1, 2, 3, 5] and (fx["S_cls"][kind == 5] == -1).all()
    assert (fx["S_cls"][kind != 5] >= 0).all()
    # the kinds are interleaved: every run of 8 cells along the raster holds ordinary, noise-free, noisy and far cells
    assert all(len(set(kind[i:i + 8].tolist()) - {5}) >= 3 for i in range(0, kind.size, 8))
    failed, _ = _judge_family(fx, solved, "S")
    assert not failed, failed


def test_injected_matrices_family_m(fx, solved):
    """Kinds 4 (sigma4/sigma3 in {0.5 .. 1}) and 7 (guard branch) under the rules, and kind 6 (degenerate) as far as it has a finite exact answer.
    The only finite matrices allowed a non-finite result are those the fixture flags ``M_nopivot``: a leading principal minor of A^T A is
    exactly zero, the unpivoted L D L^T does not exist (zero matrix, rank one, a zero first column, v3 = 0 exactly) and the solver lives on
    rounding noise - with small integers there may be none.  A finite result of such a matrix obeys the rules like any other."""
    kind, cls = fx["M_kind"], fx["M_cls"]
    assert (kind == 4).sum() == 150 and (kind == 7).sum() >= 30 and (kind == 6).sum() >= 8 and (kind == 5).sum() == 12
    assert not fx["M_nopivot"][kind == 4].any() and fx["M_nopivot"][(kind == 7) & (fx["M_w"] == 0)].all()
    failed, _ = _judge_family(fx, solved, "M")
    for i, fail, _ in failed:
        assert fail == "not finite" and fx["M_nopivot"][i], (i, fail, fx["M_A"][i])
    c, _ = solved["M"]
    assert np.isnan(c[kind == 5]).any(axis=1).all()
    # v3 = 0 exactly: at least some of them come through on rounding noise, and then take the guard branch with the right direction
    zero_w = np.nonzero((kind == 7) & (fx["M_w"] == 0))[0]
    assert sum(bool(np.isfinite(c[i]).all()) for i in zero_w) >= 2


def test_every_g13_matrix_of_kinds_0_to_4(fx, solved):
    """What tests/test_host_helpers.py::test_null_vector_matches_f64_svd leaves out as "the near-degenerate rest"."""
    failed, _ = _judge_family(fx, solved, "G")
    assert not failed, failed


def test_guard_band_cases_are_few(fx):
    total = sum(int((fx[f + "_cls"] >= 0).sum()) for f in "SMG")
    banded = sum(int(sum(sr.in_guard_band(v) for v, c in zip(fx[f + "_v"], fx[f + "_cls"]) if c >= 0)) for f in "SMG")
    assert 0 < banded <= 0.02 * total, (banded, total)
    fam_sm = sum(int((fx[f + "_cls"] >= 0).sum()) for f in "SM")
    banded_sm = sum(int(sum(sr.in_guard_band(v) for v, c in zip(fx[f + "_v"], fx[f + "_cls"]) if c >= 0)) for f in "SM")
    assert banded_sm <= 0.02 * fam_sm, (banded_sm, fam_sm)


def test_fixture_reaches_every_path(fx, solved):
    """Families S and M together (what the GPU tests launch): solve counts 3 (settled at k = 2), 4 (k = 3, the iterate that is moved), 5 (k = 4),
    6..9 (pass 0's tail loop), above 9 (shifted passes), and the guard branch - from scene cells and from injected matrices."""
    it = np.concatenate([solved["S"][1][fx["S_cls"] >= 0], solved["M"][1][fx["M_cls"] >= 0]])
    for lo, hi, least in ((3, 3, 100), (4, 4, 10), (5, 5, 10), (6, 9, 20), (10, sr.MAX_SOLVES, 50)):
        assert ((it >= lo) & (it <= hi)).sum() >= least, (lo, hi, int(((it >= lo) & (it <= hi)).sum()))
    its = solved["S"][1].reshape(-1, 64)            # the 64 lanes of a wave disagree
    assert all(len(set(row.tolist())) >= 3 for row in its)
    # the guard branch: no scene cell gets there (the f32 rounding of the pixels leaves |v3|/|v| >= 1e-9 even for a point at infinity) -
    # family M's kind 7 does, and takes the branch exactly where the exact answer asks for it
    assert not any(sr.host_guard_branch(c) for c in solved["S"][0][fx["S_cls"] >= 0])
    assert min(sr.w_fraction(v) for v in fx["S_v"][fx["S_kind"] == 3]) < 1e-8
    cM = solved["M"][0]
    hit = [i for i in np.nonzero(fx["M_kind"] == 7)[0] if sr.host_guard_branch(cM[i])]
    assert len(hit) >= 12, hit
    for i in np.nonzero((fx["M_kind"] == 7) & np.isfinite(cM).all(axis=1))[0]:
        if sr.guard_expected(fx["M_v"][i]):
            assert sr.host_guard_branch(solved["M"][0][i]), i
        elif not sr.in_guard_band(fx["M_v"][i]):
            assert not sr.host_guard_branch(solved["M"][0][i]), i


def _expected_xyz(c):
    """lfd_eval_correspondence's X from the solver's c (host build: IEEE division)."""
    if sr.host_guard_branch(c):
        return None
    with np.errstate(all="ignore"):
        return (c * (1.0 / c[3])).astype(np.float32)[:3]


def test_the_fixtures_matrix_is_the_kernels_matrix(fx, solved):
    """The per-cell routine (host build) on the stored correspondence returns the X of host_null_vector on the stored A, bit for bit: the
    generator's np.float32 row arithmetic IS lfd_eval_correspondence's.  (No scene cell takes the guard branch, where X = c / (1e-12 |c|) instead.)"""
    cams, ref, nbrs, _, _ = sr.scene_s(fx)
    params = sr.no_filter_params()
    c = solved["S"][0]
    exact_cells = 0
    for i in range(fx["S_A"].shape[0]):
        if fx["S_cls"][i] < 0:
            continue
        xa, ya, xb, yb = [float(t) for t in fx["S_corr"][i]]
        out = hb.host_eval_correspondence(cams[ref], cams[nbrs[int(fx["S_slot"][i])]], xa, ya, xb, yb, sr.S_GRID, sr.S_GRID, params)
        want = _expected_xyz(c[i])
        assert want is not None, i
        assert out[:3].view(np.uint32).tolist() == want.view(np.uint32).tolist(), (i, out[:3], want)
        exact_cells += 1
    assert exact_cells == int((fx["S_cls"] >= 0).sum()) == sr.S_GRID ** 2 - 5
    # family M: the injected cameras at pixel 0
    cM = solved["M"][0]
    n = 0
    for i in np.nonzero(fx["M_cls"] >= 0)[0]:
        want = _expected_xyz(cM[i])
        if want is None or not np.isfinite(cM[i]).all():
            continue
        ca, cb = sr.injected_cameras(fx["M_A"][i])
        out = hb.host_eval_correspondence(ca, cb, -1.0, -1.0, -1.0, -1.0, sr.M_MATCH, sr.M_MATCH, params)
        assert out[:3].view(np.uint32).tolist() == want.view(np.uint32).tolist(), (i, out[:3], want)
        n += 1
    assert n >= 150
