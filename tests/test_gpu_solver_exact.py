"""The DEVICE build of csrc/lfd_geometry.hpp::lfd_null_vector_rows against exact answers, by value, on every path.  Run with ``pytest -m gpu``.

The device build differs from the host build exactly in this routine (v_rcp_f64 + one Newton step, v_rsq_f64 + coupled steps, the exponent
select of lfd_pow2_inv_scale, lanes of a wave leaving the solver after different numbers of solves), and the other GPU tests see it only
through the survivors of well-posed scenes, which settle after two solves.  Here the kernels get the cases of
tests/golden/g19_solver_exact.npz (80-digit eigen-decompositions; tests/golden/make_solver_exact_fixture.py) and every emitted point goes
under the rules of tests/solver_ref.py, the same that tests/test_solver_exact_host.py applies to the host build:

  family S  one 32x32 reference with three neighbours whose cells are interleaved ordinary, noise-free, 10-60 px noisy, far (w -> 0) and
            NaN / Inf cells - the lanes of every wave need between 3 and more than 9 solves - through triangulate_dense and through
            triangulate_indexed with every cell selected;
  family M  204 injected 4x4 matrices, one reference with one cell each, through triangulate_indexed: sigma4/sigma3 in {0.5 .. 1} (the
            shifted passes and their inertia search), the w -> 0 guard branch, degenerate and non-finite matrices.

Device against CPU twin (the host build over the same batches) is reported, not asserted beyond the rules: measured on an MI355X,
family S 2996 of 3003 f32 coordinates bit-equal, the largest distance 12 ulp; family M 472 of 564 bit-equal, the far ones guard-branch points
of the opposite sign (the branch loses the sign of c on purpose)."""
import numpy as np
import pytest
import torch

from lichtfeld_densification_plugin_amd.core import hip_backend as hb
import solver_ref as sr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return sr.load_fixture()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _host(out):
    return dict(cell=out.cell.cpu().numpy().astype(np.int64), xyz=out.xyz.cpu().numpy(), err=out.err.cpu().numpy())


@pytest.fixture(scope="module")
def twin(fx):
    """The CPU twin on the same batches, once."""
    t = hb.HostDensifier()
    dense, idx = sr.run_family_s(t, fx, torch, torch.device("cpu"))
    m = sr.run_family_m(t, fx, torch, torch.device("cpu"))
    t.close()
    return dict(dense=_host(dense), idx=_host(idx), m=m)


@pytest.fixture(scope="module")
def device_s(fx, dev):
    d = hb.HipDensifier(dev)
    dense, idx = sr.run_family_s(d, fx, torch, dev)
    again, _ = sr.run_family_s(d, fx, torch, dev)
    d.close()
    return dict(dense=_host(dense), idx=_host(idx), again=_host(again))


def _report(name, a, b):
    """Bit-equal coordinates and the largest distance between device and twin.  (The guard branch loses the sign of c on purpose: a point
    that came out as the twin's negative is compared with it negated.)"""
    flip = (a.astype(np.float64) * b.astype(np.float64)).sum(axis=1, keepdims=True) < 0
    b = np.where(flip, -b, b)
    same = a.view(np.uint32) == b.view(np.uint32)
    ulp = sr.ulp_distance(a, b)
    print(f"[solver exact, device vs twin] {name}: {int(same.sum())} of {same.size} f32 coordinates bit-equal, largest distance {int(ulp.max()) if ulp.size else 0} ulp")


def test_scene_cells_dense_under_the_rules(fx, twin, device_s):
    got = device_s["dense"]
    assert np.array_equal(got["cell"], twin["dense"]["cell"])                 # the emitted set is the twin's
    bad = np.nonzero(fx["S_cls"] < 0)[0]
    assert not np.isin(bad, got["cell"]).any()
    # every ordinary, noise-free and noisy cell is emitted; a far cell (w -> 0) may overflow its f32 reprojection error and is dropped then
    assert np.isin(np.nonzero(np.isin(fx["S_kind"], (0, 1, 2)))[0], got["cell"]).all() and np.isin(np.nonzero(fx["S_kind"] == 3)[0], got["cell"]).sum() >= 100
    assert np.isfinite(got["xyz"]).all() and np.isfinite(got["err"]).all()
    failed, worst = [], {0: 0.0, 1: 0.0, 2: 0.0}
    for cell, xyz in zip(got["cell"], got["xyz"]):
        fail, err, _ = sr.judge(fx["S_A"][cell], fx["S_sigma"][cell], fx["S_cls"][cell], fx["S_v"][cell],
                                sr.device_direction(xyz, fx["S_v"][cell], fx["S_cls"][cell]), device=True)
        if fail:
            failed.append((int(cell), fail))
        elif err is not None:
            worst[int(fx["S_cls"][cell])] = max(worst[int(fx["S_cls"][cell])], err)
    print(f"[solver exact, device] family S: {got['cell'].size} cells, worst direction error by class of r {worst}")
    _report("family S", got["xyz"], twin["dense"]["xyz"])
    assert not failed, failed


def test_scene_cells_indexed_equal_dense_bit_for_bit(fx, twin, device_s):
    d, i = device_s["dense"], device_s["idx"]
    assert np.array_equal(np.sort(i["cell"]), d["cell"]) and np.array_equal(np.sort(twin["idx"]["cell"]), d["cell"])
    order = np.argsort(i["cell"], kind="stable")          # indexed mode groups by slot; per cell the bits are the dense kernel's
    assert np.array_equal(i["xyz"][order].view(np.uint32), d["xyz"].view(np.uint32))
    assert np.array_equal(i["err"][order].view(np.uint32), d["err"].view(np.uint32))


def test_scene_cells_repeat_bit_for_bit(device_s):
    a, b = device_s["dense"], device_s["again"]
    assert np.array_equal(a["cell"], b["cell"])
    assert np.array_equal(a["xyz"].view(np.uint32), b["xyz"].view(np.uint32)) and np.array_equal(a["err"].view(np.uint32), b["err"].view(np.uint32))


def test_injected_matrices_under_the_rules(fx, twin, dev):
    d = hb.HipDensifier(dev)
    emitted, xyz = sr.run_family_m(d, fx, torch, dev)
    d.close()
    t_emitted, t_xyz = twin["m"]
    kind, cls = fx["M_kind"], fx["M_cls"]
    # the emitted set is the twin's, non-finite and degenerate matrices (kinds 5, 6) included.  Not held to it: the guard matrices with v3 = 0
    # exactly (kind 7, ``M_nopivot``), whose third pivot is 0 in exact arithmetic - the twin's IEEE divisions are exact on these small integers
    # and one of them ends in 0 * Inf, the device's Newton-refined reciprocals leave rounding noise and a finite, correct point.  If emitted,
    # such a point goes under the rules below like any other.
    held = ~(fx["M_nopivot"] & (kind == 7))
    assert np.array_equal(emitted[held], t_emitted[held]), np.nonzero(held & (emitted != t_emitted))[0]
    assert not emitted[cls < 0].any()
    must = (cls >= 0) & ~fx["M_nopivot"] & np.isin(kind, (4, 7))
    assert emitted[must].all(), np.nonzero(must & ~emitted)[0]
    failed, guards = [], 0
    for i in np.nonzero(emitted)[0]:
        assert np.isfinite(xyz[i]).all(), i
        fail, _, _ = sr.judge(fx["M_A"][i], fx["M_sigma"][i], cls[i], fx["M_v"][i], sr.device_direction(xyz[i], fx["M_v"][i], cls[i]), device=True)
        if fail:
            failed.append((int(i), fail))
        if kind[i] == 7 and sr.guard_expected(fx["M_v"][i]):          # X = c / (1e-12 |c|): |X| = 1e12, along v
            guards += 1
            assert abs(np.linalg.norm(xyz[i].astype(np.float64)) / 1e12 - 1.0) < 1e-6, (i, xyz[i])
        elif kind[i] == 7 and not sr.in_guard_band(fx["M_v"][i]):     # the common branch: X = v / v3
            want = fx["M_v"][i][:3] / fx["M_v"][i][3]
            assert np.abs(xyz[i] - want).max() <= 1e-6 * np.abs(want).max(), (i, xyz[i], want)
    _report("family M", xyz[emitted & t_emitted], t_xyz[emitted & t_emitted])
    assert not failed, failed
    assert guards >= 12, guards
