"""The DEVICE build of the re-triangulation's solver (csrc/lfd_refine.hpp::lfd_null_vector_sym) against exact answers, through all six
instantiations of lfd_refine_kernel<KMAX, WEIGHTED>.  Run with ``pytest -m gpu``.

The other GPU tests of lfd_refine_multiview[_weighted] see the solver through well-posed scenes, whose points settle after two solves; here
HipDensifier.refine_multiview gets the cases of tests/test_refine_solver_exact_host.py - every g13 matrix of kinds 0..4, g19's family M, the
three- and four-view matrices of g21 - through tests/solver_ref.py::run_refine, the helper the host test uses, with the gates wide open, and
every result goes under the same rules (check_refine): every finite case away from the w -> 0 guard is ACCEPTED and judged, a non-finite or
guard case keeps the bits of its input.

  k = 2, 3, 4 (the number of views)     lfd_refine_kernel<4, .>: all cases
  k = 5 and k = 9                       lfd_refine_kernel<8, .> and <16, .>: g13's classes 1..3 (533), family M, g21; the surplus slots dead,
                                        the winner at the first, a middle and the last slot

Device against CPU twin follows tests/test_gpu_solver_exact.py: the accepted set is the twin's - not held to it: the matrices flagged nopivot,
which live on rounding noise that the device's Newton-refined reciprocals and the twin's IEEE divisions do not share, and the cases in the
guard's band, which may take either branch - and the distance of the coordinates is reported, not asserted beyond the rules."""
import numpy as np
import pytest
import torch

from lichtfeld_densification_plugin_amd.core import hip_backend as hb
import solver_ref as sr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return sr.refine_cases()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def dens(dev):
    d = hb.HipDensifier(dev)
    yield d
    d.close()


@pytest.fixture(scope="module")
def twin():
    t = hb.HostDensifier()
    yield t
    t.close()


def _check(cases, dens, twin, dev, precision, k):
    what = f"{'weighted' if precision else 'unweighted'}, k = {k or 'views'}"
    for name, c in cases.items():
        out = sr.run_refine(dens, c["A"], torch, dev, precision, k=k)
        failed, counts = sr.check_refine(out, c["A"], c["sigma"], c["cls"], c["v"], c["nopivot"], precision, c["names"])
        ref = sr.run_refine(twin, c["A"], torch, torch.device("cpu"), precision, k=k)
        band = np.array([cl >= 0 and cl != 3 and sr.in_guard_band(v) for cl, v in zip(c["cls"], c["v"])])          # (either branch, on either build)
        held = ~c["nopivot"] & ~band
        both = ((out["status"] & ref["status"]) & sr.ACCEPTED) != 0
        a, b = out["xyz"][both], ref["xyz"][both]
        ulp = sr.ulp_distance(a, b)
        print(f"[refine solver exact, device, {what}] {name}: {counts}; against the twin {int((a.view(np.uint32) == b.view(np.uint32)).sum())} of {a.size} "
              f"f32 coordinates bit-equal, largest distance {int(ulp.max()) if ulp.size else 0} ulp")
        assert counts["skipped"] == 0
        assert not failed, (name, what, failed)
        assert np.array_equal(out["status"][held], ref["status"][held]), (name, what, np.nonzero(held & (out["status"] != ref["status"]))[0])
    return True


@pytest.mark.parametrize("precision", [False, True], ids=["unweighted", "weighted"])
def test_every_case_on_the_device(cases, dens, twin, dev, precision):
    assert _check(cases, dens, twin, dev, precision, None)


@pytest.mark.parametrize("precision", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("k", [5, 9])
def test_more_slots_than_views_on_the_device(cases, dens, twin, dev, k, precision):
    sub = sr.refine_subset(cases)
    assert sub["G"]["A"].shape[0] == 533
    assert _check(sub, dens, twin, dev, precision, k)


def test_repeat_bit_for_bit(cases, dens, dev):
    c = cases["V4"]
    a = sr.run_refine(dens, c["A"], torch, dev, True, k=9)
    b = sr.run_refine(dens, c["A"], torch, dev, True, k=9)
    assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["xyz"].view(np.uint32), b["xyz"].view(np.uint32))
    assert np.array_equal(a["err"].view(np.uint32), b["err"].view(np.uint32))
