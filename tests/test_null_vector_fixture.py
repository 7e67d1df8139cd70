"""The host build of csrc/lfd_geometry.hpp::lfd_null_vector against values recorded from the commit before the solver's
pass 0 was written out (tests/golden/g13_null_vector.npz, made by tests/golden/make_null_vector_fixture.py on that commit):
bit-identical c[4] and the identical solve count for every stored matrix.  The host build divides where the device refines
v_rcp_f64, so this pins the STRUCTURE - which solves run, which iterate a lane returns, where NaN leaves - not the device's bits
(those are pinned by the byte comparison of bench.py --dump-outputs).  No GPU needed."""
import itertools
import os

import numpy as np
import pytest

from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from helpers import ROOT

FIXTURE = os.path.join(ROOT, "tests", "golden", "g13_null_vector.npz")
KINDS = {0: "ring scene, 0.1-2 px noise", 1: "noise-free (rank-deficient)", 2: "10-60 px noise", 3: "point at infinity",
         4: "sigma4/sigma3 near 1", 5: "NaN / Inf entries", 6: "zero, identity, huge, tiny, repeated rows"}


@pytest.fixture(scope="module")
def g13():
    return np.load(FIXTURE)


def test_fixture_covers_the_paths(g13):
    """The recorded solve counts show that every path of the solver is in the fixture: 3 (settled at k = 2), 4 (k = 3, the
    iterate that is moved), 5 (k = 4), 6..9 (the tail loop of pass 0), > 9 (shifted passes), and the NaN exits."""
    kind, it, c = g13["kind"], g13["it"].astype(int), g13["c"]
    assert g13["A"].shape == (kind.size, 4, 4) and g13["A"].dtype == np.float32 and kind.size >= 3000
    assert sorted(set(kind.tolist())) == sorted(KINDS)
    for n in (3, 4, 5, 6, 7, 8, 9):
        assert (it == n).sum() >= 20, n
    assert (it > 9).sum() >= 100                       # shifted passes ran
    assert (it[kind == 4] > 9).sum() >= 50
    assert np.isnan(c[kind == 5]).any(axis=1).all() and (it[kind == 5] == 3).all()     # NaN leaves at the first test
    assert (it[kind == 1] == 3).all()


@pytest.mark.parametrize("k", sorted(KINDS), ids=lambda k: KINDS[k].replace(" ", "_"))
def test_null_vector_is_the_recorded_one_bit_for_bit(g13, k):
    A, kind, c, it = g13["A"], g13["kind"], g13["c"], g13["it"]
    idx = np.nonzero(kind == k)[0]
    assert idx.size > 0
    for i in idx:
        x, n = hb.host_null_vector(A[i])
        assert n == int(it[i]), (i, n, int(it[i]))
        # bit patterns, so that NaN == NaN and -0.0 != +0.0
        assert x.view(np.uint64).tolist() == c[i].view(np.uint64).tolist(), (i, x, c[i])


def _settled_reference(e, ref):
    """The truth table in the comment above lfd_nullvec_settled (csrc/lfd_geometry.hpp), written from the specification:
    a NaN anywhere settles (the solver leaves at once); otherwise every error term must be within a positive ref."""
    if np.isnan(ref) or any(np.isnan(v) for v in e):
        return True
    return bool(ref > 0.0 and all(v <= ref for v in e))


def _settled_as_coded(e, ref):
    """The comparisons of lfd_nullvec_settled, operator for operator."""
    e0, e1, e2 = e
    more = (e0 > ref) or (e1 > ref) or (e2 > ref) or not (ref > 0.0)
    bad = (not (e0 == e0)) or (not (e1 == e1)) or (not (e2 == e2)) or (not (ref == ref))
    return (not more) or bad


def test_settled_truth_table():
    """Every combination of {below, equal, above, zero, +Inf, NaN} error terms with {positive, zero, +Inf, NaN} ref."""
    nan, inf = float("nan"), float("inf")
    rows = 0
    for ref in (1e-9, 0.0, inf, nan):
        for e in itertools.product((0.0, 5e-10, 1e-9, 2e-9, inf, nan), repeat=3):
            assert _settled_as_coded(e, ref) == _settled_reference(e, ref), (e, ref)
            rows += 1
    assert rows == 4 * 6 ** 3
    # the rows the comment lists
    assert _settled_reference((0.0, 0.0, 0.0), 0.0) is False          # ref == 0 never passes, even with no change at all
    assert _settled_reference((nan, 2e-9, 0.0), 1e-9) is True         # NaN wins over "more"
    assert _settled_reference((1e-9, 1e-9, 1e-9), 1e-9) is True       # equality settles
    assert _settled_reference((inf, 0.0, 0.0), inf) is True
