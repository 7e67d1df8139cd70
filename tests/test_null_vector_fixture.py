"""The host build of csrc/lfd_geometry.hpp::lfd_null_vector against values recorded from the commit before the solver's
pass 0 was written out (tests/golden/g13_null_vector.npz, made by tests/golden/make_null_vector_fixture.py on that commit):
bit-identical c[4] and the identical solve count for every stored matrix.  The host build divides where the device refines
v_rcp_f64, so this pins the STRUCTURE - which solves run, which iterate a lane returns, where NaN leaves - not the device's bits
(those are pinned by the byte comparison of bench.py --dump-outputs).  No GPU needed.

Re-recorded since (tests/golden/make_null_vector_fixture.py --rerecord), when the shifted passes began to test the sign of their pivots and
the loop solves to keep the iterate below 2^64 - 48 records, every other one is the first recording's:
  2474 2512 (kind 2), 2947 2949 2957 2967 2969 2971 2973 2977 2979 2982 2984 2987 2988 2989 2991 2993 2994 2995 3000 3002 3004 3005 3006
  3008 3010 3012 3013 3014 3016 3021 3023 3028 3032 3033 3035 3039 3042 3044 3047 3050 3058 3064 3066 (kind 4), 3146 (kind 6): a shifted
  pass found a negative pivot and searched its shift.  Among them 2949 2969 2977 2979 2993 3002 3004 3008 3010 3013, whose first record
  was the singular vector of sigma3 instead of sigma4.
  2841 2881 (kind 3, points at infinity): pass 0's tail loop rescaled an iterate above 2^64; c is the old one times a power of two."""
import hashlib
import itertools
import os

import numpy as np
import pytest

from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from helpers import ROOT

FIXTURE = os.path.join(ROOT, "tests", "golden", "g13_null_vector.npz")
RERECORDED = [2474, 2512, 2841, 2881, 2947, 2949, 2957, 2967, 2969, 2971, 2973, 2977, 2979, 2982, 2984, 2987, 2988, 2989, 2991, 2993, 2994, 2995,
              3000, 3002, 3004, 3005, 3006, 3008, 3010, 3012, 3013, 3014, 3016, 3021, 3023, 3028, 3032, 3033, 3035, 3039, 3042, 3044, 3047, 3050,
              3058, 3064, 3066, 3146]
WRONG_VECTOR = [2949, 2969, 2977, 2979, 2993, 3002, 3004, 3008, 3010, 3013]      # first record: v3 instead of v4
FIRST_RECORDING_SHA256 = "ab8016674b216c91b85947b6eb42e4db2f26e6a8b807b0b6667ffb79632605aa"     # of c and it as first recorded
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


def test_only_the_listed_records_were_rerecorded(g13):
    """The records the fixture says were replaced are the ones listed above; with their first values put back, c and it are the first
    recording's, byte for byte.  Each replaced record changed for a stated reason: a shifted pass had run (more than 9 solves) or the
    iterate had passed 2^64 (then the new c is the old one times a power of two, same solve count).  The ten wrong vectors are among
    them and now pass the exact rules (tests/solver_ref.py, tests/golden/g19_solver_exact.npz)."""
    import solver_ref as sr
    idx = g13["rerecorded"].astype(int)
    assert idx.tolist() == RERECORDED and set(WRONG_VECTOR) <= set(RERECORDED)
    c, it = g13["c"].copy(), g13["it"].copy()
    c[idx], it[idx] = g13["c_prev"], g13["it_prev"]
    assert hashlib.sha256(c.tobytes() + it.tobytes()).hexdigest() == FIRST_RECORDING_SHA256
    for j, i in enumerate(idx):
        old, new = g13["c_prev"][j], g13["c"][i]
        assert old.tobytes() != new.tobytes() or int(g13["it_prev"][j]) != int(g13["it"][i]), i
        if int(g13["it_prev"][j]) <= 9:
            assert np.abs(old).max() > 2.0 ** 64 and int(g13["it_prev"][j]) == int(g13["it"][i]), i
            ratio = new / old
            assert (ratio == ratio[0]).all() and np.log2(ratio[0]) == np.round(np.log2(ratio[0])), (i, ratio)
    fx = sr.load_fixture()
    pos = {int(i): k for k, i in enumerate(fx["G_idx"])}
    for i in WRONG_VECTOR:
        k = pos[i]
        fail, _, _ = sr.judge(fx["G_A"][k], fx["G_sigma"][k], fx["G_cls"][k], fx["G_v"][k], g13["c"][i])
        assert fail is None, (i, fail)
        # ... and the first record was v3: orthogonal to the exact v4, with the residual of sigma3
        old = g13["c_prev"][RERECORDED.index(i)]
        old = old / np.linalg.norm(old)
        assert abs(old @ fx["G_v"][k]) < 1e-6, i
        res = np.linalg.norm(fx["G_A"][k].astype(np.float64) @ old)
        assert abs(res / float(fx["G_sigma"][k][2]) - 1.0) < 1e-6, (i, res)


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
