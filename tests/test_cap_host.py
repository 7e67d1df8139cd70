"""CPU tier of the spatial point cap (lfd_cap_spatial_host): the twin against the NumPy reference of tests/cap_ref.py on the clouds
(a) - (g) - index list and statistics, element for element -, the shape of the answer, the error's tie rule and its bit-pattern order, the
independence of the thread count, every refusal, and what the cap is for: on the two-density cloud it keeps the two squares about evenly where the
random draw keeps their 10 : 1."""
import ctypes as C

import numpy as np
import pytest
import torch

import cap_ref as cr
from lichtfeld_densification_plugin_amd import densify
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

LFD_ERR_INVALID = 1
CLOUDS = cr.clouds()


@pytest.fixture(scope="module")
def twin():
    dens = hb.HostDensifier(3)
    yield dens
    dens.close()


@pytest.fixture(scope="module")
def reference():
    """name -> (keep, stats) of the reference, computed once"""
    return {name: cr.cap_ref(xyz, err, m) for name, xyz, err, m in CLOUDS}


def run(dens, xyz, err, m):
    keep = dens.cap_spatial(torch.from_numpy(xyz), None if err is None else torch.from_numpy(err), m)
    return keep.numpy(), dens.cap_stats


@pytest.mark.parametrize("case", CLOUDS, ids=[c[0] for c in CLOUDS])
def test_twin_equals_reference(twin, reference, case):
    name, xyz, err, m = case
    keep, stats = run(twin, xyz, err, m)
    want, want_stats = reference[name]
    assert keep.dtype == np.int64 and keep.tolist() == want.tolist()
    assert stats == want_stats and isinstance(stats[3], float)
    n = xyz.shape[0]
    assert (np.diff(keep) > 0).all() and (keep >= 0).all() and (keep < n).all()      # ascending, a subset of the input indices
    finest = np.unique(cr.keys_ref(xyz)[0]).size
    if finest >= m:
        assert keep.size == m
    else:
        assert keep.size == finest
    lev, c, above, _L = stats
    assert keep.size == min(m, c) and (lev == 0 or above < m)


def test_identical_points_keep_exactly_one(twin):
    name, xyz, err, m = next(c for c in CLOUDS if c[0] == "c-identical")
    keep, stats = run(twin, xyz, err, m)
    assert keep.tolist() == [int(np.argmin(err))] and stats == (21, 1, 1, 0.0)


def test_error_rule_ties_none_and_bit_patterns(twin):
    xyz, _err, _ = cr.two_density(1)
    xyz = xyz[:3000]
    n, m = xyz.shape[0], 97
    # without an error the lowest input index of a picked cell is kept
    keep_none, _ = run(twin, xyz, None, m)
    assert keep_none.tolist() == cr.cap_ref(xyz, None, m)[0].tolist()
    keys = cr.keys_ref(xyz)[0] >> np.uint64(3 * (21 - twin.cap_stats[0]))
    for i in keep_none:
        assert i == np.flatnonzero(keys == keys[i]).min()
    # an error with ties: the same choice as a constant one
    flat = np.full(n, 0.25, np.float32)
    assert run(twin, xyz, flat, m)[0].tolist() == keep_none.tolist()
    coarse = (np.arange(n) % 3).astype(np.float32)
    keep_c, _ = run(twin, xyz, coarse, m)
    assert keep_c.tolist() == cr.cap_ref(xyz, coarse, m)[0].tolist()
    for i in keep_c:
        cell = np.flatnonzero(keys == keys[i])
        assert coarse[i] == coarse[cell].min() and i == cell[coarse[cell] == coarse[i]].min()
    # -0.0 sorts below +0.0, a NaN by its bits (a positive quiet NaN above every number, a negative one below); a small cloud, and with a budget
    # of 1 the whole cloud is one cell whose winner can be named
    few = xyz[:16]
    odd = np.zeros(16, np.float32)
    odd[9], odd[12] = -0.0, -0.0
    odd[5] = np.nan
    odd.view(np.uint32)[7] = 0xffc00000
    for m_few in (1, 5):
        assert run(twin, few, odd, m_few)[0].tolist() == cr.cap_ref(few, odd, m_few)[0].tolist()
    assert run(twin, few, odd, 1)[0].tolist() == [7]                     # the negative NaN's bits are below every number's
    odd.view(np.uint32)[7] = 0
    assert run(twin, few, odd, 1)[0].tolist() == [9]                     # then the first -0.0
    odd[:] = np.nan
    odd[11] = 3.0e38
    assert run(twin, few, odd, 1)[0].tolist() == [11]                    # a positive NaN is above every number
    odd[11] = np.nan
    assert run(twin, few, odd, 1)[0].tolist() == [0]
    odd[:] = 0.0


def test_thread_count_does_not_change_the_answer(reference):
    name, xyz, err, m = next(c for c in CLOUDS if c[0] == "g-m1000")
    for threads in (1, 2, 7):
        dens = hb.HostDensifier(threads)
        try:
            keep, stats = run(dens, xyz, err, m)
        finally:
            dens.close()
        assert keep.tolist() == reference[name][0].tolist() and stats == reference[name][1]


def test_cap_that_does_not_act_and_empty_cloud(twin):
    xyz = np.random.default_rng(5).uniform(0, 1, (40, 3)).astype(np.float32)
    xyz[3] = xyz[9]
    for m in (40, 41, 1000):
        keep, stats = run(twin, xyz, None, m)
        assert keep.tolist() == list(range(40)) and stats == cr.cap_ref(xyz, None, m)[1]
    keep, stats = run(twin, np.zeros((0, 3), np.float32), None, 5)
    assert keep.size == 0 and stats == (0, 0, 0, 0.0)
    keep, stats = run(twin, np.zeros((0, 3), np.float32), np.zeros(0, np.float32), 5)
    assert keep.size == 0


def test_every_refusal_message(twin):
    lib = hb.load_library()
    n = 300
    xyz = np.random.default_rng(0).uniform(-1, 1, (n, 3)).astype(np.float32)
    err = np.zeros(n, np.float32)
    out = np.full(n, -1, np.int64)
    n_keep = C.c_int64(-1)
    stats = (C.c_double * 4)(-1, -1, -1, -1)
    p = lambda a: a.ctypes.data                                           # noqa: E731
    good = dict(xyz=p(xyz), err=p(err), n=n, m=100, out=p(out), n_keep=C.byref(n_keep), stats=stats)

    def call(**kw):
        a = {**good, **kw}
        return lib.lfd_cap_spatial_host(twin._ctx, a["xyz"], a["err"], a["n"], a["m"], a["out"], a["n_keep"], a["stats"])

    before = xyz.copy()
    assert call() == 0 and n_keep.value == 100 and (out[100:] == -1).all() and stats[1] >= 100
    assert xyz.tobytes() == before.tobytes()                              # the input is read only
    first = out.copy()
    assert call(stats=None) == 0 and out.tobytes() == first.tobytes()
    assert call(n=0, xyz=None, err=None, out=None) == 0 and n_keep.value == 0 and list(stats) == [0.0, 0.0, 0.0, 0.0]
    expect = [(dict(xyz=None), b"null xyz / keep_out"), (dict(out=None), b"null xyz / keep_out"), (dict(n_keep=None), b"null n_keep_host"),
              (dict(n=-1), b"n must be in [0, 2^31 - 1]"), (dict(n=1 << 31), b"n must be in [0, 2^31 - 1]"), (dict(m=0), b"budget must be >= 1"),
              (dict(m=-3), b"budget must be >= 1"), (dict(out=p(xyz)), b"in and out arrays overlap"),
              (dict(out=p(xyz) + 12 * n - 8), b"in and out arrays overlap"), (dict(out=p(err) + 4 * n - 8), b"in and out arrays overlap")]
    for kw, words in expect:
        assert call(**kw) == LFD_ERR_INVALID, kw
        assert lib.lfd_last_error(twin._ctx) == b"lfd_cap_spatial_host: " + words, kw
    for value in (np.nan, np.inf, -np.inf):
        bad = xyz.copy()
        bad[17, 2] = value
        assert call(xyz=p(bad)) == LFD_ERR_INVALID
        assert lib.lfd_last_error(twin._ctx) == b"lfd_cap_spatial_host: non-finite coordinate in the input"
        with pytest.raises(hb.CapInputRefused, match="non-finite coordinate"):
            twin.cap_spatial(torch.from_numpy(bad), None, 100)
        bad[17, 2] = 0.0
    assert call() == 0 and out.tobytes() == first.tobytes()               # and the context still works
    with pytest.raises(ValueError, match="xyz must be a float32 tensor"):
        twin.cap_spatial(torch.zeros((4, 2)), None, 2)
    with pytest.raises(ValueError, match="err must be None or a float32 tensor"):
        twin.cap_spatial(torch.zeros((4, 3)), torch.zeros(5), 2)


@pytest.mark.parametrize("m", [1000, 257])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_coverage_on_the_two_density_cloud(twin, seed, m):
    xyz, err, dense = cr.two_density(seed)
    keep, _ = run(twin, xyz, err, m)
    ratio = dense[keep].sum() / (~dense[keep]).sum()
    assert 0.8 <= ratio <= 1.25, ratio
    drawn = densify._cap_index(xyz.shape[0], m, seed)
    assert dense[drawn].sum() / (~dense[drawn]).sum() > 5.0              # the scene discriminates: the random cap keeps the density contrast
