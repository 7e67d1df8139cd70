"""The twin of the exact 3-nearest-neighbour distance (lfd_knn_dist2_host) against the brute-force NumPy reference
(tests/knn_ref.py): EQUAL bit for bit on every cloud of the issue, whatever the cell size - automatic, or forced to 0.01, 1 and 10 times the
longest box side, which sends a cloud through every ring and through the brute-force pass -; the caps that keep the grid path honest (a run that
brute-forced everything, or put the cloud into one cell, would still be exact); every refusal with its message; the empty cloud; and the twin
of the 68-byte record against the NumPy formula."""
import numpy as np
import pytest
import torch

import knn_ref as kr
from lichtfeld_densification_plugin_amd.core import hip_backend as hb


@pytest.fixture(scope="module")
def twin():
    t = hb.HostDensifier(2)
    yield t
    t.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run(twin, xyz, cell_size=0.0):
    out = twin.knn_dist2(torch.from_numpy(np.array(xyz, dtype=np.float32, copy=True)), cell_size)
    return out.numpy(), twin.knn_stats


@pytest.mark.parametrize("name", kr.ALL)
def test_twin_equals_brute_force_for_every_cell_size(twin, name):
    xyz, ref = kr.cloud(name), kr.reference(name)
    n = xyz.shape[0]
    seen = []
    for h in kr.cell_sizes(name):
        got, stats = run(twin, xyz, h)
        assert got.dtype == np.float32 and got.shape == (n,)
        assert np.array_equal(bits(got), bits(ref)), (name, h, int((bits(got) != bits(ref)).sum()))
        assert stats[0] > 0 and (h == 0.0 or stats[0] == h) and 1 <= stats[1] <= n and 1 <= stats[2] <= n and 0 <= stats[3] <= n
        seen.append(stats)
        print(name, "cell size", h, "stats", stats)
    if name in kr.FORCED and not name.startswith("d"):
        L = kr.longest_side(xyz)
        by_h = dict(zip(kr.cell_sizes(name), seen))
        assert by_h[10.0 * L][1] == 1 and by_h[10.0 * L][3] == 0          # one cell: ring 1 sees the whole cloud
        assert by_h[0.01 * L][3] > 0                                        # cells far smaller than the spacing: the brute-force pass runs
    if name == "c":
        assert int((ref == 0).sum()) == 4                                   # the four identical points: all-zero means (the record clamps them)
    if name == "d":
        assert np.array_equal(ref, np.full(n, 1.0, np.float32))             # the lattice: three neighbours at distance 1, ties everywhere


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_grid_path_does_the_work_on_a_surface_cloud(twin, seed):
    """(f): at most 1 % of the points may need the brute-force pass under the automatic cell size.  (The cloud has no point whose third neighbour
    is farther than 1.9 h at h = 2 L / ceil(sqrt(n)) - about 1.4 h is the farthest -: two rings settle every point, so the count should be 0.)"""
    xyz = kr.cloud(f"f{seed}")
    n = xyz.shape[0]
    h0 = 2.0 * kr.longest_side(xyz) / np.ceil(np.sqrt(n))
    assert kr.third_neighbour(xyz).max() <= 1.9 * h0
    got, stats = run(twin, xyz)
    print("stats", stats)
    assert stats[3] <= 0.01 * n
    assert np.array_equal(bits(got), bits(kr.reference(f"f{seed}")))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_far_outliers_do_not_put_the_cloud_into_one_cell(twin, seed):
    """(g): three far points inflate the box; the unrefined rule would give h = 54.5 and one cell for all of P.  The refinement has to work:
    the fullest cell holds at most 64 points and at most 16 points - only the far ones can need it - go through the brute-force pass."""
    xyz = kr.cloud(f"g{seed}")
    n = xyz.shape[0]
    h0 = 2.0 * kr.longest_side(xyz) / np.ceil(np.sqrt(n))
    assert abs(h0 - 54.5) < 0.1
    got, stats = run(twin, xyz)
    print("stats", stats)
    assert stats[0] < h0 and stats[2] <= 64 and stats[3] <= 16
    assert np.array_equal(bits(got), bits(kr.reference(f"g{seed}")))


def test_the_result_does_not_depend_on_the_threads_and_the_input_is_read_only():
    xyz = np.array(kr.cloud("g1"), copy=True)
    before = xyz.copy()
    outs = []
    for threads in (1, 3):
        t = hb.HostDensifier(threads)
        try:
            outs.append(run(t, xyz))
        finally:
            t.close()
    assert np.array_equal(bits(outs[0][0]), bits(outs[1][0])) and outs[0][1] == outs[1][1]
    assert np.array_equal(bits(xyz), bits(before))


def test_refusals_and_the_empty_cloud(twin):
    got, stats = run(twin, np.zeros((0, 3), np.float32))
    assert got.shape == (0,) and stats == (0.0, 0, 0, 0)
    for n in (1, 2, 3):
        with pytest.raises(hb.KnnInputRefused, match="fewer than four points"):
            run(twin, kr.cloud("a5")[:n])
    for bad in (np.nan, np.inf, -np.inf):
        xyz = np.array(kr.cloud("b65"), copy=True)
        xyz[17, 1] = bad
        with pytest.raises(hb.KnnInputRefused, match="non-finite coordinate"):
            run(twin, xyz)
    with pytest.raises(hb.KnnInputRefused, match="key range"):
        run(twin, kr.cloud("b65"), 1e-12)                                    # more than 2^30 cells along an axis
    with pytest.raises(hb.KnnInputRefused, match="key range"):
        run(twin, kr.cloud("b65"), 3e-8)                                     # every axis fits, the linear key does not
    for h in (-1.0, float("nan"), float("inf")):
        with pytest.raises(hb.HipBackendError, match="cell_size must be finite and >= 0") as e:
            run(twin, kr.cloud("b65"), h)
        assert not isinstance(e.value, hb.KnnInputRefused)
    with pytest.raises(ValueError, match="float32 tensor"):
        twin.knn_dist2(torch.zeros((5, 3), dtype=torch.float64))
    # the twin still works behind a refusal
    assert np.array_equal(bits(run(twin, kr.cloud("a4"))[0]), bits(kr.reference("a4")))


def make_inputs(seed, n):
    rs = np.random.RandomState(seed)
    xyz = rs.uniform(-2, 2, (n, 3)).astype(np.float32)
    nrm = rs.normal(size=(n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    nrm[0] = (0, 0, -1)                          # the flip
    nrm[1] = (0, 0, 1)
    nrm[2] = (0, 0, 0)                           # unusable: the identity
    nrm[3] = (np.nan, 0, 1)
    nrm[4] = (1, 0, 0)
    nrm[5] = (np.float32(3e-4), 0, np.float32(-1.0) + np.float32(2.0 ** -24))      # 1 + nz = 2^-24: still the flip
    nrm[6] = (np.float32(5e-4), 0, np.float32(-1.0) + np.float32(2.0 ** -23))      # 1 + nz = 2^-23: the formula
    rgb = rs.uniform(-0.1, 1.1, (n, 3)).astype(np.float32)
    rgb[7] = (np.nan, 0.5, np.float32(0.5 / 255.0))                                # NaN -> 0; a half: round to even
    d2 = (rs.uniform(0, 1, n) ** 4).astype(np.float32)
    d2[:3] = (0.0, 1e-9, 1e-7)
    return xyz, nrm, rgb, d2


@pytest.mark.parametrize("knobs", [dict(), dict(opacity=0.3, flatten=0.1), dict(flatten=0.5, max_scale=0.05), dict(max_scale=1e-30)])
def test_the_record_of_the_twin_is_the_numpy_formula(twin, knobs):
    xyz, nrm, rgb, d2 = make_inputs(4, 777)
    body = twin.pack_gaussians(*(torch.from_numpy(a) for a in (xyz, nrm, rgb, d2)), **knobs).numpy()
    assert body.dtype == np.uint8 and body.shape == (777 * 68,)
    got, ref = np.frombuffer(body.tobytes(), kr.REC68), kr.gaussian_records_ref(xyz, nrm, rgb, d2, **knobs)
    for col in ("xyz", "normal", "f_dc", "opacity", "rot"):
        assert got[col].tobytes() == ref[col].tobytes(), col
    # the scales: both sides round an f64 library log once; NumPy's and the C library's may differ in the f64's last place
    assert kr.ulp_distance(got["scale"], ref["scale"]).max() <= 1
    assert np.array_equal(got["rot"][:7], np.array([[0, 1, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0], [np.sqrt(np.float32(0.5)), 0, np.sqrt(np.float32(0.5)), 0],
                                                     [0, 1, 0, 0], got["rot"][6]], np.float32))
    assert got["rot"][6][0] > 0 and got["rot"][6][1] == 0 and got["rot"][6][2] > 0
    clamp = 0.5 * np.log(np.float64(np.float32(1e-7)))
    if not knobs.get("max_scale"):
        assert np.all(np.abs(got["scale"][:3, 0] - clamp) < 1e-6)            # 0, 1e-9 and 1e-7 all sit on the 3DGS clamp
    if knobs.get("max_scale") == 0.05:
        assert got["scale"][:, 0].max() <= np.float32(np.log(0.05)) + 1e-6 and (got["scale"][:, 0] < np.log(0.05) - 0.1).any()
    assert np.array_equal(got["scale"][:, 0], got["scale"][:, 1])
    shift = got["scale"][:, 2].astype(np.float64) - got["scale"][:, 0]
    assert np.all(np.abs(shift - np.log(knobs.get("flatten", 1.0))) < 1e-5)
    assert got["f_dc"][7].tobytes() == kr.dc_of_u8(np.array([0, 128, 0], np.uint8)).tobytes()


def test_pack_arguments_are_checked(twin):
    xyz, nrm, rgb, d2 = (torch.from_numpy(a) for a in make_inputs(1, 8))
    for kw in (dict(opacity=0.0), dict(opacity=1.0), dict(flatten=0.0), dict(flatten=1.5), dict(max_scale=-1.0), dict(max_scale=float("inf")),
               dict(opacity=float("nan"))):
        with pytest.raises(ValueError, match="opacity must be in"):
            twin.pack_gaussians(xyz, nrm, rgb, d2, **kw)
    with pytest.raises(ValueError, match="dist2 must be a float32 tensor of 8 rows"):
        twin.pack_gaussians(xyz, nrm, rgb, d2[:7])
    assert twin.pack_gaussians(xyz[:0], nrm[:0], rgb[:0], d2[:0]).shape == (0,)
