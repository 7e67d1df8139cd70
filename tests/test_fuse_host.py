"""The twin of oriented voxel fusion (lfd_fuse_oriented_host) against the NumPy reference of the rule (tests/fuse_ref.py): every
output is EQUAL - the normals included, both sides use IEEE f64 sqrt and divide -, on uniform and clustered clouds at five voxel sizes, with
degenerate normals, on the smallest inputs, on voxel faces, with both colour scales; a one-sided cloud gives the plain voxel mean bit for bit;
and the two scenes that say what the stage is for: averaging the normals' noise down, and keeping the two faces of a thin wall apart."""
import numpy as np
import pytest
import torch

import fuse_ref as fr
from lichtfeld_densification_plugin_amd import densify
from lichtfeld_densification_plugin_amd.core import hip_backend as hb


@pytest.fixture(scope="module")
def twin():
    t = hb.HostDensifier(2)
    yield t
    t.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run(twin, xyz, nrm, rgb, h):
    x, n, c, cnt = twin.fuse_oriented(*(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)) for a in (xyz, nrm, rgb)), h,
                                      with_counts=True)
    return x.numpy(), n.numpy(), c.numpy(), cnt.numpy().astype(np.int64), twin.fuse_voxels


def check(twin, xyz, nrm, rgb, h):
    """twin == reference in every output; returns the reference's tuple"""
    before = [np.array(a, copy=True) for a in (xyz, nrm, rgb)]
    got = run(twin, xyz, nrm, rgb, h)
    ref = fr.fuse_ref(xyz, nrm, rgb, h)
    assert got[0].shape == ref[0].shape and got[4] == ref[5]
    for k in range(3):
        assert np.array_equal(bits(got[k]), bits(ref[k])), ("xyz", "normals", "rgb")[k]
    assert np.array_equal(got[3], ref[3]) and int(got[3].sum()) == np.asarray(xyz).reshape(-1, 3).shape[0]
    assert ref[5] <= ref[0].shape[0] <= min(2 * ref[5], max(1, np.asarray(xyz).reshape(-1, 3).shape[0]))
    for a, b in zip((xyz, nrm, rgb), before):
        assert np.array_equal(bits(a), bits(b))                 # the inputs are read only
    return ref


@pytest.mark.parametrize("kind", ["uniform", "clustered"])
@pytest.mark.parametrize("h", [1e-4, 0.03, 0.11, 0.5, 8.0])
def test_twin_equals_the_reference(twin, kind, h):
    xyz, nrm, rgb = fr.uniform_cloud(11, 3000) if kind == "uniform" else fr.clustered_cloud(12, 4000)
    ref = check(twin, xyz, nrm, rgb, h)
    if h == 1e-4 and kind == "uniform":
        assert ref[5] == ref[0].shape[0] == 3000                # every point alone
    if h == 8.0:
        assert ref[5] == 1                                      # one voxel
    if kind == "clustered" and h == 0.11:
        assert 0 < int((ref[4] == 1).sum()) < ref[5]            # some voxels are two-sided, not all


def test_degenerate_normals(twin):
    xyz, nrm, rgb = fr.clustered_cloud(5, 2000, n_clusters=12)
    rng = np.random.default_rng(6)
    bad = rng.choice(2000, 600, replace=False)
    nrm[bad[:200]] = 0.0
    nrm[bad[200:400], rng.integers(0, 3, 200)] = np.nan
    nrm[bad[400:500], rng.integers(0, 3, 100)] = np.inf
    nrm[bad[500:600], rng.integers(0, 3, 100)] = -np.inf
    nrm[:40] = 0.0                                              # ... among them the first points of their voxels
    nrm[40:60] = np.nan
    nrm[60] = [1e-30, 0.0, 0.0]                                 # usable: its square is a normal f64
    nrm[61] = [3e38, 3e38, -3e38]                               # usable, and far from overflowing the f64 sums
    for h in (0.05, 0.3, 4.0):
        check(twin, xyz, nrm, rgb, h)
    # an unusable first point is not the pivot: the voxel's side 0 is the side of its first USABLE normal
    x = np.zeros((3, 3), np.float32)
    n3 = np.array([[np.nan, 0, 0], [0, 0, -1], [0, 0, 1]], np.float32)
    ref = check(twin, x, n3, np.zeros_like(x), 1.0)
    assert ref[3].tolist() == [2, 1] and ref[1][0].tolist() == [0, 0, -1] and ref[1][1].tolist() == [0, 0, 1]


def test_all_normals_unusable_gives_the_voxel_mean_and_zero_normals(twin):
    xyz, _, rgb = fr.uniform_cloud(3, 1500)
    for nrm in (np.zeros_like(xyz), np.full_like(xyz, np.nan)):
        ref = check(twin, xyz, nrm, rgb, 0.25)
        vx, vc = fr.voxel_mean_ref(xyz, rgb, 0.25)
        assert np.array_equal(bits(ref[0]), bits(vx)) and np.array_equal(bits(ref[2]), bits(vc)) and not ref[1].any() and not ref[4].any()


def test_the_smallest_inputs(twin):
    e = np.zeros((0, 3), np.float32)
    got = run(twin, e, e, e, 0.1)
    assert got[0].shape == (0, 3) and got[3].shape == (0,) and got[4] == 0
    one = check(twin, np.array([[1, 2, 3]], np.float32), np.array([[0, 1, 0]], np.float32), np.array([[0.2, 0.4, 0.6]], np.float32), 0.1)
    assert one[0].shape == (1, 3) and one[0][0].tolist() == [1, 2, 3] and one[1][0].tolist() == [0, 1, 0]
    two = np.array([[0.0, 0.0, 0.0], [0.01, 0.0, 0.0]], np.float32)
    up = np.array([[0, 0, 1], [0, 0, 1]], np.float32)
    opposite = check(twin, two, up * np.array([[1], [-1]], np.float32), np.ones_like(two) * 0.5, 1.0)
    assert opposite[0].shape == (2, 3) and opposite[4].tolist() == [0, 1] and opposite[5] == 1
    assert opposite[1].tolist() == [[0, 0, 1], [0, 0, -1]]
    same = check(twin, two, up, np.ones_like(two) * 0.5, 1.0)
    assert same[0].shape == (1, 3) and same[3].tolist() == [2]
    apart = check(twin, two, up, np.ones_like(two) * 0.5, 0.001)
    assert apart[0].shape == (2, 3) and apart[5] == 2


def test_points_on_voxel_faces(twin):
    # origin = min - h / 2: with h = 0.5 and min = 0 the coordinates 0.25 + 0.5 k lie exactly on faces
    g = np.stack(np.meshgrid(*[np.arange(6)] * 3, indexing="ij"), -1).reshape(-1, 3)
    xyz = (g * 0.25).astype(np.float32)
    rng = np.random.default_rng(2)
    nrm = fr.unit(rng.normal(size=xyz.shape)).astype(np.float32)
    check(twin, xyz, nrm, rng.uniform(0, 1, xyz.shape).astype(np.float32), 0.5)
    check(twin, xyz[rng.permutation(len(xyz))], nrm, np.zeros_like(xyz), 0.25)


def test_colour_scales(twin):
    xyz, nrm, rgb = fr.clustered_cloud(8, 1200, n_clusters=10)
    ref255 = check(twin, xyz, nrm, np.round(rgb * 255.0).astype(np.float32), 0.2)
    assert ref255[2].max() <= 1.0 and ref255[2].max() > 0.5
    withnan = rgb.copy()
    withnan[5, 1] = np.nan
    withnan[7] = 200.0                                          # a NaN maximum: the scale stays 1 whatever else is there
    ref = check(twin, xyz, nrm, withnan, 0.2)
    assert np.isnan(ref[2]).any() and np.nanmax(ref[2]) > 1.0


@pytest.mark.parametrize("h", [0.02, 0.2, 0.7])
def test_a_one_sided_cloud_is_the_voxel_filter_bit_for_bit(twin, h):
    xyz, nrm, rgb = fr.one_sided_cloud(21, 3500)
    d = nrm.astype(np.float64) @ nrm.astype(np.float64).T
    assert d.min() > 0.0                                        # the precondition: no two normals oppose each other
    got = run(twin, xyz, nrm, rgb, h)
    vx, vc = densify._voxel_downsample(xyz, rgb, h)             # (Open3D is not installed: the NumPy branch runs)
    assert got[0].shape == vx.shape and np.array_equal(bits(got[0]), bits(vx)) and np.array_equal(bits(got[2]), bits(vc))
    assert got[4] == vx.shape[0]
    check(twin, xyz, nrm, rgb, h)


def test_refusals_raise_their_own_exception(twin):
    xyz, nrm, rgb = fr.uniform_cloud(1, 50)
    bad = xyz.copy()
    bad[3, 1] = np.inf
    t = lambda a: torch.from_numpy(a)                           # noqa: E731
    with pytest.raises(hb.FuseInputRefused, match="non-finite coordinate"):
        twin.fuse_oriented(t(bad), t(nrm), t(rgb), 0.1)
    with pytest.raises(hb.FuseInputRefused, match="key range"):
        twin.fuse_oriented(t(xyz * np.float32(1e30)), t(nrm), t(rgb), 1e-30)
    with pytest.raises(hb.HipBackendError, match="voxel_size") as e:
        twin.fuse_oriented(t(xyz), t(nrm), t(rgb), 0.0)
    assert not isinstance(e.value, hb.FuseInputRefused)
    with pytest.raises(ValueError, match="normals"):
        twin.fuse_oriented(t(xyz), t(nrm[:10]), t(rgb), 0.1)


def test_usefulness_noise_is_averaged_down_on_a_plane(twin):
    """Six references see one plane; each normal carries about 10 degrees of noise.  Six iid samples cut the error by sqrt(6) = 2.45; the bound is 2,
    which leaves room for the small-angle approximation."""
    xyz, nrm, rgb, n0 = fr.tilted_plane_scene()
    h = 0.02
    e_in = fr.angle_deg(nrm, n0)
    assert 6.0 < np.median(e_in) < 14.0                         # the input really is that noisy
    x, n, c, cnt, nv = run(twin, xyz, nrm, rgb, h)
    ref = fr.fuse_ref(xyz, nrm, rgb, h)
    assert np.array_equal(bits(n), bits(ref[1])) and np.array_equal(cnt, ref[3])
    assert x.shape[0] == nv and not ref[4].any()                # no two-sided rows
    big = cnt >= 6
    assert big.mean() >= 0.8
    e_out = fr.angle_deg(n[big], n0)
    print(f"plane: {xyz.shape[0]} points -> {x.shape[0]} rows, median error in {np.median(e_in):.2f} deg, out {np.median(e_out):.2f} deg, "
          f"ratio {np.median(e_in) / np.median(e_out):.2f}, share of rows with count >= 6: {big.mean():.3f}")
    assert np.median(e_out) <= 0.5 * np.median(e_in)


def test_usefulness_the_two_faces_of_a_thin_wall_stay_apart(twin):
    xyz, nrm, rgb = fr.thin_wall_scene()
    h = 0.05
    z = xyz[:, 2].astype(np.float64)
    front = z < 0.02
    assert (np.abs(z[front] - 0.010) < 0.0025).all() and (np.abs(z[~front] - 0.030) < 0.0025).all()     # two faces 0.4 h apart
    assert (nrm[front, 2] < 0).all() and (nrm[~front, 2] > 0).all()                                      # opposite normals
    assert fr.angle_deg(nrm[front], [0, 0, -1.0]).max() < 60.0 and fr.angle_deg(nrm[~front], [0, 0, 1.0]).max() < 60.0
    x, n, c, cnt, nv = run(twin, xyz, nrm, rgb, h)
    ref = fr.fuse_ref(xyz, nrm, rgb, h)
    assert np.array_equal(bits(x), bits(ref[0])) and np.array_equal(bits(n), bits(ref[1]))
    assert x.shape[0] == 2 * nv                                 # every occupied voxel gives two rows
    zr = x[:, 2].astype(np.float64)
    near_front, near_back = np.abs(zr - 0.010) <= 0.002, np.abs(zr - 0.030) <= 0.002
    assert (near_front | near_back).all() and near_front.sum() == near_back.sum() == nv
    assert ((n[:, 2] < 0) == near_front).all() and ((n[:, 2] > 0) == near_back).all()
    assert not ((zr > 0.013) & (zr < 0.027)).any()              # no row between the faces
    vx, _ = fr.voxel_mean_ref(xyz, rgb, h)
    assert vx.shape[0] == nv and ((vx[:, 2] > 0.013) & (vx[:, 2] < 0.027)).all()       # ... where the plain voxel mean puts every one of its points
    print(f"wall: {xyz.shape[0]} points -> {x.shape[0]} rows in {nv} voxels; the plain voxel mean: {vx.shape[0]} points, all between the faces")
