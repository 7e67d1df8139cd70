"""Oriented voxel fusion on the device (lfd_fuse_oriented through HipDensifier.fuse_oriented) against the CPU twin - both sides
are given the SAME arrays - at the smallest sizes that take every path: the smallest inputs, more voxels than a workgroup has threads, voxels
on both sides of the thread-per-voxel / wave-per-voxel boundary (64 | 65 points) and of the LDS staging boundary (256 | 257 | 513 points, the
pivot of the last in the second chunk), one voxel, no usable normal, a clustered cloud that needs several radix passes.  Row count, counts, xyz
and rgb are EQUAL; the normals are within one f32 ulp per component (the device divides through a refined reciprocal) and the number of
components that differ at all is printed.  A one-sided cloud equals lfd_voxel_downsample on the device bit for bit; and through the driver the
written file is pack_ply_normals of a direct call on the knob-off run's capped cloud."""
import os

import numpy as np
import pytest
import torch

import fuse_ref as fr
import support_scene as sc
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LFD_ERR_STATE = 4


@pytest.fixture(scope="module")
def dens():
    d = hb.HipDensifier(DEV)
    yield d
    d.close()


@pytest.fixture(scope="module")
def twin():
    d = hb.HostDensifier(16)
    yield d
    d.close()


def bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def within_one_ulp(a, b):
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32))


def both(dens, twin, xyz, nrm, rgb, h, tag=""):
    """one call on each side over the same arrays; the device's rows after comparing every output with the twin's"""
    t = lambda a, dev: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)).to(dev)      # noqa: E731
    ins = [t(a, DEV) for a in (xyz, nrm, rgb)]
    keep = [a.clone() for a in ins]
    d = dens.fuse_oriented(*ins, h, with_counts=True)
    nv_d = dens.fuse_voxels
    w = twin.fuse_oriented(*[t(a, "cpu") for a in (xyz, nrm, rgb)], h, with_counts=True)
    for a, b in zip(ins, keep):
        assert np.array_equal(bits(a), bits(b))                     # the inputs are read only
    assert d[0].shape == w[0].shape and nv_d == twin.fuse_voxels
    assert np.array_equal(bits(d[0]), bits(w[0])), "xyz"
    assert np.array_equal(bits(d[2]), bits(w[2])), "rgb"
    assert np.array_equal(d[3].cpu().numpy(), w[3].numpy()), "counts"
    assert int(d[3].sum()) == ins[0].shape[0]
    nd, nw = d[1].cpu().numpy(), w[1].numpy()
    differ = int((bits(nd) != bits(nw)).sum())
    print(f"{tag}: {ins[0].shape[0]} points, {nv_d} voxels, {d[0].shape[0]} rows; normal components that differ from the twin's: {differ} of {nd.size}")
    assert within_one_ulp(nd, nw).all() and np.array_equal(nd == 0.0, nw == 0.0)
    return d, nv_d


def voxel_of(rng, m, centre, two_sided=True, unusable_first=0):
    """m points inside one voxel of side 1 around `centre` (an integer triple), normals near +z, every other one flipped when two_sided"""
    xyz = (np.asarray(centre, np.float64) + rng.uniform(0.0, 0.4, (m, 3))).astype(np.float32)
    xyz[0] = centre                                                  # (the first voxel's first point is the cloud's minimum: see below)
    nrm = fr.unit(np.array([0.0, 0.0, 1.0]) + rng.normal(0.0, 0.2, (m, 3)))
    if two_sided:
        nrm[1::2] *= -1.0
    nrm = nrm.astype(np.float32)
    nrm[:unusable_first] = np.array([[0, 0, 0], [np.nan, 0, 1], [np.inf, 0, 0]], np.float32)[np.arange(unusable_first) % 3]
    return xyz, nrm, rng.uniform(0.0, 1.0, (m, 3)).astype(np.float32)


class Node:
    """A camera node as the GUI hands it to dense_init_from_lfs."""

    def __init__(self, cam):
        self.has_camera, self.camera_uid = True, cam.uid
        self.camera_width, self.camera_height = cam.width, cam.height
        self.camera_focal_x, self.camera_focal_y = float(cam.K[0, 0]), float(cam.K[1, 1])
        self.camera_R, self.camera_T = cam.R, cam.t.reshape(3)
        self.image_path, self.has_mask, self.mask_path = cam.image_path, False, None


def test_the_smallest_inputs(dens, twin):
    e = np.zeros((0, 3), np.float32)
    rows = dens.fuse_oriented(*[torch.from_numpy(e).to(DEV)] * 3, 0.1, with_counts=True)
    assert rows[0].shape == (0, 3) and rows[3].shape == (0,) and dens.fuse_voxels == 0
    both(dens, twin, [[1, 2, 3]], [[0, 1, 0]], [[0.2, 0.4, 0.6]], 0.1, "n = 1")
    two = np.array([[0.0, 0.0, 0.0], [0.01, 0.0, 0.0]], np.float32)
    d, nv = both(dens, twin, two, [[0, 0, 1], [0, 0, -1]], np.full_like(two, 0.5), 1.0, "n = 2, opposite")
    assert d[0].shape[0] == 2 and nv == 1
    d, nv = both(dens, twin, two, [[0, 0, 1], [0, 0, 1]], np.full_like(two, 0.5), 1.0, "n = 2, same")
    assert d[0].shape[0] == 1 and nv == 1


def test_more_voxels_than_a_workgroup_has_threads(dens, twin):
    xyz, nrm, rgb = fr.uniform_cloud(4, 257)
    d, nv = both(dens, twin, xyz, nrm, rgb, 1e-4, "257 voxels")
    assert nv == 257 == d[0].shape[0]


@pytest.mark.parametrize("m,unusable_first", [(64, 0), (65, 0), (256, 0), (257, 0), (513, 300)])
def test_voxels_at_the_path_boundaries(dens, twin, m, unusable_first):
    """a voxel of m points among small ones: 64 | 65 is thread per voxel | wave per voxel, 256 | 257 | 513 the staging chunks; with 300 unusable
    normals in front the pivot of the 513-point voxel lies in its second chunk"""
    rng = np.random.default_rng(100 + m)
    parts = [voxel_of(rng, m, (0, 0, 0), True, unusable_first), voxel_of(rng, 7, (3, 0, 0)), voxel_of(rng, 1, (0, 2, 0)), voxel_of(rng, 3, (5, 5, 5), False)]
    xyz, nrm, rgb = (np.concatenate([p[k] for p in parts]) for k in range(3))
    assert (xyz.min(axis=0) == 0.0).all()                            # origin = min - h / 2 = -0.5: the voxels of side 1 are centred on the integer triples
    d, nv = both(dens, twin, xyz, nrm, rgb, 1.0, f"voxel of {m}")
    cnt = d[3].cpu().numpy()
    ref = fr.fuse_ref(xyz, nrm, rgb, 1.0)
    assert nv == ref[5] and np.array_equal(cnt, ref[3]) and np.array_equal(bits(d[0]), bits(ref[0]))
    assert cnt[0] + cnt[1] == m and min(cnt[0], cnt[1]) > 0.25 * (m - unusable_first)        # the large voxel comes first and is two-sided
    # shuffled: the voxel's points are spread over the input, the sums still run in ascending input index
    perm = rng.permutation(xyz.shape[0])
    both(dens, twin, xyz[perm], nrm[perm], rgb[perm], 1.0, f"voxel of {m}, shuffled")


def test_all_points_in_one_voxel_and_no_usable_normal(dens, twin):
    xyz, nrm, rgb = fr.clustered_cloud(9, 3001, n_clusters=6)
    d, nv = both(dens, twin, xyz, nrm, rgb, 50.0, "one voxel")
    assert nv == 1 and d[0].shape[0] == 2
    for bad in (np.zeros_like(nrm), np.full_like(nrm, np.nan)):
        d, nv = both(dens, twin, xyz, bad, rgb, 0.1, "no usable normal")
        assert d[0].shape[0] == nv and not d[1].cpu().numpy().any()
        v = dens.voxel_downsample(torch.from_numpy(xyz).to(DEV), torch.from_numpy(rgb).to(DEV), 0.1)
        assert np.array_equal(bits(d[0]), bits(v[0])) and np.array_equal(bits(d[2]), bits(v[1]))


def test_a_clustered_cloud_over_several_radix_passes(dens, twin):
    xyz, nrm, rgb = fr.clustered_cloud(31, 100003, n_clusters=300, spread=0.01, flip=0.7)
    d, nv = both(dens, twin, xyz, nrm, rgb, 0.01, "clustered")       # about 200 voxels along every axis: a 23-bit key, three radix passes
    two = d[0].shape[0] - nv
    assert nv > 5000 and 0.2 < two / nv < 0.45                       # about a third of the voxels are two-sided
    d, nv = both(dens, twin, xyz, nrm, rgb, 0.08, "clustered, large voxels")
    assert int(d[3].max()) > 256                                     # ... and voxels on the wave path


@pytest.mark.parametrize("h", [0.02, 0.3])
def test_a_one_sided_cloud_equals_the_voxel_filter_on_the_device(dens, twin, h):
    xyz, nrm, rgb = fr.one_sided_cloud(21, 20011)
    d, nv = both(dens, twin, xyz, nrm, rgb, h, "one-sided")
    v = dens.voxel_downsample(torch.from_numpy(xyz).to(DEV), torch.from_numpy(rgb).to(DEV), h)
    assert d[0].shape[0] == nv == v[0].shape[0]
    assert np.array_equal(bits(d[0]), bits(v[0])) and np.array_equal(bits(d[2]), bits(v[1]))


def test_colour_scales(dens, twin):
    xyz, nrm, rgb = fr.clustered_cloud(8, 5000, n_clusters=20)
    d, _ = both(dens, twin, xyz, nrm, np.round(rgb * 255.0), 0.05, "colours 0..255")
    assert 0.5 < float(d[2].max()) <= 1.0
    withnan = rgb.copy()
    withnan[5, 1] = np.nan
    withnan[7] = 200.0
    d, _ = both(dens, twin, xyz, nrm, withnan, 0.05, "a NaN colour")
    assert bool(torch.isnan(d[2]).any()) and float(d[2][~torch.isnan(d[2])].max()) > 1.0


def test_both_data_refusals_and_the_other_context_s_entry_point(dens, twin):
    xyz, nrm, rgb = fr.uniform_cloud(1, 500)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)                          # noqa: E731
    bad = xyz.copy()
    bad[3, 1] = np.nan
    with pytest.raises(hb.FuseInputRefused, match="non-finite coordinate"):
        dens.fuse_oriented(t(bad), t(nrm), t(rgb), 0.1)
    with pytest.raises(hb.FuseInputRefused, match="key range"):
        dens.fuse_oriented(t(xyz * np.float32(1e30)), t(nrm), t(rgb), 1e-30)
    both(dens, twin, xyz, nrm, rgb, 0.1, "after the refusals")
    null = (None, None, None, 0, 1.0, None, None, None, None, None, None)
    assert dens._lib.lfd_fuse_oriented_host(dens._ctx, *null) == LFD_ERR_STATE
    assert twin._lib.lfd_fuse_oriented(twin._ctx, *null) == LFD_ERR_STATE


def test_launches_share_the_context_s_workspace(dens, twin):
    small = fr.clustered_cloud(2, 900, n_clusters=5)
    large = fr.clustered_cloud(3, 30000, n_clusters=50)
    a, _ = both(dens, twin, *small, 0.05, "small")
    first = [x.clone() for x in a]
    both(dens, twin, *small, 0.05, "small again")
    both(dens, twin, *large, 0.05, "large")
    b, _ = both(dens, twin, *small, 0.05, "small after large")
    for x, y in zip(first, b):
        assert np.array_equal(bits(x), bits(y))


def test_the_cloud_and_the_normals_of_the_dense_kernel(dens, twin):
    dens.upload_cameras(sc.cameras())
    refs = [sc.reference_inputs(r, 3, 48, 64, device=DEV)[1] for r in (10, 11, 12, 13)]
    batch = hb.PreparedBatch(refs, sc.MATCH, sc.MATCH)
    out = dens.triangulate_dense(batch, sc.params())
    out = dens.estimate_normals(batch, out, 2, 0.05, 1.5)
    dens.check_launches()
    assert out.count > 4000
    xyz, nrm, rgb = out.xyz.cpu().numpy(), out.normals.cpu().numpy(), out.rgb.cpu().numpy()
    spacing = float(np.median(np.linalg.norm(xyz[1:] - xyz[:-1], axis=1)))
    d, nv = both(dens, twin, xyz, nrm, rgb, 3.0 * spacing, "dense kernel")
    assert nv < out.count / 2                                         # the four references overlap: the stage merges


@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_the_driver_writes_the_fused_cloud(tmp_path, monkeypatch, mode):
    """dense_init_from_lfs on the device: the file is pack_ply_normals of a direct fuse_oriented call on the knob-off run's capped cloud"""
    import cycle_scene
    import lichtfeld_densification_plugin_amd as lfd
    from lichtfeld_densification_plugin_amd import densify, synthetic
    from lichtfeld_densification_plugin_amd.core.writers import ply_header
    scene = cycle_scene.make_scene(str(tmp_path / "scene"), n_cams=4)
    nodes = [Node(c) for c in scene["cams"]]
    recs = densify.extract_cameras_from_lfs(nodes)
    seen = {}
    plain = densify._write_output

    def spy(path, xyz, rgb, err, device_points=None, clock=None, as_ply=None, normals=None):
        seen[os.path.basename(path)] = (device_points[0].clone(), normals.clone(), device_points[1].clone())
        return plain(path, xyz, rgb, err, device_points, clock=clock, as_ply=as_ply, normals=normals)
    monkeypatch.setattr(densify, "_write_output", spy)

    def run(name, exp):
        matcher = synthetic.SyntheticMatcher(recs, setting="turbo", device=DEV, channels=2)
        cfg = lfd.DensePipelineConfig(output_path=str(tmp_path / name), num_refs=0.75, nns_per_ref=3, seed=3, viz_interval=0, matches_per_ref=2500,
                                      pack_workers=1, triangulation_mode=mode, max_points=4000, experimental={"estimate_normals": True, **exp})
        msgs = []
        assert densify.dense_init_from_lfs(nodes, cfg, progress_callback=lambda p, m: msgs.append(m), matcher=matcher)[0] == 0
        return msgs
    h = 0.05
    assert "Fusing oriented points..." not in run("off.ply", {})
    assert "Fusing oriented points..." in run("on.ply", {"fuse_voxel_size": h})
    xyz, nrm, rgb = seen["off.ply"]                                   # what the knob-off run packed: its cloud and normals behind the cap
    assert xyz.is_cuda and 0 < xyz.shape[0] <= 4000
    d = hb.HipDensifier(DEV)
    try:
        rows = d.fuse_oriented(xyz, nrm, rgb, h)
        body = d.pack_ply_normals(rows[0], rows[1], rows[2]).cpu().numpy().tobytes()
    finally:
        d.close()
    n_rows = int(rows[0].shape[0])
    assert 0 < n_rows < xyz.shape[0]
    assert open(str(tmp_path / "on.ply"), "rb").read() == ply_header(n_rows, True) + body
