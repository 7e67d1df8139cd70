"""The distance filter on the device (lfd_voxel_downsample / HipDensifier.voxel_downsample / the GUI route of densify.dense_init_from_lfs)
against its reference, the NumPy branch of densify._voxel_downsample: the same values and the same order, bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

import lichtfeld_densification_plugin_amd as lfd
from lichtfeld_densification_plugin_amd import densify, synthetic
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from lichtfeld_densification_plugin_amd.core import pipeline as pl
from lichtfeld_densification_plugin_amd.core import writers
from lichtfeld_densification_plugin_amd.core.image_io import to_uint8_rgb
from lichtfeld_densification_plugin_amd.core.sinks import PipelineResult
from test_gpu_pipeline import FakeMatcher, _Node, _scene

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(autouse=True)
def numpy_branch(monkeypatch):
    """the reference is the NumPy branch, whatever is installed"""
    monkeypatch.setitem(sys.modules, "open3d", None)


@pytest.fixture(scope="module")
def dens():
    d = hb.HipDensifier(DEV)
    yield d
    d.close()


def _cloud(n, dist, seed, scale255=False):
    rng = np.random.default_rng(seed)
    if dist == "normal":
        xyz = rng.normal(scale=2.0, size=(n, 3))
    elif dist == "uniform":
        xyz = rng.uniform(-5.0, 5.0, size=(n, 3))
    else:                                                    # clustered: a few tight blobs, many points per voxel
        centres = rng.normal(scale=3.0, size=(8, 3))
        xyz = centres[rng.integers(0, 8, n)] + rng.normal(scale=0.02, size=(n, 3))
    rgb = rng.random((n, 3))
    if scale255:
        rgb = np.round(rgb * 255.0)
    return xyz.astype(np.float32), rgb.astype(np.float32)


def _check(dens, xyz, rgb, vs):
    exp_x, exp_c = densify._voxel_downsample(xyz, rgb, vs)
    got_x, got_c = dens.voxel_downsample(torch.from_numpy(xyz).to(DEV), torch.from_numpy(rgb).to(DEV), vs)
    assert got_x.dtype == torch.float32 and got_c.dtype == torch.float32
    np.testing.assert_array_equal(got_x.cpu().numpy(), exp_x)
    np.testing.assert_array_equal(got_c.cpu().numpy(), exp_c)
    return got_x, got_c


@pytest.mark.parametrize("vs", [0.001, 0.01, 0.1, 3.7])
@pytest.mark.parametrize("dist", ["normal", "uniform", "clustered"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4097])
def test_small_clouds(dens, n, dist, vs):
    xyz, rgb = _cloud(n, dist, seed=n * 7 + len(dist))
    _check(dens, xyz, rgb, vs)


@pytest.mark.parametrize("vs", [0.001, 0.01, 0.1, 3.7])
@pytest.mark.parametrize("dist", ["normal", "uniform", "clustered"])
def test_million_point_clouds(dens, dist, vs):
    xyz, rgb = _cloud(1_000_003, dist, seed=11)
    _check(dens, xyz, rgb, vs)


@pytest.mark.parametrize("n", [65, 4097, 1_000_003])
def test_colours_scaled_to_255(dens, n):
    xyz, rgb = _cloud(n, "clustered", seed=3, scale255=True)
    assert rgb.max() > 1.0
    _check(dens, xyz, rgb, 0.01)


def test_nan_colour_keeps_unit_scale(dens):
    # NumPy's max propagates NaN, so one NaN colour means s = 1 even beside 0..255 colours
    xyz, rgb = _cloud(5000, "normal", seed=4, scale255=True)
    rgb[17, 1] = np.nan
    _check(dens, xyz, rgb, 0.1)


@pytest.mark.parametrize("vs", [0.25, 0.1])
def test_coordinates_on_voxel_faces(dens, vs):
    rng = np.random.default_rng(5)
    xyz = (rng.integers(-40, 40, size=(20000, 3)).astype(np.float32) * np.float32(vs))
    xyz[::7] += np.float32(vs / 2)                           # some points between faces as well
    rgb = rng.random((20000, 3)).astype(np.float32)
    _check(dens, xyz, rgb, vs)


def test_million_points_in_one_voxel(dens):
    rng = np.random.default_rng(6)
    xyz = rng.uniform(1.0, 1.001, size=(1_000_000, 3)).astype(np.float32)
    rgb = rng.random((1_000_000, 3)).astype(np.float32)
    got_x, _ = _check(dens, xyz, rgb, 3.7)
    assert got_x.shape[0] == 1


def _dense_survivors(n_refs=16):
    """a dense-mode survivor cloud of the bench's kind: ring cameras, analytic warps at the 'fast' preset, the fused dense kernel"""
    h_lr, w_lr, H, W = synthetic.ROMA_PRESETS["fast"]
    cams = synthetic.ring_cameras(185, seed=0)
    d = hb.HipDensifier(DEV)
    try:
        d.upload_cameras(cams)
        refs = []
        for g in range(n_refs):
            ref = (3 * g) % 185
            nbrs = synthetic.ring_neighbours(185, ref, 3)
            s = synthetic.synth_reference(cams, ref, nbrs, H, W, w_lr, h_lr, noise_px=0.5, outlier_frac=0.05, channels=2, seed=1000 + g,
                                          cert_mode="smooth", device=DEV)
            refs.append(hb.ReferenceInputs(ref_cam=ref, nbr_cams=nbrs, cert=list(s.cert), warp=list(s.warp), image=s.image))
        cfg = lfd.DensePipelineConfig(output_path="", triangulation_mode="dense")
        out = d.triangulate_dense(hb.PreparedBatch(refs, w_lr, h_lr), hb.make_params(cfg))
        return out.xyz.clone(), out.rgb.clone()
    finally:
        d.close()


def test_dense_mode_survivor_cloud(dens):
    xyz_t, rgb_t = _dense_survivors()
    assert xyz_t.shape[0] >= 2_000_000, xyz_t.shape
    xyz, rgb = xyz_t.cpu().numpy(), rgb_t.cpu().numpy()
    _check(dens, xyz, rgb, 0.01)


def test_repeatable(dens):
    xyz, rgb = _cloud(1_000_003, "normal", seed=8)
    a = dens.voxel_downsample(torch.from_numpy(xyz).to(DEV), torch.from_numpy(rgb).to(DEV), 0.01)
    b = dens.voxel_downsample(torch.from_numpy(xyz).to(DEV), torch.from_numpy(rgb).to(DEV), 0.01)
    assert a[0].cpu().numpy().tobytes() == b[0].cpu().numpy().tobytes()
    assert a[1].cpu().numpy().tobytes() == b[1].cpu().numpy().tobytes()


def test_empty_cloud(dens):
    x, c = dens.voxel_downsample(torch.empty((0, 3), dtype=torch.float32, device=DEV), torch.empty((0, 3), dtype=torch.float32, device=DEV), 0.01)
    assert x.shape == (0, 3) and c.shape == (0, 3)


def _refused_clouds():
    xyz, rgb = _cloud(3000, "normal", seed=9)
    inf = xyz.copy()
    inf[1234, 2] = np.inf
    nan = xyz.copy()
    nan[77, 0] = np.nan
    wide = np.random.default_rng(10).uniform(0.0, 5000.0, size=(3000, 3)).astype(np.float32)   # ~5e6 keys per axis: > 2^63 cells
    return {"inf": (inf, rgb, 0.01), "nan": (nan, rgb, 0.01), "key_range": (wide, rgb, 0.001)}


@pytest.mark.parametrize("case", ["inf", "nan", "key_range"])
def test_refusals_raise_the_dedicated_exception(dens, case):
    xyz, rgb, vs = _refused_clouds()[case]
    with pytest.raises(hb.VoxelInputRefused):
        dens.voxel_downsample(torch.from_numpy(xyz).to(DEV), torch.from_numpy(rgb).to(DEV), vs)


def test_other_errors_are_not_refusals(dens):
    xyz, rgb = _cloud(10, "normal", seed=1)
    with pytest.raises(hb.HipBackendError) as e:
        dens.voxel_downsample(torch.from_numpy(xyz).to(DEV), torch.from_numpy(rgb).to(DEV), 0.0)
    assert not isinstance(e.value, hb.VoxelInputRefused)


# ---- the GUI entry point ---------------------------------------------------------------------------------------------------------------------
class Replay(FakeMatcher):
    def match_grids_batch(self, imA, imB_list):
        res = self.table[self.calls % len(self.table)]
        self.calls += 1
        return [(res[j % len(res)][0], res[j % len(res)][1]) for j in range(len(imB_list))]


def _gui_run(nodes, table, out, mode, msgs, **over):
    kw = dict(nns_per_ref=2, num_refs=3, seed=5, viz_interval=0, matches_per_ref=1200, max_points=2000, voxel_size=0.01, triangulation_mode=mode)
    kw.update(over)
    cfg = lfd.DensePipelineConfig(output_path=out, **kw)
    return densify.dense_init_from_lfs(nodes, cfg, progress_callback=lambda p, m: msgs.append((p, m)), matcher=Replay(64, 64, table))


def _no_host_arrays(self, i):
    raise AssertionError("the f32 cloud was brought to the host")


@pytest.mark.parametrize("name", ["dense.ply", "dense_points"])
@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_gui_route_matches_the_host_route(g4, tmp_path, monkeypatch, mode, name):
    cams, refs, nn, table = _scene(g4, str(tmp_path))
    nodes = [_Node(c, float(c.K[0, 0]), float(c.K[1, 1])) for c in cams]
    out = os.path.join(str(tmp_path), "gui", name)
    msgs = []
    with monkeypatch.context() as m:
        m.setattr(PipelineResult, "_get", _no_host_arrays)
        code, info = _gui_run(nodes, table, out, mode, msgs)
    assert code == 0 and info == out and os.path.isfile(out)
    raw = open(out, "rb").read()
    assert raw.startswith(b"ply\n")                           # a PLY whatever the name
    n = int(raw.split(b"element vertex ")[1].split(b"\n")[0])
    assert 0 < n <= 2000
    # reference: the pipeline's result, the cap, the NumPy filter, the host writer
    recs = densify.extract_cameras_from_lfs(nodes)
    flat = np.stack([c.flat_pose() for c in recs])
    from lichtfeld_densification_plugin_amd.core.selection import nearest_neighbors, select_cameras_kcenters
    cfg2 = lfd.DensePipelineConfig(output_path=os.path.join(str(tmp_path), "reference.ply"), nns_per_ref=2, num_refs=3, seed=5, viz_interval=0,
                                   matches_per_ref=1200, max_points=2000, voxel_size=0.01, triangulation_mode=mode)
    res = pl.run_dense_pipeline(recs, select_cameras_kcenters(flat, 3), nearest_neighbors(flat, 2), cfg2, matcher=Replay(64, 64, table))
    x, c, _ = densify._apply_point_cap(res.xyz, res.rgb, res.err, 2000, 5)
    xv, cv = densify._voxel_downsample(x, c, 0.01)
    writers.write_ply(cfg2.output_path, xv, to_uint8_rgb(cv))
    assert open(cfg2.output_path, "rb").read() == raw
    # the host route (the device filter out of the way) says and writes the same
    host_out = os.path.join(str(tmp_path), "host", name)
    host_msgs = []
    with monkeypatch.context() as m:
        m.setattr(densify, "_voxel_filter_on_device", lambda pts, vs: None)
        code2, _ = _gui_run(nodes, table, host_out, mode, host_msgs)
    assert code2 == 0 and open(host_out, "rb").read() == raw
    # the same milestones; after the pipeline (93 %: the filter) the same words (before it the messages carry measured rates)
    assert [p for p, _ in msgs] == [p for p, _ in host_msgs]
    assert [m for m in msgs if m[0] >= 93.0] == [m for m in host_msgs if m[0] >= 93.0]
    assert (93.0, "Applying distance filter...") in msgs


@pytest.mark.parametrize("case", ["inf", "nan", "key_range"])
def test_gui_route_falls_back_to_the_host_on_refusal(g4, tmp_path, monkeypatch, case):
    cams, _, _, table = _scene(g4, str(tmp_path))
    nodes = [_Node(c, float(c.K[0, 0]), float(c.K[1, 1])) for c in cams]
    xyz, rgb, vs = _refused_clouds()[case]
    err = np.zeros((xyz.shape[0],), np.float32)

    def fake_run(*args, **kwargs):
        dev = tuple(torch.from_numpy(a).to(DEV) for a in (xyz, rgb, err))
        return PipelineResult(device_points=dev, loader=lambda: (xyz.copy(), rgb.copy(), err.copy()), points_per_reference=np.array([xyz.shape[0]]))
    monkeypatch.setattr(densify, "run_dense_pipeline", fake_run)
    out = os.path.join(str(tmp_path), "gui", "refused.ply")
    msgs = []
    with np.errstate(all="ignore"):
        code, _ = _gui_run(nodes, table, out, "sampled", msgs, voxel_size=vs, max_points=0)
        assert code == 0
        xv, cv = densify._voxel_downsample(xyz, rgb, vs)
    ref = os.path.join(str(tmp_path), "ref.ply")
    writers.write_ply(ref, xv, to_uint8_rgb(cv))
    assert open(out, "rb").read() == open(ref, "rb").read()
    assert [m for m in msgs if m[0] == 93.0] == [(93.0, "Applying distance filter...")]
