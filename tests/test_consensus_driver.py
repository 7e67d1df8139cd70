"""The cross-reference consensus filter in the driver, on the host backend with the analytic matcher (core/types.py, densify.py): the knobs and
their refusals, the CLI flags, and - through both entry points, in sampled and in dense mode - the file of a knob-on run: the cloud the pipeline
returned (the knob-off cloud) under the mask of the brute-force reference / the twin, same order, same bits, in front of the point cap and the
voxel filter and behind the per-reference filters."""
import logging
import os

import numpy as np
import pytest
import torch

import consensus_ref as cr
import cycle_scene
import lichtfeld_densification_plugin_amd as lfd
from lichtfeld_densification_plugin_amd import densify, synthetic
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from lichtfeld_densification_plugin_amd.core import writers
from lichtfeld_densification_plugin_amd.core.image_io import to_uint8_rgb
from lichtfeld_densification_plugin_amd.core.types import EXPERIMENTAL_DEFAULTS

RADIUS = {"sampled": 0.02, "dense": 0.005}          # a few sample spacings of the 4-camera scene: part of the cloud goes, part stays


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    return cycle_scene.make_scene(str(tmp_path_factory.mktemp("consensus_scene")), n_cams=4)


class Node:
    def __init__(self, cam):
        self.has_camera, self.camera_uid = True, cam.uid
        self.camera_width, self.camera_height = cam.width, cam.height
        self.camera_focal_x, self.camera_focal_y = float(cam.K[0, 0]), float(cam.K[1, 1])
        self.camera_R, self.camera_T = cam.R, cam.t.reshape(3)
        self.image_path, self.has_mask, self.mask_path = cam.image_path, False, None


class Spy:
    """keeps what run_dense_pipeline returned: the cloud the consensus filter is handed"""

    def __init__(self, monkeypatch):
        self.results = []
        plain = densify.run_dense_pipeline

        def run(*a, **kw):
            res = plain(*a, **kw)
            self.results.append((res.xyz.copy(), res.rgb.copy(), res.err.copy(), np.asarray(res.points_per_reference).copy()))
            return res
        monkeypatch.setattr(densify, "run_dense_pipeline", run)


def gui_run(scene, out, mode, exp, msgs=None, backend="host", device=None, matcher_kw=None, **cfg_kw):
    nodes = [Node(c) for c in scene["cams"]]
    recs = densify.extract_cameras_from_lfs(nodes)
    matcher = synthetic.SyntheticMatcher(recs, setting="turbo", device=device or "cpu", channels=2, **(matcher_kw or {}))
    cfg = lfd.DensePipelineConfig(output_path=out, num_refs=0.75, nns_per_ref=3, seed=3, viz_interval=0, matches_per_ref=2500, pack_workers=1,
                                  backend=backend, triangulation_mode=mode, experimental=exp, **cfg_kw)
    kw = {"device": device} if device is not None else {}
    return densify.dense_init_from_lfs(nodes, cfg, progress_callback=(lambda p, m: msgs.append((p, m))) if msgs is not None else None,
                                       matcher=matcher, **kw)


def cli_run(scene, out_name, mode, extra, msgs=None):
    args = densify.build_argparser().parse_args(["--scene_root", scene["root"], "--images_subdir", "images_4", "--num_refs", "0.75", "--nns_per_ref", "3",
                                                 "--matches_per_ref", "2500", "--seed", "3", "--pack_workers", "1", "--backend", "host",
                                                 "--triangulation_mode", mode, "--out_name", out_name] + extra)
    matcher = synthetic.SyntheticMatcher(scene["cams"], setting="turbo", device="cpu", channels=2)
    rc = densify.dense_init(args, progress_callback=(lambda p, m: msgs.append((p, m))) if msgs is not None else None, matcher=matcher)
    return rc, os.path.join(scene["root"], "sparse", "0", out_name)


def expected_mask(cloud, radius, min_refs, brute):
    xyz, _rgb, _err, counts = cloud
    twin = hb.HostDensifier(4)
    try:
        cons = twin.consensus_filter(torch.from_numpy(xyz), None, None, counts, radius, min_refs, True)[4].numpy()
    finally:
        twin.close()
    if brute:                                        # (the sampled cloud is small enough for every pair)
        assert np.array_equal(cons, cr.consensus(xyz, counts, radius))
    return cons >= min_refs


def written(path, xyz, rgb, err):
    densify._write_output(path, xyz, rgb, err, None)
    return open(path, "rb").read()


def test_the_knobs_are_experimental_off_by_default_and_validated():
    assert EXPERIMENTAL_DEFAULTS["min_consensus_refs"] == 0 and EXPERIMENTAL_DEFAULTS["consensus_radius"] == 0.0
    cfg = lfd.DensePipelineConfig(output_path="a.ply")
    assert cfg.exp("min_consensus_refs") == 0 and cfg.exp("consensus_radius") == 0.0
    on = {"min_consensus_refs": 2, "consensus_radius": 0.05}
    for mode in ("sampled", "dense"):
        for backend in ("device", "host"):
            assert lfd.DensePipelineConfig(output_path="a.ply", triangulation_mode=mode, backend=backend, experimental=on).problem() is None
    assert lfd.DensePipelineConfig(output_path="a.bin", max_points=10, voxel_size=0.1, experimental={**on, "min_consensus_refs": 8}).problem() is None
    assert lfd.DensePipelineConfig(output_path="a.ply", experimental={**on, "min_consensus_refs": np.int64(1)}).problem() is None
    refused = [
        (dict(), {"min_consensus_refs": -1, "consensus_radius": 0.05}, r"min_consensus_refs'\] must be a non-negative integer"),
        (dict(), {"min_consensus_refs": 1.5, "consensus_radius": 0.05}, r"min_consensus_refs'\] must be a non-negative integer"),
        (dict(), {"min_consensus_refs": True, "consensus_radius": 0.05}, r"min_consensus_refs'\] must be a non-negative integer"),
        (dict(), {"min_consensus_refs": "two"}, r"min_consensus_refs'\] must be a non-negative integer"),
        (dict(), {"min_consensus_refs": 9, "consensus_radius": 0.05}, r"min_consensus_refs'\] = 9 is more than the 8 references"),
        (dict(), {**on, "consensus_radius": -0.1}, r"consensus_radius'\] must be finite and >= 0"),
        (dict(), {**on, "consensus_radius": float("inf")}, r"consensus_radius'\] must be finite and >= 0"),
        (dict(), {**on, "consensus_radius": float("nan")}, r"consensus_radius'\] must be finite and >= 0"),
        (dict(), {**on, "consensus_radius": "wide"}, r"consensus_radius'\] must be a number"),
        (dict(), {**on, "consensus_radius": None}, r"consensus_radius'\] must be a number"),
        (dict(), {"min_consensus_refs": 2}, r"min_consensus_refs'\] needs a distance"),
        (dict(), {"min_consensus_refs": 2, "consensus_radius": 0.0}, r"min_consensus_refs'\] needs a distance"),
        (dict(), {"consensus_radius": 0.05}, r"consensus_radius'\] is the distance of the consensus filter"),
        (dict(), {"min_consensus_refs": 0, "consensus_radius": 0.05}, r"consensus_radius'\] is the distance of the consensus filter"),
        (dict(stream_output=True), on, r"min_consensus_refs'\] has to see the whole cloud"),
        (dict(triangulation_mode="dense", stream_output=True), on, r"min_consensus_refs'\] has to see the whole cloud"),
        (dict(), {**on, "exchange_records": "ply"}, r"min_consensus_refs'\] filters f32 rows"),
        (dict(triangulation_mode="dense"), {**on, "dense_tile_segments": True}, r"min_consensus_refs'\] needs the cloud as arrays"),
    ]
    for kw, exp, text in refused:
        with pytest.raises(ValueError, match=text):
            lfd.DensePipelineConfig(output_path="a.ply", experimental=exp, **kw)
    # switched off, none of the routes is refused
    for kw, exp in ((dict(stream_output=True), {}), (dict(triangulation_mode="dense"), {"dense_tile_segments": True})):
        assert lfd.DensePipelineConfig(output_path="a.ply", experimental={**exp, "min_consensus_refs": 0}, **kw).problem() is None


def test_the_cli_flags_reach_the_configuration():
    ap = densify.build_argparser()
    args = ap.parse_args(["--scene_root", "x", "--min_consensus_refs", "2", "--consensus_radius", "0.05"])
    assert (args.min_consensus_refs, args.consensus_radius) == (2, 0.05)
    assert densify._experimental_from_args(args) == {"min_consensus_refs": 2, "consensus_radius": 0.05}
    off = ap.parse_args(["--scene_root", "x"])
    assert (off.min_consensus_refs, off.consensus_radius) == (0, 0.0) and densify._experimental_from_args(off) == {}
    cfg = lfd.DensePipelineConfig(output_path="a.ply", experimental=densify._experimental_from_args(args))
    assert cfg.exp("min_consensus_refs") == 2 and cfg.exp("consensus_radius") == 0.05
    with pytest.raises(ValueError, match="needs a distance"):
        lfd.DensePipelineConfig(output_path="a.ply", experimental=densify._experimental_from_args(ap.parse_args(["--scene_root", "x", "--min_consensus_refs", "1"])))


@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_the_gui_entry_point_writes_the_knob_off_cloud_under_the_mask(scene, tmp_path, monkeypatch, caplog, mode):
    spy = Spy(monkeypatch)

    def never(*a, **kw):
        raise AssertionError("the filter ran with the knob off")
    off_out, on_out = os.path.join(str(tmp_path), "off.ply"), os.path.join(str(tmp_path), "on.ply")
    with monkeypatch.context() as m:
        m.setattr(hb.HostDensifier, "consensus_filter", never)
        off_msgs = []
        assert gui_run(scene, off_out, mode, {}, off_msgs) == (0, off_out)
    m_refs = 1 if mode == "sampled" else 2
    msgs = []
    with caplog.at_level(logging.INFO, logger="lfd_densify"):
        assert gui_run(scene, on_out, mode, {"min_consensus_refs": m_refs, "consensus_radius": RADIUS[mode]}, msgs) == (0, on_out)
    off_cloud, on_cloud = spy.results
    for a, b in zip(off_cloud, on_cloud):                                  # what the pipeline returns does not know the knob
        assert np.array_equal(a, b)
    xyz, rgb, err, counts = on_cloud
    assert open(off_out, "rb").read() == written(os.path.join(str(tmp_path), "off_ref.ply"), xyz, rgb, err)
    keep = expected_mask(on_cloud, RADIUS[mode], m_refs, brute=(mode == "sampled"))
    n, k = xyz.shape[0], int(keep.sum())
    print(f"{mode}: {n} points, {k} kept at radius {RADIUS[mode]} with {m_refs} other reference(s)")
    assert 0.05 * n < k < 0.95 * n                                         # both happen: the comparison below can fail
    assert open(on_out, "rb").read() == written(os.path.join(str(tmp_path), "on_ref.ply"), xyz[keep], rgb[keep], err[keep])
    assert (92.0, "Applying consensus filter...") in msgs and (92.0, "Applying consensus filter...") not in off_msgs
    assert [p for p, _m in msgs if p != 92.0] == [p for p, _m in off_msgs]
    lines = [r.getMessage() for r in caplog.records if r.getMessage().startswith("Consensus filter")]
    assert lines == [f"Consensus filter (radius {RADIUS[mode]:.4f}, {m_refs} other reference{'s' if m_refs != 1 else ''}): {n:,} points in, {k:,} kept"]


@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_the_cli_entry_point_writes_the_knob_off_cloud_under_the_mask(scene, tmp_path, monkeypatch, mode):
    spy = Spy(monkeypatch)
    rc, off_path = cli_run(scene, f"off_{mode}.ply", mode, [])
    assert rc == 0
    msgs = []
    rc, on_path = cli_run(scene, f"on_{mode}.ply", mode, ["--min_consensus_refs", "1", "--consensus_radius", str(RADIUS[mode])], msgs)
    assert rc == 0 and (92.0, "Applying consensus filter...") in msgs
    off_cloud, on_cloud = spy.results
    for a, b in zip(off_cloud, on_cloud):
        assert np.array_equal(a, b)
    xyz, rgb, err, _counts = on_cloud
    assert open(off_path, "rb").read() == written(os.path.join(str(tmp_path), "off_ref.ply"), xyz, rgb, err)
    keep = expected_mask(on_cloud, RADIUS[mode], 1, brute=False)
    assert 0.05 * xyz.shape[0] < keep.sum() < 0.95 * xyz.shape[0]
    assert open(on_path, "rb").read() == written(os.path.join(str(tmp_path), "on_ref.ply"), xyz[keep], rgb[keep], err[keep])
    # a points3D.bin keeps the reprojection errors of the kept points
    rc, bin_path = cli_run(scene, f"on_{mode}.bin", mode, ["--min_consensus_refs", "1", "--consensus_radius", str(RADIUS[mode]), "--max_points", "900"])
    cx, cc, ce = densify._apply_point_cap(xyz[keep], rgb[keep], err[keep], 900, 3)
    assert rc == 0 and cx.shape[0] == 900
    assert open(bin_path, "rb").read() == written(os.path.join(str(tmp_path), "on_ref.bin"), cx, cc, ce)


def test_consensus_first_then_the_cap_then_the_voxel_filter(scene, tmp_path, monkeypatch):
    spy = Spy(monkeypatch)
    out = os.path.join(str(tmp_path), "capped.ply")
    exp = {"min_consensus_refs": 1, "consensus_radius": RADIUS["sampled"]}
    msgs = []
    assert gui_run(scene, out, "sampled", exp, msgs, max_points=1500, voxel_size=0.03) == (0, out)
    xyz, rgb, err, _counts = spy.results[0]
    keep = expected_mask(spy.results[0], RADIUS["sampled"], 1, brute=False)
    assert keep.sum() > 1500
    cx, cc, _ce = densify._apply_point_cap(xyz[keep], rgb[keep], err[keep], 1500, 3)
    vx, vc = densify._voxel_downsample(cx, cc, 0.03)
    ref = os.path.join(str(tmp_path), "capped_ref.ply")
    writers.write_ply(ref, vx, to_uint8_rgb(vc))
    assert 0 < vx.shape[0] < 1500 and open(out, "rb").read() == open(ref, "rb").read()
    steps = [m for _p, m in msgs if m.startswith("Applying")]
    assert steps == ["Applying consensus filter...", "Applying distance filter..."]


def test_behind_the_support_filter_and_the_depth_gate(scene, tmp_path, monkeypatch):
    spy = Spy(monkeypatch)
    out = os.path.join(str(tmp_path), "chain.ply")
    front = {"min_support_views": 1, "max_depth_sigma_rel": 0.02, "match_sigma_px": 0.5}
    plain = cycle_scene.run(scene, cycle_scene.matcher_for(scene), "plain.ply", triangulation_mode="dense")
    assert gui_run(scene, out, "dense", {**front, "min_consensus_refs": 1, "consensus_radius": RADIUS["dense"]}) == (0, out)
    xyz, rgb, err, counts = spy.results[0]
    assert 0 < xyz.shape[0] < plain.xyz.shape[0]                           # the per-reference filters ran first: the filter is handed their survivors
    keep = expected_mask(spy.results[0], RADIUS["dense"], 1, brute=False)
    assert 0 < keep.sum() < xyz.shape[0]
    assert open(out, "rb").read() == written(os.path.join(str(tmp_path), "chain_ref.ply"), xyz[keep], rgb[keep], err[keep])


def test_a_cloud_too_wide_for_the_radius_names_the_knob(scene, tmp_path):
    exp = {"min_consensus_refs": 1, "consensus_radius": 1e-12}
    code, msg = gui_run(scene, os.path.join(str(tmp_path), "refused.ply"), "sampled", exp)
    assert code == 1 and "consensus_radius" in msg and "key range" in msg
    with pytest.raises(RuntimeError, match="consensus_radius.*key range"):
        cli_run(scene, "refused.ply", "sampled", ["--min_consensus_refs", "1", "--consensus_radius", "1e-12"])
