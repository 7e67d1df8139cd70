"""The free-space filter in the driver, on the host backend with the analytic matcher (core/types.py, densify.py): the knobs and their refusals,
the CLI flags, the switch next to every option of the configuration matrix, and - through both entry points, in sampled and in dense mode - the
file of a knob-on run: the cloud the pipeline returned (the knob-off cloud) under the mask of the NumPy reference, same order, same bits, behind
the consensus filter and in front of the point cap and the voxel filter."""
import logging
import math
import os
import re

import numpy as np
import pytest
import torch

import consensus_ref as cr
import cycle_scene
import freespace_ref as fr
import lichtfeld_densification_plugin_amd as lfd
from lichtfeld_densification_plugin_amd import densify, synthetic
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from lichtfeld_densification_plugin_amd.core import writers
from lichtfeld_densification_plugin_amd.core.image_io import to_uint8_rgb
from lichtfeld_densification_plugin_amd.core.types import EXPERIMENTAL_DEFAULTS
from test_config_matrix import OPTIONS

TOL = 0.002         # tighter than the matcher's depth noise on this scene: part of the cloud goes, part stays
ON = {"min_freespace_violations": 1, "freespace_depth_tol_rel": TOL}
STEP = (93.0, "Applying free-space filter...")


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    return cycle_scene.make_scene(str(tmp_path_factory.mktemp("freespace_scene")), n_cams=4)


class Node:
    def __init__(self, cam):
        self.has_camera, self.camera_uid = True, cam.uid
        self.camera_width, self.camera_height = cam.width, cam.height
        self.camera_focal_x, self.camera_focal_y = float(cam.K[0, 0]), float(cam.K[1, 1])
        self.camera_R, self.camera_T = cam.R, cam.t.reshape(3)
        self.image_path, self.has_mask, self.mask_path = cam.image_path, False, None


class Spy:
    """keeps what run_dense_pipeline was given and returned - the cloud the filters are handed - and what the free-space stage made of it"""

    def __init__(self, monkeypatch):
        self.results, self.stages = [], []
        plain, stage = densify.run_dense_pipeline, densify._apply_freespace_filter

        def run(records, refs_local, *a, **kw):
            res = plain(records, refs_local, *a, **kw)
            self.results.append(dict(xyz=res.xyz.copy(), rgb=res.rgb.copy(), err=res.err.copy(), counts=np.asarray(res.points_per_reference).copy(),
                                     cams=fr.cameras(records, [int(r) for r in refs_local]), grid=res.match_grid,
                                     normals=None if res.device_normals is None else res.normals.copy()))
            return res

        def filt(result, *a, **kw):
            before = (result.xyz.copy(), np.asarray(result.points_per_reference).copy())
            out = stage(result, *a, **kw)
            self.stages.append((before, (out.xyz.copy(), out.rgb.copy(), out.err.copy(), np.asarray(out.points_per_reference).copy())))
            return out
        monkeypatch.setattr(densify, "run_dense_pipeline", run)
        monkeypatch.setattr(densify, "_apply_freespace_filter", filt)


def gui_run(scene, out, mode, exp, msgs=None, backend="host", device=None, matcher_kw=None, **cfg_kw):
    nodes = [Node(c) for c in scene["cams"]]
    recs = densify.extract_cameras_from_lfs(nodes)
    matcher = synthetic.SyntheticMatcher(recs, setting="turbo", device=device or "cpu", channels=2, **(matcher_kw or {}))
    kw = dict(num_refs=0.75, nns_per_ref=3, seed=3, viz_interval=0, matches_per_ref=2500, pack_workers=1)
    kw.update(cfg_kw)
    if not kw.get("share_features", True):                                # without feature keys the stand-in recognises the images it is handed
        from lichtfeld_densification_plugin_amd.core.image_io import load_rgb_u8
        for i, r in enumerate(recs):
            matcher.register_image(i, load_rgb_u8(r.image_path, (matcher.w_resized, matcher.h_resized)))
    cfg = lfd.DensePipelineConfig(output_path=out, backend=backend, triangulation_mode=mode, experimental=exp, **kw)
    dkw = {"device": device} if device is not None else {}
    return densify.dense_init_from_lfs(nodes, cfg, progress_callback=(lambda p, m: msgs.append((p, m))) if msgs is not None else None,
                                       matcher=matcher, **dkw)


def cli_run(scene, out_name, mode, extra, msgs=None):
    args = densify.build_argparser().parse_args(["--scene_root", scene["root"], "--images_subdir", "images_4", "--num_refs", "0.75", "--nns_per_ref", "3",
                                                 "--matches_per_ref", "2500", "--seed", "3", "--pack_workers", "1", "--backend", "host",
                                                 "--triangulation_mode", mode, "--out_name", out_name] + extra)
    matcher = synthetic.SyntheticMatcher(scene["cams"], setting="turbo", device="cpu", channels=2)
    rc = densify.dense_init(args, progress_callback=(lambda p, m: msgs.append((p, m))) if msgs is not None else None, matcher=matcher)
    return rc, os.path.join(scene["root"], "sparse", "0", out_name)


def auto_plane(cloud, mode, matches_per_ref=2500):
    w, h = (int(v) for v in cloud["cams"][1][0])
    cells = max(cloud["grid"]) if mode == "dense" else math.ceil(math.sqrt(matches_per_ref))
    return fr.plane_size(cells, w, h)


def expected_mask(cloud, plane, tol, min_v, xyz=None, counts=None):
    xyz = cloud["xyz"] if xyz is None else xyz
    counts = cloud["counts"] if counts is None else counts
    P, wh = cloud["cams"]
    viol, supp = fr.counts_of(xyz, counts, P, wh, plane[0], plane[1], tol)
    return fr.keep_mask(viol, supp, min_v)


def written(path, xyz, rgb, err):
    densify._write_output(path, xyz, rgb, err, None)
    return open(path, "rb").read()


def test_the_knobs_are_experimental_off_by_default_and_validated():
    assert EXPERIMENTAL_DEFAULTS["min_freespace_violations"] == 0 and EXPERIMENTAL_DEFAULTS["freespace_depth_tol_rel"] == 0.02
    assert EXPERIMENTAL_DEFAULTS["freespace_plane_cells"] == 0
    cfg = lfd.DensePipelineConfig(output_path="a.ply")
    assert cfg.exp("min_freespace_violations") == 0 and cfg.exp("freespace_depth_tol_rel") == 0.02 and cfg.exp("freespace_plane_cells") == 0
    on = {"min_freespace_violations": 2}
    for mode in ("sampled", "dense"):
        for backend in ("device", "host"):
            assert lfd.DensePipelineConfig(output_path="a.ply", triangulation_mode=mode, backend=backend, experimental=on).problem() is None
    assert lfd.DensePipelineConfig(output_path="a.bin", max_points=10, voxel_size=0.1, experimental={"min_freespace_violations": 255}).problem() is None
    assert lfd.DensePipelineConfig(output_path="a.ply", experimental={"min_freespace_violations": np.int64(1), "freespace_depth_tol_rel": 0.1,
                                                                      "freespace_plane_cells": 4096}).problem() is None
    assert lfd.DensePipelineConfig(output_path="a.ply", experimental={**on, "freespace_plane_cells": 8}).problem() is None
    assert lfd.DensePipelineConfig(output_path="a.ply", experimental={"freespace_depth_tol_rel": 0.02}).problem() is None     # off, at its default
    refused = [
        (dict(), {"min_freespace_violations": -1}, r"min_freespace_violations'\] must be a non-negative integer"),
        (dict(), {"min_freespace_violations": 1.5}, r"min_freespace_violations'\] must be a non-negative integer"),
        (dict(), {"min_freespace_violations": True}, r"min_freespace_violations'\] must be a non-negative integer"),
        (dict(), {"min_freespace_violations": "two"}, r"min_freespace_violations'\] must be a non-negative integer"),
        (dict(), {"min_freespace_violations": 256}, r"min_freespace_violations'\] = 256 is more than the 255 references"),
        (dict(), {**on, "freespace_depth_tol_rel": 0.0}, r"freespace_depth_tol_rel'\] must be in \(0, 1\)"),
        (dict(), {**on, "freespace_depth_tol_rel": 1.0}, r"freespace_depth_tol_rel'\] must be in \(0, 1\)"),
        (dict(), {**on, "freespace_depth_tol_rel": -0.1}, r"freespace_depth_tol_rel'\] must be in \(0, 1\)"),
        (dict(), {**on, "freespace_depth_tol_rel": 1.0 - 1e-12}, r"freespace_depth_tol_rel'\] must be in \(0, 1\)"),       # 1 as an f32
        (dict(), {**on, "freespace_depth_tol_rel": float("nan")}, r"freespace_depth_tol_rel'\] must be in \(0, 1\)"),
        (dict(), {**on, "freespace_depth_tol_rel": "tight"}, r"freespace_depth_tol_rel'\] must be a number"),
        (dict(), {**on, "freespace_depth_tol_rel": None}, r"freespace_depth_tol_rel'\] must be a number"),
        (dict(), {"freespace_depth_tol_rel": 0.05}, r"freespace_depth_tol_rel'\] is the tolerance of the free-space filter"),
        (dict(), {**on, "freespace_plane_cells": 7}, r"freespace_plane_cells'\] must be 0 \(automatic\) or an integer in 8 .. 4096"),
        (dict(), {**on, "freespace_plane_cells": 4097}, r"freespace_plane_cells'\] must be 0 \(automatic\) or an integer in 8 .. 4096"),
        (dict(), {**on, "freespace_plane_cells": -8}, r"freespace_plane_cells'\] must be 0 \(automatic\) or an integer in 8 .. 4096"),
        (dict(), {**on, "freespace_plane_cells": 64.0}, r"freespace_plane_cells'\] must be 0 \(automatic\) or an integer in 8 .. 4096"),
        (dict(), {**on, "freespace_plane_cells": True}, r"freespace_plane_cells'\] must be 0 \(automatic\) or an integer in 8 .. 4096"),
        (dict(), {"freespace_plane_cells": 64}, r"freespace_plane_cells'\] is the z-buffer size of the free-space filter"),
        (dict(stream_output=True), on, r"min_freespace_violations'\] has to see the whole cloud"),
        (dict(triangulation_mode="dense", stream_output=True), on, r"min_freespace_violations'\] has to see the whole cloud"),
        (dict(), {**on, "exchange_records": "ply"}, r"min_freespace_violations'\] filters f32 rows"),
        (dict(triangulation_mode="dense"), {**on, "dense_tile_segments": True}, r"min_freespace_violations'\] needs the cloud as arrays"),
    ]
    for kw, exp, text in refused:
        with pytest.raises(ValueError, match=text):
            lfd.DensePipelineConfig(output_path="a.ply", experimental=exp, **kw)
    # switched off, none of the routes is refused
    for kw, exp in ((dict(stream_output=True), {}), (dict(triangulation_mode="dense"), {"dense_tile_segments": True})):
        assert lfd.DensePipelineConfig(output_path="a.ply", experimental={**exp, "min_freespace_violations": 0}, **kw).problem() is None


def test_the_cli_flags_reach_the_configuration():
    ap = densify.build_argparser()
    args = ap.parse_args(["--scene_root", "x", "--min_freespace_violations", "2", "--freespace_depth_tol_rel", "0.05", "--freespace_plane_cells", "128"])
    assert (args.min_freespace_violations, args.freespace_depth_tol_rel, args.freespace_plane_cells) == (2, 0.05, 128)
    assert densify._experimental_from_args(args) == {"min_freespace_violations": 2, "freespace_depth_tol_rel": 0.05, "freespace_plane_cells": 128}
    off = ap.parse_args(["--scene_root", "x"])
    assert (off.min_freespace_violations, off.freespace_depth_tol_rel, off.freespace_plane_cells) == (0, None, 0)
    assert densify._experimental_from_args(off) == {}
    cfg = lfd.DensePipelineConfig(output_path="a.ply", experimental=densify._experimental_from_args(args))
    assert cfg.exp("min_freespace_violations") == 2 and cfg.exp("freespace_depth_tol_rel") == 0.05 and cfg.exp("freespace_plane_cells") == 128
    only_on = densify._experimental_from_args(ap.parse_args(["--scene_root", "x", "--min_freespace_violations", "1"]))
    assert only_on == {"min_freespace_violations": 1} and lfd.DensePipelineConfig(output_path="a.ply", experimental=only_on).exp("freespace_depth_tol_rel") == 0.02
    for flags, text in ((["--freespace_depth_tol_rel", "0.05"], "tolerance of the free-space filter"), (["--freespace_plane_cells", "64"], "z-buffer size")):
        with pytest.raises(ValueError, match=text):
            lfd.DensePipelineConfig(output_path="a.ply", experimental=densify._experimental_from_args(ap.parse_args(["--scene_root", "x"] + flags)))


def test_the_plane_size():
    cfg = lambda mode, cells=0, m=9000: lfd.DensePipelineConfig(output_path="a.ply", triangulation_mode=mode, matches_per_ref=m,      # noqa: E731
                                                                experimental={"min_freespace_violations": 1, "freespace_plane_cells": cells})
    assert densify.freespace_plane(cfg("sampled"), 1297, 840) == (95, 62) == fr.plane_size(math.ceil(math.sqrt(9000)), 1297, 840)
    assert densify.freespace_plane(cfg("sampled"), 840, 1297) == (62, 95)
    assert densify.freespace_plane(cfg("sampled", m=2500), 64, 64) == (50, 50)
    assert densify.freespace_plane(cfg("dense"), 1297, 840, (560, 864)) == (864, 560) == fr.plane_size(864, 1297, 840)
    assert densify.freespace_plane(cfg("dense", 96), 1297, 840, (560, 864)) == (96, 62)
    assert densify.freespace_plane(cfg("sampled", 8), 4000, 10) == (8, 1)
    with pytest.raises(RuntimeError, match="matcher's grid"):
        densify.freespace_plane(cfg("dense"), 1297, 840, None)


LEGAL_ON_HOST, REFUSED = [], {"stream": "has to see the whole cloud", "x:ply_records": "filters f32 rows"}


@pytest.mark.parametrize("option", sorted(OPTIONS))
def test_the_switch_next_to_every_option_of_the_configuration_matrix(scene, tmp_path, monkeypatch, option):
    """a legal pair: the stage hands on the cloud it was given under the reference's mask; a refused pair: its message"""
    field, value = OPTIONS[option]
    mode = "dense" if option in ("dense", "x:segments") else "sampled"
    exp, kw = dict(ON), {}
    if option.startswith("x:"):
        exp[field] = value
    elif field != "triangulation_mode":
        kw[field] = value
    out = os.path.join(str(tmp_path), "pair.ply")
    make = lambda e, backend: lfd.DensePipelineConfig(output_path=out, backend=backend, triangulation_mode=mode, experimental=e, **kw)      # noqa: E731
    if option in REFUSED or option == "x:segments":
        text = REFUSED.get(option, "needs the cloud as arrays")
        with pytest.raises(ValueError, match=r"min_freespace_violations'\] " + text):
            make(exp, "device")
        return
    try:
        make({k: v for k, v in exp.items() if k not in ON}, "host")
    except ValueError as exc:                                              # refused without the switch as well (a device-only option on the host
        with pytest.raises(ValueError, match=re.escape(str(exc))):         # backend, a form of another option): the same message with it
            make(exp, "host")
        return
    assert make(exp, "host").problem() is None
    spy = Spy(monkeypatch)
    assert gui_run(scene, out, mode, exp, **kw) == (0, out)
    (before, after), cloud = spy.stages[0], spy.results[0]
    assert np.array_equal(before[0], cloud["xyz"])                         # (no consensus filter in front here)
    keep = expected_mask(cloud, auto_plane(cloud, mode), TOL, 1)
    assert 0 < keep.sum() < len(keep)
    ids = fr.ref_ids(cloud["counts"])
    assert np.array_equal(after[0].view(np.uint32), cloud["xyz"][keep].view(np.uint32)) and np.array_equal(after[1].view(np.uint32), cloud["rgb"][keep].view(np.uint32))
    assert np.array_equal(after[2].view(np.uint32), cloud["err"][keep].view(np.uint32))
    assert np.array_equal(after[3], np.bincount(ids[keep], minlength=len(cloud["counts"])))


@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_the_gui_entry_point_writes_the_knob_off_cloud_under_the_mask(scene, tmp_path, monkeypatch, caplog, mode):
    spy = Spy(monkeypatch)

    def never(*a, **kw):
        raise AssertionError("the filter ran with the knob off")
    off_out, on_out = os.path.join(str(tmp_path), "off.ply"), os.path.join(str(tmp_path), "on.ply")
    with monkeypatch.context() as m:
        m.setattr(hb.HostDensifier, "freespace_filter", never)
        off_msgs = []
        assert gui_run(scene, off_out, mode, {}, off_msgs) == (0, off_out)
    msgs = []
    with caplog.at_level(logging.INFO, logger="lfd_densify"):
        assert gui_run(scene, on_out, mode, ON, msgs) == (0, on_out)
    off_cloud, on_cloud = spy.results
    for k in ("xyz", "rgb", "err", "counts"):                              # what the pipeline returns does not know the knob
        assert np.array_equal(off_cloud[k], on_cloud[k])
    xyz, rgb, err = on_cloud["xyz"], on_cloud["rgb"], on_cloud["err"]
    assert open(off_out, "rb").read() == written(os.path.join(str(tmp_path), "off_ref.ply"), xyz, rgb, err)
    plane = auto_plane(on_cloud, mode)
    assert max(plane) == (50 if mode == "sampled" else max(on_cloud["grid"])) and min(plane) >= 1      # ceil(sqrt(2500)); the matcher's grid
    keep = expected_mask(on_cloud, plane, TOL, 1)
    n, k = xyz.shape[0], int(keep.sum())
    print(f"{mode}: {n} points, {k} kept at tolerance {TOL} on planes of {plane}")
    assert 0.05 * n < k < 0.999 * n                                        # both happen: the comparison below can fail
    assert open(on_out, "rb").read() == written(os.path.join(str(tmp_path), "on_ref.ply"), xyz[keep], rgb[keep], err[keep])
    assert STEP in msgs and STEP not in off_msgs
    assert [p for p, _m in msgs if p != 93.0] == [p for p, _m in off_msgs]
    lines = [r.getMessage() for r in caplog.records if r.getMessage().startswith("Free-space filter")]
    assert lines == [f"Free-space filter (tolerance {TOL:g}, 1 refuting reference, planes of {plane[0]} x {plane[1]} cells): {n:,} points in, {k:,} kept"]
    # an explicit plane size is used as given
    small = os.path.join(str(tmp_path), "small.ply")
    assert gui_run(scene, small, mode, {**ON, "freespace_plane_cells": 16}) == (0, small)
    keep16 = expected_mask(on_cloud, fr.plane_size(16, *(int(v) for v in on_cloud["cams"][1][0])), TOL, 1)
    assert open(small, "rb").read() == written(os.path.join(str(tmp_path), "small_ref.ply"), xyz[keep16], rgb[keep16], err[keep16])


@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_the_cli_entry_point_writes_the_knob_off_cloud_under_the_mask(scene, tmp_path, monkeypatch, mode):
    spy = Spy(monkeypatch)
    rc, off_path = cli_run(scene, f"off_{mode}.ply", mode, [])
    assert rc == 0
    msgs = []
    flags = ["--min_freespace_violations", "1", "--freespace_depth_tol_rel", str(TOL)]
    rc, on_path = cli_run(scene, f"on_{mode}.ply", mode, flags, msgs)
    assert rc == 0 and STEP in msgs
    off_cloud, on_cloud = spy.results
    for k in ("xyz", "rgb", "err", "counts"):
        assert np.array_equal(off_cloud[k], on_cloud[k])
    xyz, rgb, err = on_cloud["xyz"], on_cloud["rgb"], on_cloud["err"]
    assert open(off_path, "rb").read() == written(os.path.join(str(tmp_path), "off_ref.ply"), xyz, rgb, err)
    keep = expected_mask(on_cloud, auto_plane(on_cloud, mode), TOL, 1)
    assert 0.05 * xyz.shape[0] < keep.sum() < 0.999 * xyz.shape[0]
    assert open(on_path, "rb").read() == written(os.path.join(str(tmp_path), "on_ref.ply"), xyz[keep], rgb[keep], err[keep])
    # a points3D.bin keeps the reprojection errors of the kept points
    rc, bin_path = cli_run(scene, f"on_{mode}.bin", mode, flags + ["--max_points", "900"])
    cx, cc, ce = densify._apply_point_cap(xyz[keep], rgb[keep], err[keep], 900, 3)
    assert rc == 0 and cx.shape[0] == 900
    assert open(bin_path, "rb").read() == written(os.path.join(str(tmp_path), "on_ref.bin"), cx, cc, ce)


def test_consensus_first_then_free_space_then_the_cap_then_the_voxel_filter(scene, tmp_path, monkeypatch):
    spy = Spy(monkeypatch)
    out = os.path.join(str(tmp_path), "capped.ply")
    radius = 0.02
    exp = {**ON, "min_consensus_refs": 1, "consensus_radius": radius}
    msgs = []
    assert gui_run(scene, out, "sampled", exp, msgs, max_points=1200, voxel_size=0.03) == (0, out)
    cloud = spy.results[0]
    xyz, rgb, err, counts = cloud["xyz"], cloud["rgb"], cloud["err"], cloud["counts"]
    agreed = cr.consensus(xyz, counts, radius) >= 1
    assert 0 < agreed.sum() < len(agreed)
    ids = fr.ref_ids(counts)
    counts2 = np.bincount(ids[agreed], minlength=len(counts))
    assert np.array_equal(spy.stages[0][0][0], xyz[agreed]) and np.array_equal(spy.stages[0][0][1], counts2)      # the stage is handed consensus' survivors
    keep = expected_mask(cloud, auto_plane(cloud, "sampled"), TOL, 1, xyz[agreed], counts2)
    assert 1200 < keep.sum() < agreed.sum()
    cx, cc, _ce = densify._apply_point_cap(xyz[agreed][keep], rgb[agreed][keep], err[agreed][keep], 1200, 3)
    vx, vc = densify._voxel_downsample(cx, cc, 0.03)
    ref = os.path.join(str(tmp_path), "capped_ref.ply")
    writers.write_ply(ref, vx, to_uint8_rgb(vc))
    assert 0 < vx.shape[0] < 1200 and open(out, "rb").read() == open(ref, "rb").read()
    steps = [m for _p, m in msgs if m.startswith("Applying")]
    assert steps == ["Applying consensus filter...", "Applying free-space filter...", "Applying distance filter..."]


def test_every_written_normal_is_the_one_its_point_had(scene, tmp_path, monkeypatch):
    spy = Spy(monkeypatch)
    out = os.path.join(str(tmp_path), "normals.ply")
    assert gui_run(scene, out, "dense", {**ON, "estimate_normals": True}) == (0, out)
    cloud = spy.results[0]
    assert cloud["normals"] is not None and cloud["normals"].shape == cloud["xyz"].shape
    keep = expected_mask(cloud, auto_plane(cloud, "dense"), TOL, 1)
    assert 0 < keep.sum() < len(keep)
    ref = os.path.join(str(tmp_path), "normals_ref.ply")
    writers.write_ply(ref, cloud["xyz"][keep], to_uint8_rgb(cloud["rgb"][keep]), cloud["normals"][keep])
    assert open(out, "rb").read() == open(ref, "rb").read()


def test_a_result_that_holds_a_shard_only_is_refused(scene):
    from lichtfeld_densification_plugin_amd.core.sinks import PipelineResult
    recs = densify.extract_cameras_from_lfs([Node(c) for c in scene["cams"]])
    cfg = lfd.DensePipelineConfig(output_path="a.ply", experimental=ON)
    z = np.zeros((10, 3), np.float32)
    shard = PipelineResult(xyz=z, rgb=z, err=np.zeros(10, np.float32), points_per_reference=np.array([10, 25, 7]))
    with pytest.raises(RuntimeError, match="needs the whole cloud with its per-reference counts"):
        densify._apply_freespace_filter(shard, cfg, recs, [0, 1, 2])
    with pytest.raises(RuntimeError, match="needs the whole cloud with its per-reference counts"):
        densify._apply_freespace_filter(PipelineResult(xyz=z, rgb=z, err=np.zeros(10, np.float32), points_per_reference=np.array([10])), cfg, recs, [0, 1, 2])
