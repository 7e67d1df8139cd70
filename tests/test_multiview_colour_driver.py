"""The multi-view colour in the driver, on the host backend with the analytic matcher (core/types.py, core/hotpath.py, core/pipeline.py,
densify.py): the knob and its refusals, the CLI flag, the log line, a knob-off file byte for byte, and - in sampled and in dense mode - the
file of a knob-on run: the knob-off file's positions, counts and order, with the colours tests/colour_ref.py gives for the knob-off points
from the run's own inputs; also behind the support filter and the re-triangulation and in front of the normals and the Gaussian file."""
import logging
import os

import numpy as np
import pytest
import torch

import colour_ref
import cycle_scene
import knn_ref as kr
import lichtfeld_densification_plugin_amd as lfd
from lichtfeld_densification_plugin_amd import densify, synthetic
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from lichtfeld_densification_plugin_amd.core import pipeline as pl
from lichtfeld_densification_plugin_amd.core.image_io import to_uint8_rgb
from lichtfeld_densification_plugin_amd.core.types import EXPERIMENTAL_DEFAULTS

REC15 = np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)])
REC27 = np.dtype([("xyz", "<f4", 3), ("normal", "<f4", 3), ("rgb", "u1", 3)])
MEAN, MEDIAN = {"multiview_colour": "mean"}, {"multiview_colour": "median"}


class Node:
    """A camera node as the GUI hands it to dense_init_from_lfs."""

    def __init__(self, cam):
        self.has_camera, self.camera_uid = True, cam.uid
        self.camera_width, self.camera_height = cam.width, cam.height
        self.camera_focal_x, self.camera_focal_y = float(cam.K[0, 0]), float(cam.K[1, 1])
        self.camera_R, self.camera_T = cam.R, cam.t.reshape(3)
        self.image_path, self.has_mask, self.mask_path = cam.image_path, False, None


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    return cycle_scene.make_scene(str(tmp_path_factory.mktemp("colour_scene")), n_cams=4)


def records(path, dtype=REC15):
    head, body = open(path, "rb").read().split(b"end_header\n", 1)
    rec = np.frombuffer(body, dtype=dtype)
    assert f"element vertex {rec.shape[0]}\n".encode() in head
    return rec


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Spy:
    """Every colour_multiview call of a run: the points that went in, what came out, and what tests/colour_ref.py says for the same points
    from the batch the call was given."""

    def __init__(self, monkeypatch, cams):
        self.calls = []
        plain = hb.HostDensifier.colour_multiview
        spy = self

        def colour(dens, batch, out, tau, mode, with_status=False, counters=None):
            assert isinstance(out, hb.TriangulationOutput)
            before = out.rgb.numpy().copy()
            res = plain(dens, batch, out, tau, mode, with_status=with_status, counters=counters)
            got = res[0] if with_status else res
            want, status = colour_ref.batch_reference(cams, batch.refs, [[t.numpy() for t in r.nbr_images] for r in batch.refs], int(batch.c.w_match),
                                                      int(batch.c.h_match), out, tau, mode)
            spy.calls.append(dict(xyz=got.xyz.numpy().copy(), before=before, rgb=got.rgb.numpy().copy(), want=want, status=status, tau=tau, mode=mode))
            return res
        monkeypatch.setattr(hb.HostDensifier, "colour_multiview", colour)


def gui_run(scene, out, mode, exp, **cfg_kw):
    nodes = [Node(c) for c in scene["cams"]]
    recs = densify.extract_cameras_from_lfs(nodes)
    matcher = synthetic.SyntheticMatcher(recs, setting="turbo", device="cpu", channels=2)
    cfg = lfd.DensePipelineConfig(output_path=out, num_refs=0.75, nns_per_ref=3, seed=3, viz_interval=0, matches_per_ref=2500, pack_workers=1,
                                  backend="host", triangulation_mode=mode, experimental=exp, **cfg_kw)
    return densify.dense_init_from_lfs(nodes, cfg, matcher=matcher), recs


def cli_run(scene, out_name, mode, extra):
    args = densify.build_argparser().parse_args(["--scene_root", scene["root"], "--images_subdir", "images_4", "--num_refs", "0.75", "--nns_per_ref", "3",
                                                 "--matches_per_ref", "2500", "--seed", "3", "--pack_workers", "1", "--backend", "host",
                                                 "--triangulation_mode", mode, "--out_name", out_name] + extra)
    matcher = synthetic.SyntheticMatcher(scene["cams"], setting="turbo", device="cpu", channels=2)
    return densify.dense_init(args, matcher=matcher), os.path.join(scene["root"], "sparse", "0", out_name)


def test_the_knob_is_experimental_off_by_default_and_validated():
    assert EXPERIMENTAL_DEFAULTS["multiview_colour"] == "off"
    cfg = lfd.DensePipelineConfig(output_path="a.bin")
    assert cfg.exp("multiview_colour") == "off" and cfg.problem() is None
    for mode in ("sampled", "dense"):
        for backend in ("device", "host"):
            for out in ("a.ply", "points3D.bin"):
                for exp in (MEAN, MEDIAN, {**MEAN, "min_support_views": 1}, {**MEDIAN, "support_thresh_px": 2.5},
                            {**MEAN, "min_support_views": 1, "multiview_refine": True, "max_depth_sigma_rel": 0.05, "match_sigma_px": 0.5},
                            {**MEAN, "min_consensus_refs": 1, "consensus_radius": 0.1}):
                    assert lfd.DensePipelineConfig(output_path=out, triangulation_mode=mode, backend=backend, max_points=10, voxel_size=0.01,
                                                   experimental=exp).problem() is None
    assert lfd.DensePipelineConfig(output_path="a.ply", experimental={**MEDIAN, "estimate_normals": True, "gaussian_init": True,
                                                                      "fuse_voxel_size": 0.05}).problem() is None
    refused = [
        (dict(), {"multiview_colour": "on"}, r"multiview_colour'\] must be 'off' .*, 'mean' or 'median'"),
        (dict(), {"multiview_colour": True}, r"multiview_colour'\] must be 'off'"),
        (dict(), {"multiview_colour": 1}, r"multiview_colour'\] must be 'off'"),
        (dict(), {"multiview_colour": None}, r"multiview_colour'\] must be 'off'"),
        (dict(stream_output=True), MEAN, r"multiview_colour'\] rewrites the colour of points held as arrays .* stream_output"),
        (dict(triangulation_mode="dense", stream_output=True), MEDIAN, r"multiview_colour'\] rewrites the colour of points held as arrays .* stream_output"),
        (dict(triangulation_mode="dense"), {**MEAN, "dense_tile_segments": True}, r"multiview_colour'\] needs the ordered dense result"),
        (dict(), {**MEAN, "exchange_records": "ply"}, r"multiview_colour'\] rewrites f32 rows; experimental\['exchange_records'\] must be 'f32'"),
        (dict(), {**MEAN, "exchange_records": "auto"}, r"multiview_colour'\] rewrites f32 rows"),
        (dict(reproj_thresh=0.0), MEAN, r"multiview_colour'\] takes the other neighbours by the support filter's test: .* must be > 0"),
    ]
    for kw, exp, text in refused:
        with pytest.raises(ValueError, match=text):
            lfd.DensePipelineConfig(**{"output_path": "a.ply", **kw}, experimental=exp)
    assert lfd.DensePipelineConfig(output_path="a.ply", reproj_thresh=0.0, experimental={**MEAN, "support_thresh_px": 1.5}).problem() is None
    for kw in (dict(stream_output=True), dict(reproj_thresh=0.0)):              # switched off, none of the routes is refused
        assert lfd.DensePipelineConfig(**{"output_path": "a.ply", **kw}, experimental={"multiview_colour": "off"}).problem() is None


def test_the_cli_flag_reaches_the_configuration():
    ap = densify.build_argparser()
    for mode in ("mean", "median"):
        assert densify._experimental_from_args(ap.parse_args(["--scene_root", "x", "--multiview_colour", mode])) == {"multiview_colour": mode}
    assert densify._experimental_from_args(ap.parse_args(["--scene_root", "x"])) == {}
    assert densify._experimental_from_args(ap.parse_args(["--scene_root", "x", "--multiview_colour", "off"])) == {}
    with pytest.raises(SystemExit):
        ap.parse_args(["--scene_root", "x", "--multiview_colour", "mode"])


def test_a_sharded_run_is_refused_when_it_starts(scene, monkeypatch):
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    monkeypatch.setattr(dist, "get_rank", lambda *a: 0)
    cfg = lfd.DensePipelineConfig(output_path=os.path.join(scene["root"], "sharded.ply"), nns_per_ref=3, backend="host", experimental=MEAN)
    with pytest.raises(ValueError, match="multiview_colour'\\] cannot run sharded"):
        pl.run_dense_pipeline(scene["cams"], scene["refs"], scene["nn"], cfg, matcher=cycle_scene.matcher_for(scene))


@pytest.mark.parametrize("mode,colour", [("sampled", "mean"), ("dense", "median")])
def test_knob_off_is_the_plain_file_and_knob_on_rewrites_the_colours_only(scene, tmp_path, monkeypatch, caplog, mode, colour):
    never_out, off_out, on_out = (os.path.join(str(tmp_path), n) for n in ("never.ply", "off.ply", "on.ply"))

    def never(*a, **kw):
        raise AssertionError("the colour stage ran with the knob off")
    with monkeypatch.context() as m:
        m.setattr(hb.HostDensifier, "colour_multiview", never)
        (rc, _), recs = gui_run(scene, never_out, mode, {})
        (rc2, _), _ = gui_run(scene, off_out, mode, {"multiview_colour": "off"})
        assert rc == 0 and rc2 == 0
    assert open(never_out, "rb").read() == open(off_out, "rb").read()
    spy = Spy(monkeypatch, recs)
    with caplog.at_level(logging.INFO):
        (rc, _), _ = gui_run(scene, on_out, mode, {"multiview_colour": colour})
    assert rc == 0 and spy.calls
    off, on = records(off_out), records(on_out)
    assert off.shape[0] > 500 and off["xyz"].tobytes() == on["xyz"].tobytes()             # the same points in the same order
    assert off["rgb"].tobytes() != on["rgb"].tobytes()
    for c in spy.calls:
        assert c["mode"] == colour and c["tau"] == 1.6                                    # support_threshold(): 2 * reproj_thresh
        assert np.array_equal(bits(c["rgb"]), bits(c["want"]))
    used = [c for c in spy.calls if c["xyz"].shape[0]]
    assert np.array_equal(bits(np.concatenate([c["xyz"] for c in used])), bits(on["xyz"]))
    assert np.array_equal(to_uint8_rgb(np.concatenate([c["before"] for c in used])), off["rgb"])       # what went in is the knob-off colour
    assert np.array_equal(to_uint8_rgb(np.concatenate([c["want"] for c in used])), on["rgb"])          # what is written is the reference's
    status = np.concatenate([c["status"] for c in used]).astype(np.int64)
    line = [r.getMessage() for r in caplog.records if r.getMessage().startswith("Multi-view colour:")]
    assert len(line) == 1
    assert f"{colour} over the confirming views" in line[0] and f"{int((status > 0).sum())} points blended" in line[0]
    assert f"{status.sum() / (status > 0).sum():.2f} views per point" in line[0]
    assert status.max() == 4 and status.mean() > 2.5
    # the CLI entry point: the flag gives the same kind of file
    rc, cli_off = cli_run(scene, f"cli_off_{mode}.ply", mode, [])
    spy = Spy(monkeypatch, scene["cams"])                                                 # (the scene's own records: what the CLI plans with)
    rc2, cli_on = cli_run(scene, f"cli_on_{mode}.ply", mode, ["--multiview_colour", colour])
    assert rc == 0 and rc2 == 0
    c_off, c_on = records(cli_off), records(cli_on)
    assert c_off["xyz"].tobytes() == c_on["xyz"].tobytes() and c_off["rgb"].tobytes() != c_on["rgb"].tobytes()
    used = [c for c in spy.calls if c["xyz"].shape[0]]
    assert np.array_equal(to_uint8_rgb(np.concatenate([c["want"] for c in used])), c_on["rgb"])


def test_points3d_bin_takes_the_new_colour(scene, monkeypatch):
    rc, off_path = cli_run(scene, "off_points3D.bin", "sampled", [])
    spy = Spy(monkeypatch, scene["cams"])
    rc2, on_path = cli_run(scene, "on_points3D.bin", "sampled", ["--multiview_colour", "mean"])
    assert rc == 0 and rc2 == 0
    rec = np.dtype([("id", "<u8"), ("xyz", "<f8", 3), ("rgb", "u1", 3), ("err", "<f8")])             # upstream's 43-byte record behind the u64 count
    off, on = (np.frombuffer(open(p, "rb").read()[8:], dtype=rec) for p in (off_path, on_path))
    assert off.shape[0] > 500 and off["xyz"].tobytes() == on["xyz"].tobytes() and off["err"].tobytes() == on["err"].tobytes()
    used = [c for c in spy.calls if c["xyz"].shape[0]]
    assert np.array_equal(to_uint8_rgb(np.concatenate([c["want"] for c in used])), on["rgb"]) and off["rgb"].tobytes() != on["rgb"].tobytes()


@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_the_stage_composes_with_the_stages_around_it(scene, tmp_path, monkeypatch, mode):
    """Behind the support filter and the re-triangulation (it colours the points they leave, where they leave them), in front of the normals
    and the Gaussian file (f_dc is the new colour)."""
    around = {"min_support_views": 1, "multiview_refine": True, "estimate_normals": True, "normal_radius_cells": 2}
    off_out, on_out, g_out = (os.path.join(str(tmp_path), n) for n in ("off.ply", "on.ply", "gauss.ply"))
    (rc, _), recs = gui_run(scene, off_out, mode, around)
    spy = Spy(monkeypatch, recs)
    (rc2, _), _ = gui_run(scene, on_out, mode, {**around, **MEDIAN})
    assert rc == 0 and rc2 == 0
    off, on = records(off_out, REC27), records(on_out, REC27)
    assert off.shape[0] > 300 and off["xyz"].tobytes() == on["xyz"].tobytes() and off["normal"].tobytes() == on["normal"].tobytes()
    used = [c for c in spy.calls if c["xyz"].shape[0]]
    assert np.array_equal(bits(np.concatenate([c["xyz"] for c in used])), bits(on["xyz"]))              # the refined, filtered points
    for c in spy.calls:
        assert np.array_equal(bits(c["rgb"]), bits(c["want"]))
    assert np.array_equal(to_uint8_rgb(np.concatenate([c["want"] for c in used])), on["rgb"]) and off["rgb"].tobytes() != on["rgb"].tobytes()
    (rc3, _), _ = gui_run(scene, g_out, mode, {**around, **MEDIAN, "gaussian_init": True})
    assert rc3 == 0
    gauss = np.frombuffer(open(g_out, "rb").read().split(b"end_header\n", 1)[1], dtype=kr.REC68)
    assert gauss["xyz"].tobytes() == on["xyz"].tobytes()
    assert gauss["f_dc"].tobytes() == kr.dc_of_u8(on["rgb"]).tobytes()
