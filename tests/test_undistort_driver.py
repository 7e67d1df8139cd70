"""experimental['undistort_images'] in the driver, on the host backend with the analytic matcher wrapped to record the images it is handed
(core/types.py, densify.py, core/pipeline.py, core/packing.py, core/image_io.py): the knob, its flag and its refusal; on a SIMPLE_RADIAL and an
OPENCV scene the matcher receives exactly the PIL resize of the reference-undistorted decode and the cameras' masks are what the reference says,
in sampled and dense mode, with and without mask files; with the knob off the run is the run of the same scene with pinhole cameras, byte for
byte, plus one warning; a fisheye scene is refused by name before anything is matched; the GUI entry point, whose nodes carry no distortion,
logs one line and writes the knob-off bytes."""
import logging
import os

import numpy as np
import pytest

import undistort_scene as us
import lichtfeld_densification_plugin_amd as lfd
from lichtfeld_densification_plugin_amd import densify
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from lichtfeld_densification_plugin_amd.core import pipeline as pl
from lichtfeld_densification_plugin_amd.core.types import EXPERIMENTAL_DEFAULTS, CameraRecord

SIZE = (320, 320)            # the "turbo" preset's match size


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    made = {}

    def get(model, masks=False):
        if (model, masks) not in made:
            made[(model, masks)] = us.make_scene(str(tmp_path_factory.mktemp(f"undistort_{model.lower()}_{int(masks)}")), model, masks=masks)
        return made[(model, masks)]
    return get


class PackSpy:
    """keeps every package the loader made: the host-prepared image and masks of the reference and its neighbours"""

    def __init__(self, monkeypatch):
        self.views = {}
        plain = pl.pack_reference

        def pack(*a, **kw):
            p = plain(*a, **kw)
            if p is not None:
                for cam, img, mask in zip([p.ref_index] + list(p.nbr_indices), [p.image] + list(p.nbr_images), [p.mask_a] + list(p.nbr_masks)):
                    self.views[int(cam)] = (np.array(img), None if mask is None else np.array(mask))
            return p
        monkeypatch.setattr(pl, "pack_reference", pack)


def run(scene, out_name, mode, on, matcher=None):
    cfg = lfd.DensePipelineConfig(output_path=os.path.join(scene["root"], out_name), nns_per_ref=3, seed=3, viz_interval=0, matches_per_ref=2500,
                                  pack_workers=2, backend="host", triangulation_mode=mode, experimental={"undistort_images": True} if on else {})
    matcher = matcher or us.matcher_for(scene)
    return pl.run_dense_pipeline(scene["cams"], scene["refs"], scene["nn"], cfg, matcher=matcher), matcher


def cli_run(scene, out_name, mode, extra, matcher=None):
    args = densify.build_argparser().parse_args(["--scene_root", scene["root"], "--images_subdir", "images_4", "--num_refs", "0.75", "--nns_per_ref", "3",
                                                 "--matches_per_ref", "2500", "--seed", "3", "--pack_workers", "1", "--backend", "host",
                                                 "--triangulation_mode", mode, "--out_name", out_name] + extra)
    matcher = matcher or us.matcher_for(scene)
    rc = densify.dense_init(args, matcher=matcher)
    return rc, os.path.join(scene["root"], "sparse", "0", out_name), matcher


def test_the_knob_is_experimental_off_by_default_and_validated():
    assert EXPERIMENTAL_DEFAULTS["undistort_images"] is False
    assert lfd.DensePipelineConfig(output_path="a.ply").exp("undistort_images") is False
    for mode in ("sampled", "dense"):
        for backend in ("device", "host"):
            for prep in (False, True):
                if prep and backend == "host":
                    continue
                cfg = lfd.DensePipelineConfig(output_path="a.ply", triangulation_mode=mode, backend=backend, device_image_prep=prep,
                                              experimental={"undistort_images": True})
                assert cfg.problem() is None
    assert lfd.DensePipelineConfig(output_path="a.ply", stream_output=True, experimental={"undistort_images": np.bool_(True)}).problem() is None
    for bad in (1, 0, "yes", None, 1.0):
        with pytest.raises(ValueError, match=r"undistort_images'\] must be True or False"):
            lfd.DensePipelineConfig(output_path="a.ply", experimental={"undistort_images": bad})


def test_the_cli_flag_reaches_the_configuration():
    ap = densify.build_argparser()
    on, off = ap.parse_args(["--scene_root", "x", "--undistort_images"]), ap.parse_args(["--scene_root", "x"])
    assert on.undistort_images is True and off.undistort_images is False
    assert densify._experimental_from_args(on) == {"undistort_images": True} and densify._experimental_from_args(off) == {}


def test_the_record_fields_and_the_model_table():
    rec = CameraRecord.from_krt(1, np.eye(3), np.eye(3), np.zeros(3), 10, 8)
    assert rec.distortion is None and rec.distortion_model is None and rec.active_distortion() is None

    class Cam:
        def __init__(self, name, params):
            self.model, self.params, self.width, self.height = type("M", (), {"name": name})(), np.asarray(params, np.float64), 10, 8
    f = densify.distortion_from_camera
    z = (0.0,) * 8
    assert f(Cam("SIMPLE_PINHOLE", [5, 1, 2])) == (5, 5, 1, 2) + z and f(Cam("PINHOLE", [5, 6, 1, 2])) == (5, 6, 1, 2) + z
    assert f(Cam("SIMPLE_RADIAL", [5, 1, 2, 0.1])) == (5, 5, 1, 2, 0.1) + z[1:]
    assert f(Cam("RADIAL", [5, 1, 2, 0.1, 0.2])) == (5, 5, 1, 2, 0.1, 0.2) + z[2:]
    assert f(Cam("OPENCV", [5, 6, 1, 2, 0.1, 0.2, 0.3, 0.4])) == (5, 6, 1, 2, 0.1, 0.2, 0.3, 0.4) + z[4:]
    full = [5, 6, 1, 2, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8]
    assert f(Cam("FULL_OPENCV", full)) == tuple(float(v) for v in full)
    third = 1.0 / 3.0                                                    # f64 as stored: not through the record's f32 K
    assert f(Cam("SIMPLE_RADIAL", [third, 1, 2, third]))[0] == third and float(np.float32(third)) != third
    for name, n in (("SIMPLE_RADIAL_FISHEYE", 4), ("RADIAL_FISHEYE", 5), ("OPENCV_FISHEYE", 8), ("THIN_PRISM_FISHEYE", 12), ("FOV", 5), ("DIVISION", 4)):
        assert f(Cam(name, [5.0] * n)) is None, name
    assert f(Cam("simple_radial", [5, 1, 2, 0.1])) == f(Cam("SIMPLE_RADIAL", [5, 1, 2, 0.1]))


def test_colmap_records_carry_the_parameters_and_synthetic_defaults_write_the_same_files(scenes, tmp_path):
    sr, cv = scenes("SIMPLE_RADIAL"), scenes("OPENCV")
    for rec in sr["cams"]:
        assert rec.distortion_model == "SIMPLE_RADIAL" and rec.distortion[4:] == (-1.5,) + (0.0,) * 7 and rec.distortion[0] == rec.distortion[1]
        assert rec.active_distortion() == rec.distortion and np.float32(rec.distortion[2]) == rec.K[0, 2]
    for rec in cv["cams"]:
        assert rec.distortion_model == "OPENCV" and rec.distortion[4:] == (2.0, -3.0, 0.02, -0.015, 0.0, 0.0, 0.0, 0.0)
    ph = scenes("PINHOLE")
    assert all(r.distortion_model == "PINHOLE" and r.distortion is not None and r.active_distortion() is None for r in ph["cams"])
    # camera_model / distortion left at their defaults: the files of a call without them
    from lichtfeld_densification_plugin_amd import synthetic
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    synthetic.write_colmap_scene(a, n_cams=3, width=64, height=48, fmt="png")
    synthetic.write_colmap_scene(b, n_cams=3, width=64, height=48, fmt="png", camera_model="PINHOLE", distortion=())
    for name in ("cameras.bin", "images.bin", "points3D.bin"):
        assert open(os.path.join(a, "sparse", "0", name), "rb").read() == open(os.path.join(b, "sparse", "0", name), "rb").read()
    with pytest.raises(ValueError, match="SIMPLE_RADIAL stores 4 parameters"):
        synthetic.write_colmap_scene(str(tmp_path / "c"), n_cams=2, width=64, height=48, fmt="png", camera_model="SIMPLE_RADIAL", distortion=(0.1, 0.2, 0.3))


@pytest.mark.parametrize("masks", [False, True], ids=["no_masks", "mask_files"])
@pytest.mark.parametrize("mode", ["sampled", "dense"])
@pytest.mark.parametrize("model", ["SIMPLE_RADIAL", "OPENCV"])
def test_the_matcher_receives_the_undistorted_images_and_the_masks_are_the_references(scenes, monkeypatch, model, mode, masks):
    scene = scenes(model, masks)
    spy = PackSpy(monkeypatch)
    res, matcher = run(scene, f"on_{mode}.ply", mode, True)
    assert res.xyz.shape[0] > 0 and len(matcher.seen) == len(scene["cams"])
    n_masked = 0
    for cam_index, seen in matcher.seen.items():
        img, mask = us.expected_view(scene["cams"][cam_index], SIZE, undistort=True)
        plain, _ = us.expected_view(scene["cams"][cam_index], SIZE, undistort=False)
        assert np.array_equal(seen, img)
        assert not np.array_equal(seen, plain)                          # (the comparison above can fail: undistorting changes the image)
        got_img, got_mask = spy.views[cam_index]
        assert np.array_equal(got_img, img)
        assert (got_mask is None) == (mask is None) and (mask is None or np.array_equal(got_mask, mask))
        n_masked += mask is not None
    # the barrel camera needs no mask of its own; the pincushion one always has its frame of uncovered pixels
    assert n_masked == (len(matcher.seen) if (masks or model == "OPENCV") else 0)


@pytest.mark.parametrize("mode", ["sampled", "dense"])
@pytest.mark.parametrize("model", ["SIMPLE_RADIAL", "OPENCV"])
def test_knob_off_is_the_pinhole_run_byte_for_byte_plus_one_warning(scenes, monkeypatch, caplog, model, mode):
    """With the knob off the coefficients are ignored and no new code runs: the run equals, byte for byte, this code's run of the same scene
    written with pinhole cameras of the same K, and the matcher is handed the plain PIL resize of the decode.  That is what this test proves;
    that a pinhole run writes the bytes it wrote before the knob existed is what the golden tests, which are unchanged, hold."""
    scene, pinhole = scenes(model), scenes(us.PINHOLE_OF[model])

    def never(*a, **kw):
        raise AssertionError("the undistortion ran with the knob off")
    monkeypatch.setattr(hb, "host_undistort_image", never)
    with caplog.at_level(logging.INFO, logger="lfd_densify"):
        rc, path, matcher = cli_run(scene, f"off_{mode}.ply", mode, [])
    warnings = [r.getMessage() for r in caplog.records if "distortion" in r.getMessage()]
    assert rc == 0 and len(warnings) == 1 and "undistort_images" in warnings[0] and "ignored" in warnings[0] and model in warnings[0]
    assert [r.levelno for r in caplog.records if "distortion" in r.getMessage()] == [logging.WARNING]
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="lfd_densify"):
        rc2, path2, matcher2 = cli_run(pinhole, f"off_{mode}.ply", mode, [])
    assert rc2 == 0 and not [r for r in caplog.records if "distortion" in r.getMessage()]
    assert open(path, "rb").read() == open(path2, "rb").read()
    for cam_index, seen in matcher.seen.items():
        assert np.array_equal(seen, us.expected_view(scene["cams"][cam_index], SIZE, undistort=False)[0])
        assert np.array_equal(seen, matcher2.seen[cam_index])


def test_the_cli_flag_undistorts_and_a_pinhole_scene_logs_one_line(scenes, monkeypatch, caplog):
    scene = scenes("SIMPLE_RADIAL")
    rc, _path, matcher = cli_run(scene, "flag.ply", "sampled", ["--undistort_images"])
    assert rc == 0
    for cam_index, seen in matcher.seen.items():
        assert np.array_equal(seen, us.expected_view(scene["cams"][cam_index], SIZE, undistort=True)[0])
    pinhole = scenes("PINHOLE")
    rc, off_path, _m = cli_run(pinhole, "plain.ply", "sampled", [])

    def never(*a, **kw):
        raise AssertionError("the undistortion ran on a scene without distortion")
    monkeypatch.setattr(hb, "host_undistort_image", never)
    with caplog.at_level(logging.INFO, logger="lfd_densify"):
        rc2, on_path, _m = cli_run(pinhole, "knob.ply", "sampled", ["--undistort_images"])
    lines = [r.getMessage() for r in caplog.records if "undistort_images" in r.getMessage()]
    assert rc == 0 and rc2 == 0 and len(lines) == 1 and "no camera carries distortion" in lines[0]
    assert open(off_path, "rb").read() == open(on_path, "rb").read()


@pytest.mark.parametrize("model", ["OPENCV_FISHEYE", "SIMPLE_RADIAL_FISHEYE"])
def test_a_fisheye_scene_is_refused_by_name_before_anything_is_matched(scenes, model):
    scene = scenes(model)
    assert all(r.distortion is None and r.distortion_model == model for r in scene["cams"])
    matcher = us.matcher_for(scene)
    with pytest.raises(RuntimeError, match=model + " camera") as e:
        cli_run(scene, "refused.ply", "sampled", ["--undistort_images"], matcher=matcher)
    assert "view_" in str(e.value) and "undistort_images" in str(e.value) and matcher.calls == 0
    assert cli_run(scene, "ignored.ply", "sampled", [], matcher=matcher)[0] == 0        # knob off: upstream's behaviour, the model's pinhole part


class Node:
    def __init__(self, cam):
        self.has_camera, self.camera_uid = True, cam.uid
        self.camera_width, self.camera_height = cam.width, cam.height
        self.camera_focal_x, self.camera_focal_y = float(cam.K[0, 0]), float(cam.K[1, 1])
        self.camera_R, self.camera_T = cam.R, cam.t.reshape(3)
        self.image_path, self.has_mask, self.mask_path = cam.image_path, False, None


@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_the_gui_entry_point_logs_one_line_and_writes_the_knob_off_bytes(scenes, tmp_path, monkeypatch, caplog, mode):
    scene = scenes("SIMPLE_RADIAL")
    nodes = [Node(c) for c in scene["cams"]]

    def gui(out, exp):
        recs = densify.extract_cameras_from_lfs(nodes)
        cfg = lfd.DensePipelineConfig(output_path=out, num_refs=0.75, nns_per_ref=3, seed=3, viz_interval=0, matches_per_ref=2500, pack_workers=1,
                                      backend="host", triangulation_mode=mode, experimental=exp)
        return densify.dense_init_from_lfs(nodes, cfg, matcher=us.RecordingMatcher(recs, setting="turbo", device="cpu", channels=2))
    off, on = str(tmp_path / "off.ply"), str(tmp_path / "on.ply")
    assert gui(off, {}) == (0, off)

    def never(*a, **kw):
        raise AssertionError("the undistortion ran for cameras that carry no distortion")
    monkeypatch.setattr(hb, "host_undistort_image", never)
    with caplog.at_level(logging.INFO, logger="lfd_densify"):
        assert gui(on, {"undistort_images": True}) == (0, on)
    lines = [r.getMessage() for r in caplog.records if "undistort_images" in r.getMessage()]
    assert len(lines) == 1 and "no camera carries distortion" in lines[0]
    assert open(off, "rb").read() == open(on, "rb").read()
    # an unsupported model reaches the GUI's caller as (1, message)
    fisheye = densify.extract_cameras_from_lfs(nodes)
    for r in fisheye:
        r.distortion_model = "FOV"
    monkeypatch.setattr(densify, "extract_cameras_from_lfs", lambda _nodes: fisheye)
    code, msg = gui(str(tmp_path / "refused.ply"), {"undistort_images": True})
    assert code == 1 and "FOV camera" in msg and "undistort_images" in msg


def test_an_image_that_is_not_of_the_calibrations_size_is_refused_by_name(scenes, tmp_path):
    """The validity plane and the model are evaluated on the calibration's pixel grid: with the knob on an image of another size stops the run
    before anything is matched, naming the image and both sizes; with the knob off nothing looks."""
    import dataclasses
    from PIL import Image
    scene = scenes("SIMPLE_RADIAL")
    small = str(tmp_path / "half.png")
    Image.open(scene["cams"][0].image_path).resize((us.W // 2, us.H // 2)).save(small)
    cams = [dataclasses.replace(c, image_path=small) if i == 0 else c for i, c in enumerate(scene["cams"])]
    odd = dict(scene, cams=cams)
    matcher = us.matcher_for(odd)
    with pytest.raises(RuntimeError, match=f"half.png is {us.W // 2} x {us.H // 2}, its SIMPLE_RADIAL camera {us.W} x {us.H}"):
        run(odd, "odd.ply", "sampled", True, matcher=matcher)
    assert matcher.calls == 0
    assert run(odd, "odd_off.ply", "sampled", False, matcher=matcher)[0].xyz.shape[0] > 0
