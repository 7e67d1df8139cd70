"""The per-image exposure gains in the driver, on the host backend with the analytic matcher (core/types.py,
core/hotpath.py, core/pipeline.py, densify.py): the knob and its refusals, the CLI flag, a knob-off file byte for byte with no json beside
it, and - in sampled and in dense mode, both factor modes, both entry points - the file of a knob-on run: the knob-off file's positions,
counts and order, with the knob-off colours under the rule min(c * f, 1) and the factors ``<output>.gains.json`` lists."""
import json
import os

import numpy as np
import pytest

import cycle_scene
import lichtfeld_densification_plugin_amd as lfd
from lichtfeld_densification_plugin_amd import densify, synthetic
from lichtfeld_densification_plugin_amd.core import gains
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from lichtfeld_densification_plugin_amd.core import pipeline as pl
from lichtfeld_densification_plugin_amd.core.image_io import to_uint8_rgb
from lichtfeld_densification_plugin_amd.core.types import EXPERIMENTAL_DEFAULTS

REC15 = np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)])
LUMA, RGB = {"gain_compensation": "luma"}, {"gain_compensation": "rgb"}


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
    return cycle_scene.make_scene(str(tmp_path_factory.mktemp("gain_scene")), n_cams=4)


def records(path):
    head, body = open(path, "rb").read().split(b"end_header\n", 1)
    rec = np.frombuffer(body, dtype=REC15)
    assert f"element vertex {rec.shape[0]}\n".encode() in head
    return rec


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Spy:
    """What the run's one compensation step was given and what its lfd_gain_apply_host call did."""

    def __init__(self, monkeypatch, tau=1.6):
        self.steps, self.applies, self.accumulates = [], [], 0
        spy, want_tau = self, tau
        plain_step, plain_apply, plain_acc = densify._apply_gain_compensation, hb.HostDensifier.gain_apply, hb.HostDensifier.gain_accumulate

        def step(result, config, camera_records, refs_local, progress_callback=None):
            spy.steps.append(dict(uids=[int(camera_records[int(i)].uid) for i in refs_local], counts=np.asarray(result.points_per_reference).copy(),
                                  xyz=np.asarray(result.xyz).copy(), err=np.asarray(result.err).copy()))
            out = plain_step(result, config, camera_records, refs_local, progress_callback)
            spy.steps[-1].update(out_xyz=np.asarray(out.xyz).copy(), out_err=np.asarray(out.err).copy(),
                                 out_counts=np.asarray(out.points_per_reference).copy())
            return out

        def apply(dens, rgb, ref_counts, factors):
            out = plain_apply(dens, rgb, ref_counts, factors)
            spy.applies.append(dict(before=rgb.numpy().copy(), counts=np.asarray(ref_counts).copy(), factors=np.asarray(factors).copy(),
                                    after=out.numpy().copy()))
            return out

        def accumulate(dens, batch, out, tau, table=None):
            assert tau == want_tau                                                # support_threshold(): 2 * reproj_thresh
            spy.accumulates += 1
            return plain_acc(dens, batch, out, tau, table=table)
        monkeypatch.setattr(densify, "_apply_gain_compensation", step)
        monkeypatch.setattr(hb.HostDensifier, "gain_apply", apply)
        monkeypatch.setattr(hb.HostDensifier, "gain_accumulate", accumulate)


def gui_run(scene, out, mode, exp, **cfg_kw):
    nodes = [Node(c) for c in scene["cams"]]
    matcher = synthetic.SyntheticMatcher(densify.extract_cameras_from_lfs(nodes), setting="turbo", device="cpu", channels=2)
    cfg = lfd.DensePipelineConfig(output_path=out, num_refs=0.75, nns_per_ref=3, seed=3, viz_interval=0, matches_per_ref=2500, pack_workers=1,
                                  backend="host", triangulation_mode=mode, experimental=exp, **cfg_kw)
    return densify.dense_init_from_lfs(nodes, cfg, matcher=matcher)


def cli_run(scene, out_name, mode, extra):
    args = densify.build_argparser().parse_args(["--scene_root", scene["root"], "--images_subdir", "images_4", "--num_refs", "0.75", "--nns_per_ref", "3",
                                                 "--matches_per_ref", "2500", "--seed", "3", "--pack_workers", "1", "--backend", "host",
                                                 "--triangulation_mode", mode, "--out_name", out_name] + extra)
    matcher = synthetic.SyntheticMatcher(scene["cams"], setting="turbo", device="cpu", channels=2)
    return densify.dense_init(args, matcher=matcher), os.path.join(scene["root"], "sparse", "0", out_name)


def test_the_knob_is_experimental_off_by_default_and_validated():
    assert EXPERIMENTAL_DEFAULTS["gain_compensation"] == "off"
    cfg = lfd.DensePipelineConfig(output_path="a.bin")
    assert cfg.exp("gain_compensation") == "off" and cfg.problem() is None
    for mode in ("sampled", "dense"):
        for backend in ("device", "host"):
            for out in ("a.ply", "points3D.bin"):
                for exp in (LUMA, RGB, {**LUMA, "min_support_views": 1}, {**RGB, "support_thresh_px": 2.5},
                            {**LUMA, "min_support_views": 1, "multiview_refine": True, "max_depth_sigma_rel": 0.05, "match_sigma_px": 0.5},
                            {**RGB, "min_consensus_refs": 1, "consensus_radius": 0.1}):
                    assert lfd.DensePipelineConfig(output_path=out, triangulation_mode=mode, backend=backend, max_points=10, voxel_size=0.01,
                                                   experimental=exp).problem() is None
    assert lfd.DensePipelineConfig(output_path="a.ply", experimental={**RGB, "estimate_normals": True, "gaussian_init": True,
                                                                      "fuse_voxel_size": 0.05}).problem() is None
    refused = [
        (dict(), {"gain_compensation": "on"}, r"gain_compensation'\] must be 'off', 'luma' .* or 'rgb'"),
        (dict(), {"gain_compensation": True}, r"gain_compensation'\] must be 'off'"),
        (dict(), {"gain_compensation": 1}, r"gain_compensation'\] must be 'off'"),
        (dict(), {"gain_compensation": None}, r"gain_compensation'\] must be 'off'"),
        (dict(), {**LUMA, "multiview_colour": "mean"}, r"gain_compensation'\] cannot run with experimental\['multiview_colour'\].* two-pass driver is out of scope"),
        (dict(), {**RGB, "multiview_colour": "median"}, r"gain_compensation'\] cannot run with experimental\['multiview_colour'\]"),
        (dict(stream_output=True), LUMA, r"gain_compensation'\] rewrites the colour of the collected cloud .* stream_output"),
        (dict(triangulation_mode="dense", stream_output=True), RGB, r"gain_compensation'\] rewrites the colour of the collected cloud .* stream_output"),
        (dict(triangulation_mode="dense"), {**LUMA, "dense_tile_segments": True}, r"gain_compensation'\] needs the ordered dense result"),
        (dict(), {**LUMA, "exchange_records": "ply"}, r"gain_compensation'\] rewrites f32 rows; experimental\['exchange_records'\] must be 'f32'"),
        (dict(reproj_thresh=0.0), LUMA, r"gain_compensation'\] takes the confirming views by the support filter's test: .* must be > 0"),
    ]
    for kw, exp, text in refused:
        with pytest.raises(ValueError, match=text):
            lfd.DensePipelineConfig(**{"output_path": "a.ply", **kw}, experimental=exp)
    assert lfd.DensePipelineConfig(output_path="a.ply", reproj_thresh=0.0, experimental={**LUMA, "support_thresh_px": 1.5}).problem() is None
    for kw in (dict(stream_output=True), dict(reproj_thresh=0.0)):              # switched off, none of the routes is refused
        assert lfd.DensePipelineConfig(**{"output_path": "a.ply", **kw}, experimental={"gain_compensation": "off"}).problem() is None


def test_the_cli_flag_reaches_the_configuration():
    ap = densify.build_argparser()
    for mode in ("luma", "rgb"):
        assert densify._experimental_from_args(ap.parse_args(["--scene_root", "x", "--gain_compensation", mode])) == {"gain_compensation": mode}
    assert densify._experimental_from_args(ap.parse_args(["--scene_root", "x"])) == {}
    assert densify._experimental_from_args(ap.parse_args(["--scene_root", "x", "--gain_compensation", "off"])) == {}
    with pytest.raises(SystemExit):
        ap.parse_args(["--scene_root", "x", "--gain_compensation", "mean"])


def test_a_sharded_run_is_refused_when_it_starts(scene, monkeypatch):
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    monkeypatch.setattr(dist, "get_rank", lambda *a: 0)
    cfg = lfd.DensePipelineConfig(output_path=os.path.join(scene["root"], "sharded.ply"), nns_per_ref=3, backend="host", experimental=LUMA)
    with pytest.raises(ValueError, match="gain_compensation'\\] cannot run sharded"):
        pl.run_dense_pipeline(scene["cams"], scene["refs"], scene["nn"], cfg, matcher=cycle_scene.matcher_for(scene))


def check_run(spy, off, on, json_path, gain_mode, names):
    """One knob-on run against the knob-off file ``off``: the json, the one apply call, and the file ``on``."""
    assert off.shape[0] > 500 and off["xyz"].tobytes() == on["xyz"].tobytes()             # the same points in the same order
    assert len(spy.steps) == 1 and len(spy.applies) == 1 and spy.accumulates >= 1
    step, call = spy.steps[0], spy.applies[0]
    js = json.load(open(json_path))
    assert js["mode"] == gain_mode and js["components"] == 1 and js["clamped"] == [] and js["min_samples"] == 64
    by_uid = {im["uid"]: im for im in js["images"]}
    assert sorted(im["name"] for im in js["images"]) == sorted(names) and len(by_uid) == len(names)
    assert all(im["pairs"] > 0 and im["samples"] >= 64 * im["pairs"] for im in js["images"])
    rows = []
    for uid in step["uids"]:
        f = by_uid[uid]["factor"]
        rows.append([f] * 3 if gain_mode == "luma" else f)
        assert isinstance(f, float) if gain_mode == "luma" else (isinstance(f, list) and len(f) == 3)
    factors = np.asarray(rows, np.float32)
    assert np.array_equal(bits(call["factors"]), bits(factors)) and np.array_equal(call["counts"], step["counts"])
    assert np.abs(factors - 1.0).max() < 0.2 and (factors != 1.0).any()
    if gain_mode == "rgb":
        assert (factors[:, 0] != factors[:, 1]).any()
    # only the colour changes
    for name in ("xyz", "err", "counts"):
        assert np.array_equal(step[name], step["out_" + name])
    want = gains.apply_rule(call["before"], np.repeat(factors, step["counts"], axis=0))
    assert np.array_equal(bits(call["after"]), bits(want))
    assert np.array_equal(bits(step["xyz"]), bits(on["xyz"]))
    assert np.array_equal(to_uint8_rgb(call["before"]), off["rgb"])                        # what went in is the knob-off colour
    assert np.array_equal(to_uint8_rgb(want), on["rgb"]) and off["rgb"].tobytes() != on["rgb"].tobytes()


@pytest.mark.parametrize("mode,gain_mode", [("sampled", "luma"), ("dense", "rgb"), ("sampled", "rgb"), ("dense", "luma")])
def test_knob_off_is_the_plain_file_and_knob_on_rewrites_the_colours_only(scene, tmp_path, monkeypatch, mode, gain_mode):
    never_out, off_out, on_out = (os.path.join(str(tmp_path), n) for n in ("never.ply", "off.ply", "on.ply"))

    def never(*a, **kw):
        raise AssertionError("a gain stage ran with the knob off")
    with monkeypatch.context() as m:
        m.setattr(hb.HostDensifier, "gain_accumulate", never)
        m.setattr(hb.HostDensifier, "gain_apply", never)
        rc, _ = gui_run(scene, never_out, mode, {})
        rc2, _ = gui_run(scene, off_out, mode, {"gain_compensation": "off"})
        assert rc == 0 and rc2 == 0
    assert open(never_out, "rb").read() == open(off_out, "rb").read()
    assert not os.path.exists(never_out + ".gains.json") and not os.path.exists(off_out + ".gains.json")
    names = [os.path.basename(c.image_path) for c in scene["cams"]]
    with monkeypatch.context() as m:
        spy = Spy(m)
        rc, _ = gui_run(scene, on_out, mode, {"gain_compensation": gain_mode})
        assert rc == 0
    check_run(spy, records(off_out), records(on_out), on_out + ".gains.json", gain_mode, names)
    # the CLI entry point: the flag gives the same kind of file
    rc, cli_off = cli_run(scene, f"cli_off_{mode}_{gain_mode}.ply", mode, [])
    with monkeypatch.context() as m:
        spy = Spy(m, tau=3.0)                                                             # (the CLI's default reproj_thresh is 1.5)
        rc2, cli_on = cli_run(scene, f"cli_on_{mode}_{gain_mode}.ply", mode, ["--gain_compensation", gain_mode])
    assert rc == 0 and rc2 == 0 and not os.path.exists(cli_off + ".gains.json")
    check_run(spy, records(cli_off), records(cli_on), cli_on + ".gains.json", gain_mode, names)


def test_the_stage_composes_with_the_filters_around_it(scene, tmp_path, monkeypatch):
    """Behind the support filter and the re-triangulation (the statistics are those of the points they leave), in front of the consensus
    filter (which sees the compensated colour and keeps its rows)."""
    around = {"min_support_views": 1, "multiview_refine": True, "min_consensus_refs": 1, "consensus_radius": 0.05}
    off_out, on_out = (os.path.join(str(tmp_path), n) for n in ("off.ply", "on.ply"))
    rc, _ = gui_run(scene, off_out, "dense", around)
    spy = Spy(monkeypatch)
    rc2, _ = gui_run(scene, on_out, "dense", {**around, **LUMA})
    assert rc == 0 and rc2 == 0
    off, on = records(off_out), records(on_out)
    assert off.shape[0] > 300 and off["xyz"].tobytes() == on["xyz"].tobytes() and off["rgb"].tobytes() != on["rgb"].tobytes()
    assert spy.steps[0]["xyz"].shape[0] >= on.shape[0] and len(spy.applies) == 1


def test_images_at_different_exposures_come_out_at_one_through_the_driver(tmp_path_factory, monkeypatch):
    """Which image gets which factor, end to end: the same scene twice, once as it is and once with every photograph multiplied by its own
    gain - 1.15, 0.85 and 1 for the three references, 1 for the fourth camera - before it is written; the matcher is analytic, so both give
    the same points.  The photographs of this scene are patterns of their own, not renderings of one surface, so their contrast is first
    compressed into [0.25, 0.6] (in both copies): every value then stays inside [0.05, 0.95] under every gain, both runs count the same
    samples, and the statistics are linear in ln - every row's ln(B / A) moves by ln(g_b / g_a), the solved factors by 1 / g up to one
    common constant.  The compensated colour of a point is then the plain copy's compensated colour times that constant whichever reference
    made it - unless a factor goes to the wrong reference, which shows as a difference of ln(1.15 / 0.85) = 0.30 between references.
    Compared per reference as the ratio of mean colours.  Asserted at 0.03, the issue's level for the solved factors - a tenth of
    ln(1.15 / 0.85); what remains is the u8 rounding of the scaled photographs, 0.5 / 255 on values above 0.2, averaged over hundreds of
    points: far inside it."""
    from PIL import Image
    plain = cycle_scene.make_scene(str(tmp_path_factory.mktemp("gain_plain")), n_cams=4)
    scaled = cycle_scene.make_scene(str(tmp_path_factory.mktemp("gain_scaled")), n_cams=4)
    out = str(tmp_path_factory.mktemp("gain_exposures"))
    runs = {}

    def rewrite(scene, gain_of):
        for cam in scene["cams"]:
            im = 0.25 + 0.35 * np.asarray(Image.open(cam.image_path)).astype(np.float64) / 255.0
            Image.fromarray(np.rint(255.0 * im * gain_of[int(cam.uid)]).astype(np.uint8)).save(cam.image_path)

    def run(name, scene):
        with monkeypatch.context() as m:
            spy = Spy(m)
            rc, _ = gui_run(scene, os.path.join(out, name + ".ply"), "dense", LUMA)
            assert rc == 0 and len(spy.applies) == 1
        runs[name] = (spy.steps[0], spy.applies[0])

    rewrite(plain, {int(c.uid): 1.0 for c in plain["cams"]})
    run("plain_on", plain)
    # the three references get three different gains, the camera that is only a neighbour 1
    gain_of = {int(c.uid): 1.0 for c in plain["cams"]}
    gain_of.update(zip(runs["plain_on"][0]["uids"], (1.15, 0.85, 1.0)))
    rewrite(scaled, gain_of)
    run("scaled_on", scaled)
    (step_a, call_a), (step_b, call_b) = runs["plain_on"], runs["scaled_on"]
    assert np.array_equal(bits(step_a["xyz"]), bits(step_b["xyz"])) and np.array_equal(step_a["counts"], step_b["counts"])
    assert len(set(step_a["uids"])) == 3 and step_a["uids"] == step_b["uids"]
    assert 0.2 <= call_b["before"].min() and call_b["before"].max() <= 0.7               # nothing leaves the sampled range
    off, on = [], []
    lo = 0
    for uid, n in zip(step_a["uids"], step_a["counts"].tolist()):
        assert n > 200
        mean = lambda a: float(a[lo:lo + n].astype(np.float64).mean())
        off.append(np.log(mean(call_b["before"]) / mean(call_a["before"])) - np.log(gain_of[uid]))      # uncompensated: the reference's own gain
        on.append(np.log(mean(call_b["after"]) / mean(call_a["after"])))
        lo += n
    print("uncompensated, ln(ratio / gain) per reference:", off, "compensated, ln ratio per reference:", on)
    assert max(abs(v) for v in off) <= 0.03
    assert max(on) - min(on) <= 0.03
