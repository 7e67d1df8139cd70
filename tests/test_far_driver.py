"""The far-field shell in the driver, on the host backend with the analytic matcher of tests/far_scene.py (core/types.py,
core/hotpath.py, core/pipeline.py, core/strategies.py, densify.py): the knobs, their flags and every refusal; a knob-off file byte for byte
with nothing beside it and no far call made; 'file' - the main file untouched, the shell PLY and the json beside it; 'merge' - the main
file's records followed by the shell's; both with normals; the commit rule of the asynchronous schedules; the json's overlap count."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import colour_scene as cs
import far_ref
import far_scene as fs
import lichtfeld_densification_plugin_amd as lfd
from lichtfeld_densification_plugin_amd import densify
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from lichtfeld_densification_plugin_amd.core import pipeline as pl
from lichtfeld_densification_plugin_amd.core.hotpath import HotPath
from lichtfeld_densification_plugin_amd.core.types import EXPERIMENTAL_DEFAULTS, FAR_KNOBS

REC15 = np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)])
REC27 = np.dtype([("xyz", "<f4", 3), ("nrm", "<f4", 3), ("rgb", "u1", 3)])
FILE, MERGE = {"far_shell": "file"}, {"far_shell": "merge"}


class Node:
    """A camera node as the GUI hands it to dense_init_from_lfs."""

    def __init__(self, cam):
        self.has_camera, self.camera_uid = True, cam.uid
        self.camera_width, self.camera_height = cam.width, cam.height
        self.camera_focal_x, self.camera_focal_y = float(cam.K[0, 0]), float(cam.K[1, 1])
        self.camera_R, self.camera_T = cam.R, cam.t.reshape(3)
        self.image_path, self.has_mask, self.mask_path = cam.image_path, False, None


@pytest.fixture(scope="module")
def cams(tmp_path_factory):
    return fs.write_scene(str(tmp_path_factory.mktemp("far_scene")))


def records(path, dtype=REC15):
    head, body = open(path, "rb").read().split(b"end_header\n", 1)
    rec = np.frombuffer(body, dtype=dtype)
    assert f"element vertex {rec.shape[0]}\n".encode() in head
    return rec


def gui_run(cams, out, mode, exp, **cfg_kw):
    nodes = [Node(c) for c in cams]
    matcher = fs.Matcher(densify.extract_cameras_from_lfs(nodes))
    cfg = lfd.DensePipelineConfig(output_path=out, num_refs=0.75, nns_per_ref=3, seed=3, viz_interval=0, matches_per_ref=2500, pack_workers=1,
                                  backend="host", triangulation_mode=mode, experimental=exp, **cfg_kw)
    return densify.dense_init_from_lfs(nodes, cfg, matcher=matcher)


def test_the_knobs_are_experimental_off_by_default_and_validated():
    assert EXPERIMENTAL_DEFAULTS["far_shell"] == "off"
    assert [EXPERIMENTAL_DEFAULTS[k] for k in FAR_KNOBS] == [0.0, 0.5, 2, 256, 2, 0.0]
    cfg = lfd.DensePipelineConfig(output_path="a.bin")
    assert cfg.exp("far_shell") == "off" and cfg.problem() is None and cfg.far_threshold() == cfg.reproj_thresh
    assert lfd.DensePipelineConfig(output_path="a.ply", experimental={**FILE, "far_thresh_px": 0.3}).far_threshold() == 0.3
    for mode in ("sampled", "dense"):
        for backend in ("device", "host"):
            for exp in (FILE, MERGE, {**FILE, "far_certainty": 1.0, "far_min_views": 8, "far_shell_cells": 512, "far_min_samples": 1},
                        {**MERGE, "far_shell_cells": 8, "far_shell_radius": 50.0, "far_thresh_px": 0.25, "estimate_normals": True},
                        {**FILE, "min_support_views": 1, "min_consensus_refs": 1, "consensus_radius": 0.1, "gain_compensation": "luma"}):
                assert lfd.DensePipelineConfig(output_path="a.ply", triangulation_mode=mode, backend=backend, max_points=10,
                                               experimental=exp).problem() is None
    assert lfd.DensePipelineConfig(output_path="points3D.bin", experimental=FILE).problem() is None      # the shell is a PLY of its own
    assert lfd.DensePipelineConfig(output_path="a.ply", experimental={**FILE, "estimate_normals": True, "gaussian_init": True}).problem() is None
    refused = [
        (dict(), {"far_shell": "on"}, r"far_shell'\] must be 'off', 'file' .* or 'merge'"),
        (dict(), {"far_shell": True}, r"far_shell'\] must be 'off'"),
        (dict(), {"far_shell": None}, r"far_shell'\] must be 'off'"),
        (dict(), {**FILE, "far_thresh_px": -1.0}, r"far_thresh_px'\] must be a finite number >= 0"),
        (dict(), {**FILE, "far_thresh_px": float("nan")}, r"far_thresh_px'\] must be a finite number >= 0"),
        (dict(), {**FILE, "far_certainty": 0.0}, r"far_certainty'\] must be in \(0, 1\]"),
        (dict(), {**FILE, "far_certainty": 1.5}, r"far_certainty'\] must be in \(0, 1\]"),
        (dict(), {**FILE, "far_min_views": 0}, r"far_min_views'\] must be an integer in 1 .. 8"),
        (dict(), {**FILE, "far_min_views": 9}, r"far_min_views'\] must be an integer in 1 .. 8"),
        (dict(), {**FILE, "far_min_views": 2.0}, r"far_min_views'\] must be an integer in 1 .. 8"),
        (dict(), {**FILE, "far_shell_cells": 7}, r"far_shell_cells'\] must be an integer in 8 .. 512"),
        (dict(), {**FILE, "far_shell_cells": 513}, r"far_shell_cells'\] must be an integer in 8 .. 512"),
        (dict(), {**FILE, "far_min_samples": 0}, r"far_min_samples'\] must be an integer >= 1"),
        (dict(), {**FILE, "far_shell_radius": -2.0}, r"far_shell_radius'\] must be a finite number >= 0"),
        (dict(), {**FILE, "far_shell_radius": float("inf")}, r"far_shell_radius'\] must be a finite number >= 0"),
        (dict(), {"far_shell_cells": 128}, r"far_shell_cells'\] is a knob of the far-field shell: it needs experimental\['far_shell'\]"),
        (dict(), {"far_certainty": 0.7}, r"far_certainty'\] is a knob of the far-field shell"),
        (dict(no_filter=True), FILE, r"far_shell'\] collects the cells the filters drop .* no_filter"),
        (dict(min_parallax_deg=0.0), MERGE, r"far_shell'\] needs min_parallax_deg > 0"),
        (dict(reproj_thresh=0.0), FILE, r"far_shell'\] compares in pixels: .* must be > 0"),
        (dict(stream_output=True), FILE, r"far_shell'\] is placed around the finished cloud; stream_output"),
        (dict(triangulation_mode="dense", stream_output=True), MERGE, r"far_shell'\] is placed around the finished cloud; stream_output"),
        (dict(triangulation_mode="dense"), {**FILE, "dense_tile_segments": True}, r"far_shell'\] needs the cloud as arrays; .*dense_tile_segments"),
        (dict(), {**FILE, "exchange_records": "ply"}, r"far_shell'\] measures the cloud's f32 rows; experimental\['exchange_records'\] must be 'f32'"),
        (dict(), {**MERGE, "estimate_normals": True, "gaussian_init": True}, r"far_shell'\] = 'merge' cannot run with experimental\['gaussian_init'\]"),
        (dict(output_path="points3D.bin"), MERGE, r"far_shell'\] = 'merge' appends PLY records: output_path must end in .ply"),
    ]
    for kw, exp, text in refused:
        with pytest.raises(ValueError, match=text):
            lfd.DensePipelineConfig(**{"output_path": "a.ply", **kw}, experimental=exp)
    assert lfd.DensePipelineConfig(output_path="a.ply", reproj_thresh=0.0, sampson_thresh=1.0, experimental={**FILE, "far_thresh_px": 0.5}).problem() is None
    for kw in (dict(stream_output=True), dict(no_filter=True), dict(min_parallax_deg=0.0)):     # switched off, none of the routes is refused
        assert lfd.DensePipelineConfig(**{"output_path": "a.ply", **kw}, experimental={"far_shell": "off"}).problem() is None


def test_the_cli_flags_reach_the_configuration():
    ap = densify.build_argparser()
    for mode in ("file", "merge"):
        assert densify._experimental_from_args(ap.parse_args(["--scene_root", "x", "--far_shell", mode])) == {"far_shell": mode}
    got = densify._experimental_from_args(ap.parse_args(["--scene_root", "x", "--far_shell", "file", "--far_thresh_px", "0.4", "--far_certainty", "0.6",
                                                         "--far_min_views", "3", "--far_shell_cells", "128", "--far_min_samples", "4",
                                                         "--far_shell_radius", "75"]))
    assert got == {"far_shell": "file", "far_thresh_px": 0.4, "far_certainty": 0.6, "far_min_views": 3, "far_shell_cells": 128, "far_min_samples": 4,
                   "far_shell_radius": 75.0}
    assert isinstance(got["far_min_views"], int) and isinstance(got["far_shell_cells"], int)
    assert densify._experimental_from_args(ap.parse_args(["--scene_root", "x"])) == {}
    assert densify._experimental_from_args(ap.parse_args(["--scene_root", "x", "--far_shell", "off"])) == {}
    with pytest.raises(SystemExit):
        ap.parse_args(["--scene_root", "x", "--far_shell", "sky"])


def test_a_sharded_run_is_refused_when_it_starts(cams, tmp_path, monkeypatch):
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    monkeypatch.setattr(dist, "get_rank", lambda *a: 0)
    cfg = lfd.DensePipelineConfig(output_path=os.path.join(str(tmp_path), "sharded.ply"), nns_per_ref=3, backend="host", experimental=FILE)
    with pytest.raises(ValueError, match="far_shell'\\] cannot run sharded"):
        pl.run_dense_pipeline(cams, [0, 1, 2], [[1, 2, 3], [0, 2, 3], [1, 3, 0], [2, 1, 0]], cfg, matcher=fs.Matcher(cams))


def check_shell(shell, js, with_normals):
    """The shell's records against its json: on the sphere, in front of the rig and above the horizon, looking inwards."""
    centre, radius = np.asarray(js["centre"]), js["radius"]
    assert shell.shape[0] == js["cells_kept"] > 200
    d = (shell["xyz"].astype(np.float64) - centre) / radius
    assert np.allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-5)
    assert (d[:, 1] > 0.5).all() and (d[:, 2] > -0.03).all()
    assert shell["rgb"].min() >= 70 and shell["rgb"].max() <= 200                       # the backdrop's texture: 0.55 +- 0.15
    if with_normals:
        assert np.allclose(shell["nrm"].astype(np.float64), -d, atol=1e-5)


@pytest.mark.parametrize("mode,normals", [("dense", False), ("sampled", False), ("dense", True)])
def test_off_is_the_plain_file_file_leaves_it_alone_and_merge_appends(cams, tmp_path, monkeypatch, mode, normals):
    extra = {"estimate_normals": True} if normals else {}
    rec = REC27 if normals else REC15
    never_out, off_out, file_out, merge_out = (os.path.join(str(tmp_path), n) for n in ("never.ply", "off.ply", "file.ply", "merge.ply"))

    def never(*a, **kw):
        raise AssertionError("a far-field stage ran with the knob off")
    with monkeypatch.context() as m:
        m.setattr(hb.HostDensifier, "far_accumulate", never)
        m.setattr(hb.HostDensifier, "far_emit", never)
        rc, _ = gui_run(cams, never_out, mode, dict(extra))
        rc2, _ = gui_run(cams, off_out, mode, {"far_shell": "off", **extra})
        assert rc == 0 and rc2 == 0
    plain = open(never_out, "rb").read()
    assert plain == open(off_out, "rb").read()
    for out in (never_out, off_out):
        assert not os.path.exists(out + ".shell.json") and not os.path.exists(os.path.splitext(out)[0] + "_shell.ply")
    main = records(off_out, rec)
    assert main.shape[0] > 2000
    # the gap: nothing of the knob-off cloud lies beyond the ground (2.2 .. 3 units in front of the rig)
    assert main["xyz"][:, 1].max() < 3.5
    # 'file'
    rc, _ = gui_run(cams, file_out, mode, {**FILE, **extra})
    assert rc == 0 and open(file_out, "rb").read() == plain
    js = json.load(open(file_out + ".shell.json"))
    shell = records(os.path.splitext(file_out)[0] + "_shell.ply", rec)
    check_shell(shell, js, normals)
    assert js["mode"] == "file" and js["far_shell_cells"] == 256 and js["far_min_samples"] == 2 and js["far_min_views"] == 2
    assert js["far_thresh_px"] == 0.8 and js["far_certainty"] == 0.5 and js["far_shell_radius"] == 0.0
    assert js["far_cells_with_a_point"] == 0                                             # the overlap: no far cell also made a point
    assert set(js["far_cells"]) <= {os.path.basename(c.image_path) for c in cams} and len(js["far_cells"]) == 3      # the three references
    assert all(n > 10000 for n in js["far_cells"].values()) and js["samples"] == sum(js["far_cells"].values())
    assert js["cells_occupied"] >= js["cells_kept"] and js["samples_kept"] <= js["samples"]
    # the automatic radius: 10 x the cameras' spread here (the cloud is 3 units away), around the cameras' mean centre
    centre = np.mean([np.asarray(c.C, np.float64) for c in cams], axis=0)
    r_cams = max(float(np.linalg.norm(np.asarray(c.C, np.float64) - centre)) for c in cams)
    r_cloud = float(np.linalg.norm(main["xyz"].astype(np.float64) - centre, axis=1).max())
    assert np.allclose(js["centre"], centre) and np.isclose(js["radius"], max(10.0 * r_cams, 1.25 * r_cloud), rtol=1e-12)
    # 'merge': the main file's records, then the shell's
    rc, _ = gui_run(cams, merge_out, mode, {**MERGE, **extra})
    assert rc == 0
    merged = records(merge_out, rec)
    assert merged[:main.shape[0]].tobytes() == main.tobytes() and merged[main.shape[0]:].tobytes() == shell.tobytes()
    assert json.load(open(merge_out + ".shell.json"))["mode"] == "merge" and not os.path.exists(os.path.splitext(merge_out)[0] + "_shell.ply")


def test_the_shell_composes_with_cap_and_fixed_radius_and_a_bin_output(cams, tmp_path):
    out = os.path.join(str(tmp_path), "points3D.bin")
    rc, _ = gui_run(cams, out, "dense", {**FILE, "far_shell_radius": 40.0, "far_shell_cells": 64, "far_min_samples": 5}, max_points=500)
    assert rc == 0
    js = json.load(open(out + ".shell.json"))
    shell = records(os.path.join(str(tmp_path), "points3D_shell.ply"))
    assert js["radius"] == 40.0 and js["far_shell_cells"] == 64 and shell.shape[0] == js["cells_kept"] > 50
    assert np.allclose(np.linalg.norm(shell["xyz"].astype(np.float64) - np.asarray(js["centre"]), axis=1), 40.0, atol=1e-4)


# ---- the commit rule of the asynchronous schedules (core/hotpath.py), on the host ----------------------------------------------------------------
MATCH, H, W, K = 64, 12, 16, 3


def hot_for():
    cfg = lfd.DensePipelineConfig(output_path="a.ply", backend="host", experimental={**FILE, "far_shell_cells": 32})
    return HotPath(fs.cameras(), cfg, 1.0, MATCH, MATCH, torch.device("cpu"), None)


def launch(hot, scene):
    """What launch_sampled does behind its kernel, with the twin's dense points in the buffers: the stages of ``_filtered``, the far-field
    statistics among them, attached to the buffers that ``finish_sampled`` will collect."""
    batch = hb.PreparedBatch([scene.inputs], MATCH, MATCH)
    out = hot._take_buffers(H * W, 1, K)
    assert hot.dens._lib.lfd_triangulate_dense_host(hot.dens._ctx, C.byref(batch.c), C.byref(cs.params()), C.byref(out.c), out.ref_offsets.data_ptr(),
                                                    out.seg_counts.data_ptr()) == 0
    out = hot._filtered(batch, out)
    assert out.far_pending is not None
    return batch, out


def test_a_launch_redone_reference_by_reference_counts_once():
    scenes = [fs.make(r, fs.others(r, K), H, W, match=MATCH) for r in range(3)]
    cams = fs.cameras()
    want = [far_ref.accumulate(cams, [s.inputs], MATCH, MATCH, 0.8, 0.5, 2, 32) for s in scenes]
    hot = hot_for()
    try:
        handle = launch(hot, scenes[0])
        plain = handle[1].collect

        def void(*a, **kw):
            del handle[1].collect                # (the buffers are recycled: the next launch that takes them collects as usual)
            res = plain(*a, **kw)
            res.sel_status[0] = sorted(hb.SELECT_VOIDS_STREAM)[0]
            return res
        handle[1].collect = void
        assert hot.finish_sampled(handle, check_selection=False) is not None                      # void as a whole: the caller redoes it
        assert int(hot.far_result()["table"].abs().sum()) == 0 and hot.far_result()["far_cells"] == {}
        behind = launch(hot, scenes[1])
        behind[1].far_pending = None                                                              # launched behind it: SampledLoop._recover drops it
        hot.finish_sampled(behind, check_selection=False)
        assert int(hot.far_result()["table"].abs().sum()) == 0
        for i in (0, 1, 2):                                                                       # redone reference by reference: each counts once
            hot.finish_sampled(launch(hot, scenes[i]), check_selection=False)
        got = hot.far_result()
        total = sum(w[0].view(np.int64) for w in want)
        assert np.array_equal(got["table"].numpy(), total)
        assert got["far_cells"] == {int(cams[s.ref].uid): int(w[1][0]) for s, w in zip(scenes, want)} and got["overlap"] == 0
        # a refused reference keeps nothing and costs the one behind it nothing
        bad, good = launch(hot, scenes[0]), launch(hot, scenes[1])

        def refuse(*a, **kw):
            del bad[1].collect
            raise ValueError("a must be non-empty")
        bad[1].collect = refuse
        with pytest.raises(ValueError, match="non-empty"):
            hot.finish_sampled(bad)
        hot.finish_sampled(good)
        assert np.array_equal(hot.far_result()["table"].numpy(), total + want[1][0].view(np.int64))
    finally:
        hot.close()


def test_the_synchronous_routes_accumulate_once_per_launch():
    scenes = [fs.make(r, fs.others(r, K), H, W, match=MATCH) for r in range(2)]
    cams = fs.cameras()
    want, counters, _per = far_ref.accumulate(cams, [s.inputs for s in scenes], MATCH, MATCH, 0.8, 0.5, 2, 32)
    hot = hot_for()
    try:
        res = hot.dense([s.inputs for s in scenes], None)
        assert res.count > 100
        got = hot.far_result()
        assert np.array_equal(got["table"].numpy().view(np.uint64), want) and got["overlap"] == 0
        assert got["far_cells"] == {int(cams[s.ref].uid): int(n) for s, n in zip(scenes, counters)}
    finally:
        hot.close()
