"""The pose refinement in the driver, on the host backend with the analytic matcher of tests/pose_scene.py (core/types.py,
core/hotpath.py, core/pipeline.py, core/strategies.py, densify.py): the knobs, their flags and every refusal; through densify.dense_init on
the scene written to disk, a knob-off run makes no pose call and writes nothing beside its file, and with the refinement on the point file
is the knob-off file byte for byte - sampled and dense mode, refs_per_launch 1 and 0, the GUI's entry point - with <output>.poses.json
beside it; the effect: a second run with pose_corrections has the wrong camera back on its epipolar lines; the commit rule of the
asynchronous schedules."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import colour_scene as cs
import lichtfeld_densification_plugin_amd as lfd
import pose_ref
import pose_scene as ps
from lichtfeld_densification_plugin_amd import densify
from lichtfeld_densification_plugin_amd.core import colmap_io
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from lichtfeld_densification_plugin_amd.core import pipeline as pl
from lichtfeld_densification_plugin_amd.core import poses as pose_report
from lichtfeld_densification_plugin_amd.core.hotpath import HotPath
from lichtfeld_densification_plugin_amd.core.types import EXPERIMENTAL_DEFAULTS, POSE_KNOBS

ON = {"pose_refine": "report"}
WRONG = (2, (0.5, 0.0, 0.0), (0.0, 0.0, 0.0))


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
    root = str(tmp_path_factory.mktemp("pose_scene"))
    return dict(root=root, cams=ps.write_colmap(root, WRONG))


def cli_run(scene, out_name, mode, extra, noise_px=0.0):
    args = densify.build_argparser().parse_args(["--scene_root", scene["root"], "--images_subdir", "images", "--num_refs", "1.0", "--nns_per_ref", "3",
                                                 "--matches_per_ref", "2500", "--seed", "3", "--pack_workers", "1", "--backend", "host",
                                                 "--roma_setting", "turbo", "--triangulation_mode", mode, "--out_name", out_name] + extra)
    records = densify.plan_scene(args)[0]
    return densify.dense_init(args, matcher=ps.Matcher(records, noise_px=noise_px)), os.path.join(scene["root"], "sparse", "0", out_name)


def test_the_knobs_are_experimental_off_by_default_and_validated():
    assert EXPERIMENTAL_DEFAULTS["pose_refine"] == "off" and EXPERIMENTAL_DEFAULTS["pose_corrections"] == ""
    assert [EXPERIMENTAL_DEFAULTS[k] for k in POSE_KNOBS] == [0.5, 8.0, 256]
    cfg = lfd.DensePipelineConfig(output_path="a.bin")
    assert cfg.exp("pose_refine") == "off" and cfg.problem() is None
    for mode in ("sampled", "dense"):
        for backend in ("device", "host"):
            for kw, exp in ((dict(), ON), (dict(no_filter=True), {**ON, "pose_certainty": 1.0, "pose_min_samples": 1, "pose_inlier_px": 64.0}),
                            (dict(max_points=10), {**ON, "epipolar_audit": "report", "estimate_normals": True, "pose_corrections": "x.json"}),
                            (dict(), {**ON, "min_support_views": 1, "min_consensus_refs": 1, "consensus_radius": 0.1, "far_shell": "file"}),
                            (dict(stream_output=True), {"pose_corrections": "x.json"})):
                assert lfd.DensePipelineConfig(output_path="a.ply", triangulation_mode=mode, backend=backend, experimental=exp, **kw).problem() is None
    refused = [
        (dict(), {"pose_refine": "on"}, r"pose_refine'\] must be 'off' or 'report'"),
        (dict(), {"pose_refine": True}, r"pose_refine'\] must be 'off' or 'report'"),
        (dict(), {**ON, "pose_certainty": 0.0}, r"pose_certainty'\] must be in \(0, 1\]"),
        (dict(), {**ON, "pose_certainty": 1.5}, r"pose_certainty'\] must be in \(0, 1\]"),
        (dict(), {**ON, "pose_certainty": float("nan")}, r"pose_certainty'\] must be in \(0, 1\]"),
        (dict(), {**ON, "pose_inlier_px": 0.0}, r"pose_inlier_px'\] must be in \(0, 64\]"),
        (dict(), {**ON, "pose_inlier_px": 64.5}, r"pose_inlier_px'\] must be in \(0, 64\]"),
        (dict(), {**ON, "pose_inlier_px": float("inf")}, r"pose_inlier_px'\] must be in \(0, 64\]"),
        (dict(), {**ON, "pose_min_samples": 0}, r"pose_min_samples'\] must be an integer >= 1"),
        (dict(), {**ON, "pose_min_samples": 2.0}, r"pose_min_samples'\] must be an integer >= 1"),
        (dict(), {"pose_corrections": 3}, r"pose_corrections'\] must be a string"),
        (dict(), {"pose_certainty": 0.7}, r"pose_certainty'\] is a knob of the pose refinement: it needs experimental\['pose_refine'\] = 'report'"),
        (dict(), {"pose_inlier_px": 4.0}, r"pose_inlier_px'\] is a knob of the pose refinement"),
        (dict(), {"pose_min_samples": 16}, r"pose_min_samples'\] is a knob of the pose refinement"),
        (dict(stream_output=True), ON, r"pose_refine'\] is launched beside the point stages .* stream_output"),
        (dict(triangulation_mode="dense", stream_output=True), ON, r"pose_refine'\] is launched beside the point stages .* stream_output"),
        (dict(triangulation_mode="dense"), {**ON, "dense_tile_segments": True}, r"pose_refine'\] is launched beside the ordered dense result"),
        (dict(), {**ON, "exchange_records": "ply"}, r"pose_refine'\] is launched beside f32 rows; experimental\['exchange_records'\] must be 'f32'"),
    ]
    for kw, exp, text in refused:
        with pytest.raises(ValueError, match=text):
            lfd.DensePipelineConfig(**{"output_path": "a.ply", **kw}, experimental=exp)
    assert lfd.DensePipelineConfig(output_path="a.ply", stream_output=True, experimental={"pose_refine": "off"}).problem() is None


def test_the_cli_flags_reach_the_configuration():
    ap = densify.build_argparser()
    assert densify._experimental_from_args(ap.parse_args(["--scene_root", "x", "--pose_refine", "report"])) == ON
    got = densify._experimental_from_args(ap.parse_args(["--scene_root", "x", "--pose_refine", "report", "--pose_certainty", "0.6", "--pose_inlier_px", "4",
                                                         "--pose_min_samples", "64", "--pose_corrections", "a.poses.json"]))
    assert got == {**ON, "pose_certainty": 0.6, "pose_inlier_px": 4.0, "pose_min_samples": 64, "pose_corrections": "a.poses.json"}
    assert isinstance(got["pose_min_samples"], int)
    assert densify._experimental_from_args(ap.parse_args(["--scene_root", "x"])) == {}
    assert densify._experimental_from_args(ap.parse_args(["--scene_root", "x", "--pose_refine", "off"])) == {}
    with pytest.raises(SystemExit):
        ap.parse_args(["--scene_root", "x", "--pose_refine", "apply"])


def test_a_sharded_run_is_refused_when_it_starts(scene, tmp_path, monkeypatch):
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    monkeypatch.setattr(dist, "get_rank", lambda *a: 0)
    cfg = lfd.DensePipelineConfig(output_path=os.path.join(str(tmp_path), "sharded.ply"), nns_per_ref=3, backend="host", experimental=ON)
    with pytest.raises(ValueError, match="pose_refine'\\] cannot run sharded"):
        pl.run_dense_pipeline(scene["cams"], [0, 1, 2], [ps.neighbours(r, 3) for r in range(8)], cfg, matcher=ps.Matcher(scene["cams"]))


@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_the_refinement_moves_nothing_and_writes_the_poses(scene, monkeypatch, mode):
    def never(*a, **kw):
        raise AssertionError("the pose statistics ran with the knob off")
    with monkeypatch.context() as m:
        m.setattr(hb.HostDensifier, "pose_accumulate", never)
        rc, never_out = cli_run(scene, f"never_{mode}.ply", mode, [])
        assert rc == 0
        rc, off_out = cli_run(scene, f"off_{mode}.ply", mode, ["--pose_refine", "off"])
        assert rc == 0
    plain = open(never_out, "rb").read()
    assert plain == open(off_out, "rb").read() and len(plain) > 20000
    assert not os.path.exists(never_out + ".poses.json") and not os.path.exists(off_out + ".poses.json")
    rc, on_out = cli_run(scene, f"on_{mode}.ply", mode, ["--pose_refine", "report"])
    assert rc == 0 and open(on_out, "rb").read() == plain
    text = open(on_out + ".poses.json").read()
    js = pose_report.from_json(text)
    assert pose_report.to_json(js) == text
    assert js["knobs"] == {"pose_certainty": 0.5, "pose_inlier_px": 8.0, "pose_min_samples": 256}
    assert [c["name"] for c in js["cameras"]] == [os.path.basename(c.image_path) for c in scene["cams"]]
    assert len(js["pairs"]) == 24 and js["scene"]["usable_pairs"] == 24 and js["scene"]["cameras_left_out"] == []
    wrong = js["cameras"][WRONG[0]]
    assert wrong["uid"] == scene["cams"][WRONG[0]].uid and 0.35 < wrong["rotation_step_deg"] < 0.5
    assert max(c["rotation_step_deg"] for c in js["cameras"] if c is not wrong) < 0.15
    # refs_per_launch 1 (0, the default, above): the same file, the same report
    rc, one_out = cli_run(scene, f"one_{mode}.ply", mode, ["--pose_refine", "report", "--refs_per_launch", "1"])
    assert rc == 0 and open(one_out, "rb").read() == plain and open(one_out + ".poses.json").read() == text


def audit_worst_bin(path):
    js = json.load(open(path + ".audit.json"))
    return max(p["median_bin"] for p in js["pairs"] if p["usable"])


def relative_rotation_after(js, pairs):
    poses = {c["uid"] - 1: (colmap_io._Rotation(c["qvec"]).matrix(), np.asarray(c["tvec"])) for c in js["cameras"]}
    return ps.worst_relative_rotation_deg(poses, pairs)


def test_effect(scene):
    """Dense mode, the record of camera 2 rotated by 0.5 degrees, the epipolar audit on in both runs.  Run 1 writes poses.json; run 2 takes it
    through pose_corrections.  The second audit's worst pair median bin drops; the corrected relative rotations come within the reference's
    own un-quantised step from the same matches plus the quantisation allowance QUANT_DEG (tests/test_pose_host.py measured
    8.7e-4 degrees between the two steps at the most, the allowance is twice that); a third run from the TRUE records moves no camera by
    more than the reference's own step does, plus the allowance."""
    QUANT_DEG = 1.8e-3
    rc, first = cli_run(scene, "effect_1.ply", "dense", ["--pose_refine", "report", "--epipolar_audit", "report"])
    assert rc == 0
    js = pose_report.from_json(open(first + ".poses.json").read())
    rc, second = cli_run(scene, "effect_2.ply", "dense", ["--pose_corrections", first + ".poses.json", "--epipolar_audit", "report", "--pose_refine", "report"])
    assert rc == 0
    # the driver's neighbour table joins cameras 0 .. 3 and 4 .. 7 by the single pair (3, 4), which fixes five of the seven parameters of one
    # group against the other: the second group's scale and the length of that one baseline are not determined, and the solve says so
    # instead of stepping along them
    assert js["scene"]["dropped_directions"] == 2
    before, after = audit_worst_bin(first), audit_worst_bin(second)
    print("worst pair median bin:", before, "->", after)
    assert before >= 12 and after <= 1
    # the reference's step over the pairs the driver matched, on the matcher's grid
    pairs = [(p["reference_uid"] - 1, p["neighbour_uid"] - 1) for p in js["pairs"]]
    by_ref = {}
    for a, b in pairs:
        by_ref.setdefault(a, []).append(b)
    records = ps.cameras(WRONG)
    refs = [ps.make(a, nb, 320, 320, match=320).inputs for a, nb in sorted(by_ref.items())]
    gn = pose_ref.gn_step(records, refs, 320, 320)
    start = ps.worst_relative_rotation_deg({i: pose_ref.pose64(records[i]) for i in range(ps.N_CAMS)}, pairs)
    ref_after, lib_after = ps.worst_relative_rotation_deg(gn["poses"], pairs), relative_rotation_after(js, pairs)
    print("worst relative rotation:", start, "-> reference", ref_after, "library", lib_after)
    assert 0.49 < start < 0.51 and ref_after < 0.05 and lib_after <= ref_after + QUANT_DEG
    # the second run's own report: what is left is small, and its input poses are the first run's output
    js2 = pose_report.from_json(open(second + ".poses.json").read())
    assert js2["scene"]["max_rotation_step_deg"] < 0.02 and js2["scene"]["rms_px"] < 0.05 < 0.5 < js["scene"]["rms_px"]
    for c1, c2 in zip(js["cameras"], js2["cameras"]):
        assert np.abs(np.asarray(c1["tvec"]) - np.asarray(c2["input_tvec"])).max() < 1e-6
    # from the true records
    true_root = os.path.join(scene["root"], "true")
    true = dict(root=true_root, cams=ps.write_colmap(true_root))
    rc, third = cli_run(true, "true.ply", "dense", ["--pose_refine", "report"], noise_px=0.5)
    assert rc == 0
    js3 = pose_report.from_json(open(third + ".poses.json").read())
    refs = [ps.make(a, nb, 320, 320, match=320, noise_px=0.5).inputs for a, nb in sorted(by_ref.items())]
    gn3 = pose_ref.gn_step(ps.cameras(), refs, 320, 320)
    lib_step, ref_step = max(c["rotation_step_deg"] for c in js3["cameras"]), max(gn3["step_deg"].values())
    print("largest step from the true records (0.5 px noise): reference", ref_step, "library", lib_step)
    assert lib_step <= ref_step + QUANT_DEG


def test_the_gui_entry_point_takes_the_corrections_and_refuses_other_poses(scene, tmp_path):
    cams = scene["cams"]
    nodes = [Node(c) for c in cams]

    def gui(out, exp):
        cfg = lfd.DensePipelineConfig(output_path=out, num_refs=1.0, nns_per_ref=3, seed=3, viz_interval=0, matches_per_ref=2500, pack_workers=1,
                                      backend="host", triangulation_mode="dense", experimental=exp)
        return densify.dense_init_from_lfs(nodes, cfg, matcher=ps.Matcher(densify.extract_cameras_from_lfs(nodes)))
    first = os.path.join(str(tmp_path), "first.ply")
    assert gui(first, {**ON, "epipolar_audit": "report"})[0] == 0
    second = os.path.join(str(tmp_path), "second.ply")
    assert gui(second, {"pose_corrections": first + ".poses.json", "epipolar_audit": "report"})[0] == 0
    assert audit_worst_bin(first) >= 12 and audit_worst_bin(second) <= 1 and not os.path.exists(second + ".poses.json")
    assert len(open(second, "rb").read()) > len(open(first, "rb").read())                  # the wrong camera's points are back
    # a file computed for other poses, and a file that is not there
    other = pose_report.from_json(open(first + ".poses.json").read())
    other["cameras"][3]["input_tvec"][0] += 0.01
    bad = os.path.join(str(tmp_path), "other.poses.json")
    open(bad, "w").write(pose_report.to_json(other))
    rc, msg = gui(os.path.join(str(tmp_path), "third.ply"), {"pose_corrections": bad})
    assert rc == 1 and "computed for other poses" in msg and not os.path.exists(os.path.join(str(tmp_path), "third.ply"))
    rc, msg = gui(os.path.join(str(tmp_path), "fourth.ply"), {"pose_corrections": os.path.join(str(tmp_path), "missing.json")})
    assert rc == 1 and "missing.json" in msg


# ---- the commit rule of the asynchronous schedules (core/hotpath.py), on the host ----------------------------------------------------------------
MATCH, H, W, K = 64, 12, 16, 3


def hot_for():
    cfg = lfd.DensePipelineConfig(output_path="a.ply", backend="host", experimental=ON)
    return HotPath(ps.cameras(WRONG), cfg, 1.0, MATCH, MATCH, torch.device("cpu"), None)


def launch(hot, scene_):
    """What launch_sampled does behind its kernel, with the twin's dense points in the buffers: the stages of ``_filtered``, the pose launch
    among them, attached to the buffers that ``finish_sampled`` will collect."""
    batch = hb.PreparedBatch([scene_.inputs], MATCH, MATCH, cameras=hot.cams)
    out = hot._take_buffers(H * W, 1, K)
    assert hot.dens._lib.lfd_triangulate_dense_host(hot.dens._ctx, C.byref(batch.c), C.byref(cs.params()), C.byref(out.c), out.ref_offsets.data_ptr(),
                                                    out.seg_counts.data_ptr()) == 0
    out = hot._filtered(batch, out)
    assert out.pose_pending is not None
    return batch, out


def want_rows(scenes, times=1):
    cams = ps.cameras(WRONG)
    rows = {}
    for s in scenes:
        table = pose_ref.table(cams, [s.inputs], K, MATCH, MATCH, 0.5, 8.0)[0]
        for j, n in enumerate(s.nbrs):
            rows[(int(cams[s.ref].uid), int(cams[n].uid))] = [times * int(v) for v in table[j]]
    return rows


def test_a_launch_redone_reference_by_reference_counts_once():
    scenes = [ps.make(r, ps.neighbours(r, K), H, W, match=MATCH) for r in (1, 2, 3)]
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
        assert hot.pose_result()["rows"] == {}
        behind = launch(hot, scenes[1])
        behind[1].pose_pending = None                                                             # launched behind it: SampledLoop._recover drops it
        hot.finish_sampled(behind, check_selection=False)
        assert hot.pose_result()["rows"] == {}
        for i in (0, 1, 2):                                                                       # redone reference by reference: each counts once
            hot.finish_sampled(launch(hot, scenes[i]), check_selection=False)
        got = hot.pose_result()["rows"]
        assert got == want_rows(scenes) and any(r[3] > 0 for r in got.values())
        # a refused reference keeps nothing and costs the one behind it nothing
        bad, good = launch(hot, scenes[0]), launch(hot, scenes[1])

        def refuse(*a, **kw):
            del bad[1].collect
            raise ValueError("a must be non-empty")
        bad[1].collect = refuse
        with pytest.raises(ValueError, match="non-empty"):
            hot.finish_sampled(bad)
        hot.finish_sampled(good)
        want = want_rows(scenes)
        want.update(want_rows(scenes[1:2], times=2))
        assert hot.pose_result()["rows"] == want
    finally:
        hot.close()


def test_the_synchronous_routes_count_once_per_launch():
    scenes = [ps.make(r, ps.neighbours(r, K), H, W, match=MATCH) for r in (1, 2)]
    hot = hot_for()
    try:
        res = hot.dense([s.inputs for s in scenes], None)
        assert res.count > 100 and hot.pose_result()["rows"] == want_rows(scenes)
    finally:
        hot.close()
