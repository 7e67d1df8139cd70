"""The epipolar audit in the driver, on the host backend with the analytic matcher of tests/audit_scene.py (core/types.py,
core/hotpath.py, core/pipeline.py, core/strategies.py, densify.py): the knobs, their flags and every refusal; a knob-off run makes no audit
call and writes nothing beside its file; with the audit on the point file is the knob-off file byte for byte - sampled and dense mode, with
previews, with refs_per_launch 1 and 0 - and <output>.audit.json names the camera whose record was pitched; the maps; the commit rule of the
asynchronous schedules."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import audit_ref
import audit_scene as asc
import colour_scene as cs
import lichtfeld_densification_plugin_amd as lfd
from lichtfeld_densification_plugin_amd import densify
from lichtfeld_densification_plugin_amd.core import audit as audit_report
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from lichtfeld_densification_plugin_amd.core import pipeline as pl
from lichtfeld_densification_plugin_amd.core.hotpath import HotPath
from lichtfeld_densification_plugin_amd.core.types import AUDIT_KNOBS, EXPERIMENTAL_DEFAULTS

ON = {"epipolar_audit": "report"}
PITCHED = (2, 0.5)


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
    return asc.write_scene(str(tmp_path_factory.mktemp("audit_scene")), PITCHED)


def gui_run(cams, out, mode, exp, displaced=None, **cfg_kw):
    nodes = [Node(c) for c in cams]
    matcher = asc.Matcher(densify.extract_cameras_from_lfs(nodes), displaced=displaced)
    kw = dict(output_path=out, num_refs=1.0, nns_per_ref=3, seed=3, viz_interval=0, matches_per_ref=2500, pack_workers=1, backend="host",
              triangulation_mode=mode, experimental=exp)
    kw.update(cfg_kw)
    return densify.dense_init_from_lfs(nodes, lfd.DensePipelineConfig(**kw), matcher=matcher, **({"on_sequential_viz": lambda p: None} if
                                                                                                   kw["viz_interval"] else {}))


def test_the_knobs_are_experimental_off_by_default_and_validated():
    assert EXPERIMENTAL_DEFAULTS["epipolar_audit"] == "off"
    assert [EXPERIMENTAL_DEFAULTS[k] for k in AUDIT_KNOBS] == [0.5, 256, 0.0, ""]
    cfg = lfd.DensePipelineConfig(output_path="a.bin")
    assert cfg.exp("epipolar_audit") == "off" and cfg.problem() is None and cfg.audit_warn_threshold() == cfg.reproj_thresh
    assert lfd.DensePipelineConfig(output_path="a.ply", experimental={**ON, "audit_warn_px": 0.3}).audit_warn_threshold() == 0.3
    for mode in ("sampled", "dense"):
        for backend in ("device", "host"):
            for kw, exp in ((dict(), ON), (dict(no_filter=True), {**ON, "audit_certainty": 1.0, "audit_min_samples": 1}),
                            (dict(max_points=10), {**ON, "audit_maps_dir": "epi", "audit_warn_px": 2.0, "estimate_normals": True}),
                            (dict(), {**ON, "min_support_views": 1, "min_consensus_refs": 1, "consensus_radius": 0.1, "far_shell": "file"})):
                assert lfd.DensePipelineConfig(output_path="a.ply", triangulation_mode=mode, backend=backend, experimental=exp, **kw).problem() is None
    refused = [
        (dict(), {"epipolar_audit": "on"}, r"epipolar_audit'\] must be 'off' or 'report'"),
        (dict(), {"epipolar_audit": True}, r"epipolar_audit'\] must be 'off' or 'report'"),
        (dict(), {**ON, "audit_certainty": 0.0}, r"audit_certainty'\] must be in \(0, 1\]"),
        (dict(), {**ON, "audit_certainty": 1.5}, r"audit_certainty'\] must be in \(0, 1\]"),
        (dict(), {**ON, "audit_certainty": float("nan")}, r"audit_certainty'\] must be in \(0, 1\]"),
        (dict(), {**ON, "audit_min_samples": 0}, r"audit_min_samples'\] must be an integer >= 1"),
        (dict(), {**ON, "audit_min_samples": 2.0}, r"audit_min_samples'\] must be an integer >= 1"),
        (dict(), {**ON, "audit_warn_px": -1.0}, r"audit_warn_px'\] must be a finite number >= 0"),
        (dict(), {**ON, "audit_warn_px": float("inf")}, r"audit_warn_px'\] must be a finite number >= 0"),
        (dict(), {**ON, "audit_maps_dir": 3}, r"audit_maps_dir'\] must be a string"),
        (dict(), {"audit_certainty": 0.7}, r"audit_certainty'\] is a knob of the epipolar audit: it needs experimental\['epipolar_audit'\] = 'report'"),
        (dict(), {"audit_min_samples": 16}, r"audit_min_samples'\] is a knob of the epipolar audit"),
        (dict(), {"audit_warn_px": 1.0}, r"audit_warn_px'\] is a knob of the epipolar audit"),
        (dict(), {"audit_maps_dir": "epi"}, r"audit_maps_dir'\] is a knob of the epipolar audit"),
        (dict(reproj_thresh=0.0, sampson_thresh=1.0), ON, r"epipolar_audit'\] warns in pixels: .* must be > 0"),
        (dict(stream_output=True), ON, r"epipolar_audit'\] is launched beside the point stages .* stream_output"),
        (dict(triangulation_mode="dense", stream_output=True), ON, r"epipolar_audit'\] is launched beside the point stages .* stream_output"),
        (dict(triangulation_mode="dense"), {**ON, "dense_tile_segments": True}, r"epipolar_audit'\] is launched beside the ordered dense result"),
        (dict(), {**ON, "exchange_records": "ply"}, r"epipolar_audit'\] is launched beside f32 rows; experimental\['exchange_records'\] must be 'f32'"),
    ]
    for kw, exp, text in refused:
        with pytest.raises(ValueError, match=text):
            lfd.DensePipelineConfig(**{"output_path": "a.ply", **kw}, experimental=exp)
    assert lfd.DensePipelineConfig(output_path="a.ply", reproj_thresh=0.0, sampson_thresh=1.0, experimental={**ON, "audit_warn_px": 0.5}).problem() is None
    assert lfd.DensePipelineConfig(output_path="a.ply", stream_output=True, experimental={"epipolar_audit": "off"}).problem() is None


def test_the_cli_flags_reach_the_configuration():
    ap = densify.build_argparser()
    assert densify._experimental_from_args(ap.parse_args(["--scene_root", "x", "--epipolar_audit", "report"])) == ON
    got = densify._experimental_from_args(ap.parse_args(["--scene_root", "x", "--epipolar_audit", "report", "--audit_certainty", "0.6",
                                                         "--audit_min_samples", "64", "--audit_warn_px", "1.5", "--audit_maps_dir", "epi"]))
    assert got == {**ON, "audit_certainty": 0.6, "audit_min_samples": 64, "audit_warn_px": 1.5, "audit_maps_dir": "epi"}
    assert isinstance(got["audit_min_samples"], int)
    assert densify._experimental_from_args(ap.parse_args(["--scene_root", "x"])) == {}
    assert densify._experimental_from_args(ap.parse_args(["--scene_root", "x", "--epipolar_audit", "off"])) == {}
    with pytest.raises(SystemExit):
        ap.parse_args(["--scene_root", "x", "--epipolar_audit", "fix"])


def test_a_sharded_run_is_refused_when_it_starts(cams, tmp_path, monkeypatch):
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    monkeypatch.setattr(dist, "get_rank", lambda *a: 0)
    cfg = lfd.DensePipelineConfig(output_path=os.path.join(str(tmp_path), "sharded.ply"), nns_per_ref=3, backend="host", experimental=ON)
    with pytest.raises(ValueError, match="epipolar_audit'\\] cannot run sharded"):
        pl.run_dense_pipeline(cams, [0, 1, 2], [asc.neighbours(r, 3) for r in range(6)], cfg, matcher=asc.Matcher(cams))


@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_the_audit_moves_nothing_and_names_the_pitched_camera(cams, tmp_path, monkeypatch, mode):
    never_out, off_out, on_out, one_out, viz_out = (os.path.join(str(tmp_path), n) for n in ("never.ply", "off.ply", "on.ply", "one.ply", "viz.ply"))

    def never(*a, **kw):
        raise AssertionError("the audit ran with the knob off")
    with monkeypatch.context() as m:
        m.setattr(hb.HostDensifier, "epipolar_audit", never)
        assert gui_run(cams, never_out, mode, {})[0] == 0 and gui_run(cams, off_out, mode, {"epipolar_audit": "off"})[0] == 0
    plain = open(never_out, "rb").read()
    assert plain == open(off_out, "rb").read() and len(plain) > 20000
    assert not os.path.exists(never_out + ".audit.json") and not os.path.exists(off_out + ".audit.json")
    warned = []
    monkeypatch.setattr(densify.log, "warn", lambda msg: warned.append(str(msg)))
    assert gui_run(cams, on_out, mode, ON)[0] == 0
    assert open(on_out, "rb").read() == plain
    text = open(on_out + ".audit.json").read()
    js = json.loads(text)
    assert audit_report.to_json(js) == text and "maps" not in js
    assert js["knobs"] == {"audit_certainty": 0.5, "audit_min_samples": 256, "audit_warn_px": 0.8}
    uid = int(cams[PITCHED[0]].uid)
    assert js["scene"]["suspects"] == [uid] and len(js["pairs"]) == 18 and js["scene"]["usable_pairs"] == 18
    assert [c["name"] for c in js["cameras"]] == [os.path.basename(c.image_path) for c in cams]
    for p in js["pairs"]:
        assert (p["median_px"] > 1.5) == (uid in (p["reference_uid"], p["neighbour_uid"])) and sum(p["histogram"]) == p["n"] > 1000
    assert len([w for w in warned if "epipolar audit" in w]) == 1 and f"uid {uid}" in warned[0] and os.path.basename(cams[PITCHED[0]].image_path) in warned[0]
    # refs_per_launch 1 (0, the default, above) and previews: the same file, the same report
    assert gui_run(cams, one_out, mode, ON, refs_per_launch=1)[0] == 0
    assert open(one_out, "rb").read() == plain and open(one_out + ".audit.json").read() == text
    assert gui_run(cams, viz_out, mode, ON, viz_interval=1)[0] == 0
    assert open(viz_out, "rb").read() == plain and open(viz_out + ".audit.json").read() == text


def test_the_maps(tmp_path):
    true = asc.write_scene(str(tmp_path / "scene"))
    out = os.path.join(str(tmp_path), "run", "maps.ply")
    box = (10, 30, 20, 44)
    os.makedirs(os.path.dirname(out))
    assert gui_run(true, out, "dense", {**ON, "audit_maps_dir": "epi"}, displaced=box, num_refs=0.5)[0] == 0
    js = json.load(open(out + ".audit.json"))
    refs = js["maps"]["references"]
    assert js["maps"]["dir"] == "epi" and len(refs) == 3 and js["scene"]["suspects"] == []
    files = sorted(os.listdir(os.path.join(str(tmp_path), "run", "epi")))
    assert files == sorted(e["map"] for e in refs) and all(f.endswith("_epi.npy") for f in files)
    for e in refs:
        m = np.load(os.path.join(str(tmp_path), "run", "epi", e["map"]))
        assert m.dtype == np.float32 and m.shape == (e["height"], e["width"]) and e["map"] == os.path.splitext(e["image"])[0] + "_epi.npy"
        assert int(np.isfinite(m).sum()) == e["cells_with_data"] > 0
        inside = np.zeros(m.shape, bool)
        inside[box[0]:box[1], box[2]:box[3]] = True
        assert (m[inside & np.isfinite(m)] >= 2.5).all() and (m[~inside & np.isfinite(m)] == 0).all()
    # two image files with one stem: refused with the depth maps' message, before anything runs
    twins = [c if i else type(c)(**{**c.__dict__, "image_path": os.path.join(str(tmp_path), "other", os.path.basename(true[1].image_path))})
             for i, c in enumerate(true)]
    rc, msg = gui_run(twins, os.path.join(str(tmp_path), "dup.ply"), "dense", {**ON, "audit_maps_dir": "epi"})
    assert rc == 1 and "names a camera's maps after its image file" in msg and not os.path.exists(os.path.join(str(tmp_path), "dup.ply"))


# ---- the commit rule of the asynchronous schedules (core/hotpath.py), on the host ----------------------------------------------------------------
MATCH, H, W, K = 64, 12, 16, 3


def hot_for():
    cfg = lfd.DensePipelineConfig(output_path="a.ply", backend="host", experimental=ON)
    return HotPath(asc.cameras(), cfg, 1.0, MATCH, MATCH, torch.device("cpu"), None)


def launch(hot, scene):
    """What launch_sampled does behind its kernel, with the twin's dense points in the buffers: the stages of ``_filtered``, the audit's launch
    among them, attached to the buffers that ``finish_sampled`` will collect."""
    batch = hb.PreparedBatch([scene.inputs], MATCH, MATCH, cameras=hot.cams)
    out = hot._take_buffers(H * W, 1, K)
    assert hot.dens._lib.lfd_triangulate_dense_host(hot.dens._ctx, C.byref(batch.c), C.byref(cs.params()), C.byref(out.c), out.ref_offsets.data_ptr(),
                                                    out.seg_counts.data_ptr()) == 0
    out = hot._filtered(batch, out)
    assert out.audit_pending is not None
    return batch, out


def want_rows(scenes, times=1):
    cams = asc.cameras()
    rows = {}
    for s in scenes:
        table = audit_ref.audit(cams, [s.inputs], K, MATCH, MATCH, 0.5)[0]
        for j, n in enumerate(s.nbrs):
            rows[(int(cams[s.ref].uid), int(cams[n].uid))] = [times * int(v) for v in table[j]]
    return rows


def test_a_launch_redone_reference_by_reference_counts_once():
    scenes = [asc.make(r, asc.neighbours(r, K), H, W, match=MATCH) for r in range(3)]
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
        assert hot.audit_result()["rows"] == {}
        behind = launch(hot, scenes[1])
        behind[1].audit_pending = None                                                            # launched behind it: SampledLoop._recover drops it
        hot.finish_sampled(behind, check_selection=False)
        assert hot.audit_result()["rows"] == {}
        for i in (0, 1, 2):                                                                       # redone reference by reference: each counts once
            hot.finish_sampled(launch(hot, scenes[i]), check_selection=False)
        assert hot.audit_result()["rows"] == want_rows(scenes) and hot.audit_result()["maps"] is None
        # a refused reference keeps nothing and costs the one behind it nothing
        bad, good = launch(hot, scenes[0]), launch(hot, scenes[1])

        def refuse(*a, **kw):
            del bad[1].collect
            raise ValueError("a must be non-empty")
        bad[1].collect = refuse
        with pytest.raises(ValueError, match="non-empty"):
            hot.finish_sampled(bad)
        hot.finish_sampled(good)
        got, want = hot.audit_result()["rows"], want_rows(scenes)
        want.update(want_rows(scenes[1:2], times=2))
        assert got == want
    finally:
        hot.close()


def test_the_synchronous_routes_count_once_per_launch():
    scenes = [asc.make(r, asc.neighbours(r, K), H, W, match=MATCH) for r in range(2)]
    hot = hot_for()
    try:
        res = hot.dense([s.inputs for s in scenes], None)
        assert res.count > 100 and hot.audit_result()["rows"] == want_rows(scenes)
    finally:
        hot.close()
