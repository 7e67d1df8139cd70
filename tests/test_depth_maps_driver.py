"""The depth maps in the driver (core/types.py, densify.py): the knobs and their refusals, the CLI flags, the shared plane rule, and - on the host
backend with the analytic matcher, through both entry points - the files of a knob-on run: one map per loaded camera plus depth_maps.json, each
map the NumPy reference's rendering of the cloud the pipeline returned, the point file byte-identical to the knob-off run's; with normals, the
normal maps.  On the device: the maps equal the reference's rendering of the cloud that very run wrote, read back from its PLY."""
import json
import os

import numpy as np
import pytest

import cycle_scene
import depth_ref as dr
import freespace_ref as fr
import lichtfeld_densification_plugin_amd as lfd
from lichtfeld_densification_plugin_amd import densify
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from lichtfeld_densification_plugin_amd.core.types import EXPERIMENTAL_DEFAULTS
from test_freespace_driver import Node, cli_run, gui_run

STEP = (94.0, "Rendering depth maps...")
DEPENDENT = {"depth_map_cells": 0, "depth_map_splat_cells": 1, "depth_map_window_cells": 3, "depth_map_tol_rel": 0.02}


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    return cycle_scene.make_scene(str(tmp_path_factory.mktemp("depth_scene")), n_cams=4)


def read_ply_xyz(path, normals=False):
    """positions (and normals) of a binary PLY of this package: 15-byte x y z r g b or 27-byte x y z nx ny nz r g b vertices"""
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    n = int(head.split(b"element vertex ")[1].split(b"\n")[0])
    dt = np.dtype([("xyz", "<f4", 3)] + ([("nrm", "<f4", 3)] if normals else []) + [("rgb", "u1", 3)])
    assert len(body) == n * dt.itemsize
    rec = np.frombuffer(body, dt)
    return np.ascontiguousarray(rec["xyz"]), (np.ascontiguousarray(rec["nrm"]) if normals else None)


def check_maps(maps_dir, cams, xyz, normals, plane, r=1, R=3, tol=0.02):
    """every file of the directory against the reference's rendering of (xyz, normals) into ``cams`` (CameraRecords)"""
    P, wh = fr.cameras(cams)
    want = dr.render(xyz, normals, P, wh, plane[0], plane[1], r, R, tol)
    stems = [os.path.splitext(os.path.basename(c.image_path))[0] for c in cams]
    expected = {s + ".npy" for s in stems} | ({s + "_normal.npy" for s in stems} if normals is not None else set()) | {"depth_maps.json"}
    assert set(os.listdir(maps_dir)) == expected
    meta = json.load(open(os.path.join(maps_dir, "depth_maps.json")))
    assert meta["plane"] == {"width": plane[0], "height": plane[1]} and (meta["splat_cells"], meta["window_cells"], meta["tol_rel"]) == (r, R, tol)
    assert meta["points"] == len(xyz) and meta["normals"] == (normals is not None) and len(meta["cameras"]) == len(cams)
    valid_total = 0
    for c, (cam, stem, entry) in enumerate(zip(cams, stems, meta["cameras"])):
        d = np.load(os.path.join(maps_dir, stem + ".npy"))
        assert d.dtype == np.float32 and d.shape == (plane[1], plane[0]) and np.array_equal(dr.bits(d), dr.bits(want[0][c])), stem
        valid = d > 0
        assert entry["image"] == os.path.basename(cam.image_path) and entry["depth"] == stem + ".npy"
        assert (entry["width"], entry["height"], entry["valid_cells"]) == (cam.width, cam.height, int(valid.sum()))
        assert entry["depth_min"] == (float(d[valid].min()) if valid.any() else None) and entry["depth_max"] == (float(d[valid].max()) if valid.any() else None)
        if normals is not None:
            nm = np.load(os.path.join(maps_dir, stem + "_normal.npy"))
            assert nm.dtype == np.float32 and nm.shape == (plane[1], plane[0], 3) and np.array_equal(dr.bits(nm), dr.bits(want[2][c])), stem
            assert entry["normal"] == stem + "_normal.npy" and not nm[~valid].any()
        else:
            assert entry["normal"] is None
        valid_total += int(valid.sum())
    assert valid_total > 0
    return want


def test_the_knobs_are_experimental_off_by_default_and_validated():
    assert EXPERIMENTAL_DEFAULTS["depth_maps_dir"] == "" and {k: EXPERIMENTAL_DEFAULTS[k] for k in DEPENDENT} == DEPENDENT
    on = {"depth_maps_dir": "maps"}
    for mode in ("sampled", "dense"):
        for backend in ("device", "host"):
            assert lfd.DensePipelineConfig(output_path="a.ply", triangulation_mode=mode, backend=backend, experimental=on).problem() is None
    assert lfd.DensePipelineConfig(output_path="a.bin", max_points=10, voxel_size=0.1, experimental={**on, "depth_map_cells": 4096}).problem() is None
    assert lfd.DensePipelineConfig(output_path="a.ply", experimental={**on, "depth_map_cells": np.int64(8), "depth_map_splat_cells": 0,
                                                                      "depth_map_window_cells": 0, "depth_map_tol_rel": 0.5}).problem() is None
    assert lfd.DensePipelineConfig(output_path="a.ply", experimental={**on, "depth_map_splat_cells": 3, "depth_map_window_cells": 8}).problem() is None
    assert lfd.DensePipelineConfig(output_path="a.ply", experimental=dict(DEPENDENT)).problem() is None           # off, all at their defaults
    refused = [
        (dict(), {"depth_maps_dir": None}, r"depth_maps_dir'\] must be a string"),
        (dict(), {"depth_maps_dir": True}, r"depth_maps_dir'\] must be a string"),
        (dict(), {"depth_maps_dir": 3}, r"depth_maps_dir'\] must be a string"),
        (dict(), {**on, "depth_map_cells": 7}, r"depth_map_cells'\] must be 0 \(automatic\) or an integer in 8 .. 4096"),
        (dict(), {**on, "depth_map_cells": 4097}, r"depth_map_cells'\] must be 0 \(automatic\) or an integer in 8 .. 4096"),
        (dict(), {**on, "depth_map_cells": 64.0}, r"depth_map_cells'\] must be 0 \(automatic\) or an integer in 8 .. 4096"),
        (dict(), {**on, "depth_map_cells": True}, r"depth_map_cells'\] must be 0 \(automatic\) or an integer in 8 .. 4096"),
        (dict(), {**on, "depth_map_splat_cells": -1}, r"depth_map_splat_cells'\] must be an integer in 0 .. 3"),
        (dict(), {**on, "depth_map_splat_cells": 4}, r"depth_map_splat_cells'\] must be an integer in 0 .. 3"),
        (dict(), {**on, "depth_map_splat_cells": 1.0}, r"depth_map_splat_cells'\] must be an integer in 0 .. 3"),
        (dict(), {**on, "depth_map_splat_cells": False}, r"depth_map_splat_cells'\] must be an integer in 0 .. 3"),
        (dict(), {**on, "depth_map_window_cells": -1}, r"depth_map_window_cells'\] must be an integer in 0 .. 8"),
        (dict(), {**on, "depth_map_window_cells": 9}, r"depth_map_window_cells'\] must be an integer in 0 .. 8"),
        (dict(), {**on, "depth_map_window_cells": "3"}, r"depth_map_window_cells'\] must be an integer in 0 .. 8"),
        (dict(), {**on, "depth_map_tol_rel": 0.0}, r"depth_map_tol_rel'\] must be in \(0, 1\)"),
        (dict(), {**on, "depth_map_tol_rel": 1.0}, r"depth_map_tol_rel'\] must be in \(0, 1\)"),
        (dict(), {**on, "depth_map_tol_rel": 1.0 - 1e-12}, r"depth_map_tol_rel'\] must be in \(0, 1\)"),               # 1 as an f32
        (dict(), {**on, "depth_map_tol_rel": float("nan")}, r"depth_map_tol_rel'\] must be in \(0, 1\)"),
        (dict(), {**on, "depth_map_tol_rel": True}, r"depth_map_tol_rel'\] must be in \(0, 1\)"),
        (dict(), {**on, "depth_map_tol_rel": "tight"}, r"depth_map_tol_rel'\] must be a number"),
        (dict(), {**on, "depth_map_tol_rel": None}, r"depth_map_tol_rel'\] must be a number"),
        (dict(), {"depth_map_cells": 64}, r"depth_map_cells'\] is the plane size of the depth maps: it needs experimental\['depth_maps_dir'\]"),
        (dict(), {"depth_map_splat_cells": 2}, r"depth_map_splat_cells'\] is the splat radius of the depth maps: it needs"),
        (dict(), {"depth_map_window_cells": 0}, r"depth_map_window_cells'\] is the visibility window of the depth maps: it needs"),
        (dict(), {"depth_map_tol_rel": 0.05}, r"depth_map_tol_rel'\] is the depth tolerance of the depth maps: it needs"),
        (dict(stream_output=True), on, r"depth_maps_dir'\] renders the whole cloud"),
        (dict(triangulation_mode="dense", stream_output=True), on, r"depth_maps_dir'\] renders the whole cloud"),
        (dict(), {**on, "exchange_records": "ply"}, r"depth_maps_dir'\] renders f32 rows"),
        (dict(triangulation_mode="dense"), {**on, "dense_tile_segments": True}, r"depth_maps_dir'\] needs the cloud as arrays"),
    ]
    for kw, exp, text in refused:
        with pytest.raises(ValueError, match=text):
            lfd.DensePipelineConfig(output_path="a.ply", experimental=exp, **kw)
    for kw, exp in ((dict(stream_output=True), {}), (dict(triangulation_mode="dense"), {"dense_tile_segments": True})):      # off: none is refused
        assert lfd.DensePipelineConfig(output_path="a.ply", experimental={**exp, "depth_maps_dir": ""}, **kw).problem() is None


def test_a_sharded_run_is_refused_by_name(scene, tmp_path, monkeypatch):
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    monkeypatch.setattr(dist, "get_rank", lambda *a: 0)
    out = os.path.join(str(tmp_path), "sharded.ply")
    cfg = lfd.DensePipelineConfig(output_path=out, backend="host", experimental={"depth_maps_dir": "maps"})
    recs = densify.extract_cameras_from_lfs([Node(c) for c in scene["cams"]])
    with pytest.raises(ValueError, match=r"depth_maps_dir'\] cannot run sharded over several GPUs"):
        densify.run_dense_pipeline(recs, [0, 1], [[1], [0], [0], [0]], cfg)


def test_the_cli_flags_reach_the_configuration():
    ap = densify.build_argparser()
    args = ap.parse_args(["--scene_root", "x", "--depth_maps_dir", "maps", "--depth_map_cells", "128", "--depth_map_splat_cells", "2",
                          "--depth_map_window_cells", "5", "--depth_map_tol_rel", "0.05"])
    want = {"depth_maps_dir": "maps", "depth_map_cells": 128, "depth_map_splat_cells": 2, "depth_map_window_cells": 5, "depth_map_tol_rel": 0.05}
    assert densify._experimental_from_args(args) == want
    cfg = lfd.DensePipelineConfig(output_path="a.ply", experimental=densify._experimental_from_args(args))
    assert {k: cfg.exp(k) for k in want} == want
    off = ap.parse_args(["--scene_root", "x"])
    assert off.depth_maps_dir == "" and densify._experimental_from_args(off) == {}
    only_on = densify._experimental_from_args(ap.parse_args(["--scene_root", "x", "--depth_maps_dir", "/abs/maps"]))
    assert only_on == {"depth_maps_dir": "/abs/maps"}
    zero = densify._experimental_from_args(ap.parse_args(["--scene_root", "x", "--depth_maps_dir", "m", "--depth_map_window_cells", "0"]))
    assert zero == {"depth_maps_dir": "m", "depth_map_window_cells": 0}                   # an explicit 0 is a value, not "not given"
    for flags, text in ((["--depth_map_cells", "64"], "plane size"), (["--depth_map_splat_cells", "2"], "splat radius"),
                        (["--depth_map_window_cells", "0"], "visibility window"), (["--depth_map_tol_rel", "0.05"], "depth tolerance")):
        with pytest.raises(ValueError, match=text):
            lfd.DensePipelineConfig(output_path="a.ply", experimental=densify._experimental_from_args(ap.parse_args(["--scene_root", "x"] + flags)))


def test_the_plane_rule_is_shared_with_the_free_space_filter():
    cfg = lambda mode, cells=0, m=9000: lfd.DensePipelineConfig(output_path="a.ply", triangulation_mode=mode, matches_per_ref=m,      # noqa: E731
                                                                experimental={"depth_maps_dir": "m", "depth_map_cells": cells})
    assert densify.depth_map_plane(cfg("sampled"), 1297, 840) == (95, 62) == densify.freespace_plane(cfg("sampled"), 1297, 840)
    assert densify.depth_map_plane(cfg("sampled"), 840, 1297) == (62, 95)
    assert densify.depth_map_plane(cfg("dense"), 1297, 840, (560, 864)) == (864, 560) == fr.plane_size(864, 1297, 840)
    assert densify.depth_map_plane(cfg("dense", 96), 1297, 840, (560, 864)) == (96, 62)
    assert densify.freespace_plane(cfg("dense", 96), 1297, 840, (560, 864)) == (864, 560)        # each caller reads its own knob
    with pytest.raises(RuntimeError, match=r"depth_map_cells'\] = 0 takes the matcher's grid"):
        densify.depth_map_plane(cfg("dense"), 1297, 840, None)


class Spy:
    """keeps the cloud each run's depth-map stage was handed"""

    def __init__(self, monkeypatch):
        self.clouds = []
        stage = densify._write_depth_maps

        def spy(result, *a, **kw):
            self.clouds.append(dict(xyz=result.xyz.copy(), normals=None if result.device_normals is None else result.normals.copy(), grid=result.match_grid))
            return stage(result, *a, **kw)
        monkeypatch.setattr(densify, "_write_depth_maps", spy)


@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_the_gui_entry_point_writes_one_map_per_camera_and_the_knob_off_file(scene, tmp_path, monkeypatch, mode):
    spy = Spy(monkeypatch)

    def never(*a, **kw):
        raise AssertionError("the renderer ran with the knob off")
    off_out, on_out = os.path.join(str(tmp_path), "off.ply"), os.path.join(str(tmp_path), "on.ply")
    with monkeypatch.context() as m:
        m.setattr(hb.HostDensifier, "render_depth", never)
        off_msgs = []
        assert gui_run(scene, off_out, mode, {}, off_msgs, max_points=700) == (0, off_out)
    assert os.listdir(str(tmp_path)) == ["off.ply"]
    msgs = []
    assert gui_run(scene, on_out, mode, {"depth_maps_dir": "maps"}, msgs, max_points=700) == (0, on_out)
    assert open(on_out, "rb").read() == open(off_out, "rb").read()                       # a side output: the point file is the knob-off file
    assert STEP in msgs and STEP not in off_msgs and [p for p, _m in msgs if p != 94.0] == [p for p, _m in off_msgs]
    cloud = spy.clouds[1]
    assert cloud["xyz"].shape[0] > 700 and cloud["normals"] is None                      # the cloud in front of the cap
    recs = densify.extract_cameras_from_lfs([Node(c) for c in scene["cams"]])
    assert len(recs) == 4                                                                # every loaded camera, not only the 3 references
    w, h = recs[0].width, recs[0].height
    plane = fr.plane_size(50 if mode == "sampled" else max(cloud["grid"]), w, h)         # ceil(sqrt(2500)); the matcher's grid
    check_maps(os.path.join(str(tmp_path), "maps"), recs, cloud["xyz"], None, plane)
    # the knobs are used as given, an absolute directory as it is
    other = os.path.join(str(tmp_path), "elsewhere", "m")
    exp = {"depth_maps_dir": other, "depth_map_cells": 16, "depth_map_splat_cells": 0, "depth_map_window_cells": 8, "depth_map_tol_rel": 0.1}
    assert gui_run(scene, on_out, mode, exp, max_points=700) == (0, on_out)
    check_maps(other, recs, cloud["xyz"], None, fr.plane_size(16, w, h), 0, 8, 0.1)


def test_the_cli_entry_point_writes_the_maps_next_to_the_output(scene, monkeypatch):
    spy = Spy(monkeypatch)
    rc, off_path = cli_run(scene, "maps_off.ply", "sampled", [])
    assert rc == 0
    msgs = []
    rc, on_path = cli_run(scene, "maps_on.ply", "sampled", ["--depth_maps_dir", "depth", "--depth_map_splat_cells", "2"], msgs)
    assert rc == 0 and STEP in msgs and open(on_path, "rb").read() == open(off_path, "rb").read()
    cams = scene["cams"]
    plane = fr.plane_size(50, cams[0].width, cams[0].height)
    check_maps(os.path.join(os.path.dirname(on_path), "depth"), cams, spy.clouds[1]["xyz"], None, plane, r=2)


def test_with_normals_the_normal_maps_appear(scene, tmp_path, monkeypatch):
    spy = Spy(monkeypatch)
    out = os.path.join(str(tmp_path), "normals.ply")
    assert gui_run(scene, out, "dense", {"estimate_normals": True, "depth_maps_dir": "maps"}) == (0, out)
    cloud = spy.clouds[0]
    assert cloud["normals"] is not None and cloud["normals"].shape == cloud["xyz"].shape
    recs = densify.extract_cameras_from_lfs([Node(c) for c in scene["cams"]])
    plane = fr.plane_size(max(cloud["grid"]), recs[0].width, recs[0].height)
    check_maps(os.path.join(str(tmp_path), "maps"), recs, cloud["xyz"], cloud["normals"], plane)
    xyz, nrm = read_ply_xyz(out, normals=True)                                            # and they are the PLY's normals: nothing was capped
    assert np.array_equal(dr.bits(xyz), dr.bits(cloud["xyz"])) and np.array_equal(dr.bits(nrm), dr.bits(cloud["normals"]))


def test_two_cameras_with_the_same_stem_end_the_run(scene, tmp_path):
    nodes = [Node(c) for c in scene["cams"]]
    first = nodes[0].image_path
    twin_dir = os.path.join(str(tmp_path), "copy")
    os.makedirs(twin_dir)
    clash = os.path.join(twin_dir, os.path.splitext(os.path.basename(first))[0] + os.path.splitext(nodes[2].image_path)[1])
    with open(nodes[2].image_path, "rb") as src, open(clash, "wb") as dst:
        dst.write(src.read())
    cams = list(scene["cams"])
    import copy
    cams[2] = copy.copy(cams[2])
    cams[2].image_path = clash
    out = os.path.join(str(tmp_path), "clash.ply")
    rc, message = gui_run({**scene, "cams": cams}, out, "sampled", {"depth_maps_dir": "maps"})
    assert rc == 1 and "both give" in message and repr(first) in message and repr(clash) in message
    assert gui_run({**scene, "cams": cams}, out, "sampled", {}) == (0, out)               # the same scene without the knob runs


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_the_device_run_s_maps_are_the_reference_rendering_of_the_cloud_it_wrote(tmp_path, mode):
    import torch
    root = str(tmp_path)
    scene = cycle_scene.make_scene(root, n_cams=4)
    out = os.path.join(root, "dev.ply")
    normals = mode == "dense"
    exp = {"depth_maps_dir": "maps", **({"estimate_normals": True} if normals else {})}
    assert gui_run(scene, out, mode, exp, backend="device", device=torch.device("cuda:0"), max_points=0) == (0, out)
    xyz, nrm = read_ply_xyz(out, normals=normals)                                         # max_points = 0: the file holds the cloud that was rendered
    assert xyz.shape[0] > 1000
    recs = densify.extract_cameras_from_lfs([Node(c) for c in scene["cams"]])
    cells = 50 if mode == "sampled" else None
    meta = json.load(open(os.path.join(root, "maps", "depth_maps.json")))
    plane = (meta["plane"]["width"], meta["plane"]["height"])
    if cells:
        assert plane == fr.plane_size(cells, recs[0].width, recs[0].height)
    check_maps(os.path.join(root, "maps"), recs, xyz, nrm, plane)
