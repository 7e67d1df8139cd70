"""The per-point normals in the driver, on the host backend with the analytic matcher (core/types.py, core/hotpath.py, densify.py): the three
knobs and their refusals, the CLI flags, the new switch paired with every option tests/test_config_matrix.py pairs, and - through both entry
points, in sampled and in dense mode - the file of a knob-on run: the knob-off file's xyz and rgb columns byte for byte plus the normals a direct
estimate_normals call gives for the same points, also behind the point cap and the consensus filter."""
import os

import numpy as np
import pytest
import torch

import cycle_scene
import lichtfeld_densification_plugin_amd as lfd
import test_config_matrix as matrix          # the table of options this file pairs the switch with is THAT file's (its OPTIONS, built as it builds them)
from lichtfeld_densification_plugin_amd import densify, synthetic
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from lichtfeld_densification_plugin_amd.core import pipeline as pl
from lichtfeld_densification_plugin_amd.core.types import EXPERIMENTAL_DEFAULTS

REC15 = np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)])
REC27 = np.dtype([("xyz", "<f4", 3), ("normal", "<f4", 3), ("rgb", "u1", 3)])
ON = {"estimate_normals": True}


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
    return cycle_scene.make_scene(str(tmp_path_factory.mktemp("normals_scene")), n_cams=4)


def records(path, normals: bool):
    head, body = open(path, "rb").read().split(b"end_header\n", 1)
    names = [l.split()[-1].decode() for l in head.split(b"\n") if l.startswith(b"property")]
    assert names == (["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"] if normals else ["x", "y", "z", "red", "green", "blue"])
    rec = np.frombuffer(body, dtype=REC27 if normals else REC15)
    assert f"element vertex {rec.shape[0]}\n".encode() in head
    return rec


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Spy:
    """Every estimate_normals call of a run: what it returned, and what a DIRECT call of a context of its own gives for the same points."""

    def __init__(self, monkeypatch, cams):
        self.calls = []
        plain = hb.HostDensifier.estimate_normals
        spy = self

        def estimate(dens, batch, out, radius, step, thr, with_status=False, counters=None):
            res = plain(dens, batch, out, radius, step, thr, with_status=with_status, counters=counters)
            got = res[0] if with_status else res
            own = hb.HostDensifier(2)
            try:
                own.upload_cameras(cams)
                direct, status = plain(own, batch, got, radius, step, thr, with_status=True)
            finally:
                own.close()
            spy.calls.append(dict(xyz=got.xyz.numpy().copy(), normals=got.normals.numpy().copy(), direct=direct.normals.numpy().copy(),
                                  status=status.numpy().copy(), radius=radius, step=step, thr=thr))
            return res
        monkeypatch.setattr(hb.HostDensifier, "estimate_normals", estimate)

    def by_point(self):
        """xyz bits -> normal bits over every call (a position two references share would have to carry the same normal to be usable)"""
        table = {}
        for c in self.calls:
            for x, n in zip(bits(c["xyz"]), bits(c["normals"])):
                table.setdefault(x.tobytes(), set()).add(n.tobytes())
        return table


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


def test_the_knobs_are_experimental_off_by_default_and_validated():
    assert EXPERIMENTAL_DEFAULTS["estimate_normals"] is False
    assert EXPERIMENTAL_DEFAULTS["normal_radius_cells"] == 3 and EXPERIMENTAL_DEFAULTS["normal_depth_step_rel"] == 0.05
    cfg = lfd.DensePipelineConfig(output_path="a.bin")
    assert cfg.exp("estimate_normals") is False and cfg.problem() is None
    for mode in ("sampled", "dense"):
        for backend in ("device", "host"):
            for exp in (ON, {**ON, "normal_radius_cells": 1}, {**ON, "normal_radius_cells": np.int64(4), "normal_depth_step_rel": 0.2},
                        {**ON, "min_support_views": 1, "multiview_refine": True, "max_depth_sigma_rel": 0.05, "match_sigma_px": 0.5},
                        {**ON, "min_consensus_refs": 1, "consensus_radius": 0.1}):
                assert lfd.DensePipelineConfig(output_path="a.PLY", triangulation_mode=mode, backend=backend, max_points=10, experimental=exp).problem() is None
    refused = [
        (dict(), {"estimate_normals": 1}, r"estimate_normals'\] must be True or False"),
        (dict(), {"estimate_normals": "yes"}, r"estimate_normals'\] must be True or False"),
        (dict(), {**ON, "normal_radius_cells": 0}, r"normal_radius_cells'\] must be an integer in 1 \.\. 4"),
        (dict(), {**ON, "normal_radius_cells": 5}, r"normal_radius_cells'\] must be an integer in 1 \.\. 4"),
        (dict(), {**ON, "normal_radius_cells": 2.0}, r"normal_radius_cells'\] must be an integer in 1 \.\. 4"),
        (dict(), {**ON, "normal_radius_cells": True}, r"normal_radius_cells'\] must be an integer in 1 \.\. 4"),
        (dict(), {**ON, "normal_depth_step_rel": 0.0}, r"normal_depth_step_rel'\] must be finite and > 0"),
        (dict(), {**ON, "normal_depth_step_rel": -0.1}, r"normal_depth_step_rel'\] must be finite and > 0"),
        (dict(), {**ON, "normal_depth_step_rel": float("inf")}, r"normal_depth_step_rel'\] must be finite and > 0"),
        (dict(), {**ON, "normal_depth_step_rel": float("nan")}, r"normal_depth_step_rel'\] must be finite and > 0"),
        (dict(), {**ON, "normal_depth_step_rel": "steep"}, r"normal_depth_step_rel'\] must be a number"),
        (dict(), {"normal_radius_cells": 2}, r"normal_radius_cells'\] is the window of the normal estimate: it needs experimental\['estimate_normals'\]"),
        (dict(), {"estimate_normals": False, "normal_depth_step_rel": 0.1},
         r"normal_depth_step_rel'\] is the depth step of the normal estimate: it needs experimental\['estimate_normals'\]"),
        (dict(no_filter=True), ON, r"estimate_normals'\] takes a window cell by the two-view tests; no_filter"),
        (dict(stream_output=True), ON, r"estimate_normals'\] writes 27-byte vertices .* stream_output"),
        (dict(triangulation_mode="dense", stream_output=True), ON, r"estimate_normals'\] writes 27-byte vertices .* stream_output"),
        (dict(triangulation_mode="dense"), {**ON, "dense_tile_segments": True}, r"estimate_normals'\] needs the ordered dense result"),
        (dict(), {**ON, "exchange_records": "ply"}, r"estimate_normals'\] adds a column to f32 rows"),
        (dict(), {**ON, "exchange_records": "auto"}, r"estimate_normals'\] adds a column to f32 rows"),
        (dict(voxel_size=0.05), ON, r"estimate_normals'\] cannot be combined with voxel_size"),
        (dict(output_path="points3D.bin"), ON, r"estimate_normals'\] writes the normals as PLY vertex properties: output_path must end in \.ply"),
    ]
    for kw, exp, text in refused:
        with pytest.raises(ValueError, match=text):
            lfd.DensePipelineConfig(**{"output_path": "a.ply", **kw}, experimental=exp)
    # switched off, none of the routes is refused
    for kw in (dict(stream_output=True), dict(voxel_size=0.05), dict(no_filter=True), dict(output_path="points3D.bin")):
        assert lfd.DensePipelineConfig(**{"output_path": "a.ply", **kw}, experimental={"estimate_normals": False}).problem() is None


def test_the_cli_flags_reach_the_configuration():
    ap = densify.build_argparser()
    args = ap.parse_args(["--scene_root", "x", "--estimate_normals", "--normal_radius_cells", "2", "--normal_depth_step_rel", "0.1"])
    assert densify._experimental_from_args(args) == {"estimate_normals": True, "normal_radius_cells": 2, "normal_depth_step_rel": 0.1}
    assert densify._experimental_from_args(ap.parse_args(["--scene_root", "x"])) == {}
    assert densify._experimental_from_args(ap.parse_args(["--scene_root", "x", "--estimate_normals"])) == {"estimate_normals": True}
    with pytest.raises(ValueError, match="needs experimental\\['estimate_normals'\\]"):
        lfd.DensePipelineConfig(output_path="a.ply", experimental=densify._experimental_from_args(ap.parse_args(["--scene_root", "x", "--normal_radius_cells", "2"])))


def test_a_sharded_run_is_refused_when_it_starts(scene, monkeypatch):
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    monkeypatch.setattr(dist, "get_rank", lambda *a: 0)
    cfg = lfd.DensePipelineConfig(output_path=os.path.join(scene["root"], "sharded.ply"), nns_per_ref=3, backend="host", experimental=ON)
    with pytest.raises(ValueError, match="estimate_normals'\\] cannot run sharded"):
        pl.run_dense_pipeline(scene["cams"], scene["refs"], scene["nn"], cfg, matcher=cycle_scene.matcher_for(scene))


def test_the_switch_paired_with_every_option_of_the_matrix(tmp_path_factory):
    """A legal pair gives the plain run's points (and one normal per point), a refused pair its message - at construction and from the driver."""
    from PIL import Image
    from conftest import load_golden
    from helpers import oracle_cams
    g4 = load_golden("g4_pipeline.npz")
    tmp = str(tmp_path_factory.mktemp("normals_matrix"))
    cams = []
    for i, c in enumerate(oracle_cams(g4)):
        path = os.path.join(tmp, f"im{i:02d}.png")
        Image.fromarray(g4["images"][i]).save(path)
        cams.append(lfd.CameraRecord(uid=int(g4["cam_uid"][i]), image_path=path, width=c.width, height=c.height, K=c.K, R=c.R, t=c.t, P=c.P, C=c.C))
    refs = [int(r) for r in g4["refs_local"]]
    table = [[(torch.from_numpy(g4[f"ref{r}_warp"][j]), torch.from_numpy(g4[f"ref{r}_cert"][j])) for j in range(2)] for r in refs]
    sc = dict(cams=cams, refs=refs, nn=g4["nn_table"], table=table, tmp=tmp)

    def run(names, normals, tag):
        kw = matrix._kwargs(names, "host", os.path.join(tmp, tag, "out.ply"))
        if normals:
            kw["experimental"]["estimate_normals"] = True
        return kw, (lambda: pl.run_dense_pipeline(sc["cams"], sc["refs"], sc["nn"], lfd.DensePipelineConfig(**kw), matcher=matrix._Replay(sc["table"])))

    expected_refusals = {"no_filter": "no_filter", "stream": "stream_output", "voxel": "voxel_size", "x:ply_records": "exchange_records",
                         "x:segments": None, "x:shared_file": None, "device_prep": None}       # (None: refused on the host backend whatever the switch)
    outcomes = {}
    for name in sorted(matrix.OPTIONS):
        kw, go = run((name,), True, "on_" + name.replace(":", ""))
        probe = lfd.DensePipelineConfig(output_path="probe.ply")
        for k, v in kw.items():
            setattr(probe, k, v)
        why = probe.problem()
        if why is not None:
            with pytest.raises(ValueError) as e1:
                lfd.DensePipelineConfig(**kw)
            assert str(e1.value) == why
            with pytest.raises(ValueError) as e2:
                pl.run_dense_pipeline(sc["cams"], sc["refs"], sc["nn"], probe, matcher=matrix._Replay(sc["table"]))
            assert why in str(e2.value)
            outcomes[name] = why
            continue
        res = go()
        plain = run((name,), False, "off_" + name.replace(":", ""))[1]()
        assert np.array_equal(bits(res.xyz), bits(plain.xyz)) and np.array_equal(bits(res.rgb), bits(plain.rgb)) and np.array_equal(bits(res.err), bits(plain.err))
        np.testing.assert_array_equal(res.points_per_reference, plain.points_per_reference)
        assert plain.normals is None and plain.device_normals is None
        assert res.normals.shape == res.xyz.shape and res.normals.dtype == np.float32
        length = np.linalg.norm(res.normals.astype(np.float64), axis=1)
        assert (np.abs(length - 1.0) <= 2.0 ** -22).all()
        outcomes[name] = "ran"
    for name, word in expected_refusals.items():
        assert outcomes[name] != "ran", name
        if word:
            assert "estimate_normals" in outcomes[name] and word in outcomes[name], (name, outcomes[name])
    assert sum(1 for v in outcomes.values() if v == "ran") >= 10, outcomes


@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_both_entry_points_write_the_knob_off_points_with_their_normals(scene, tmp_path, monkeypatch, mode):
    off_out, on_out = os.path.join(str(tmp_path), "off.ply"), os.path.join(str(tmp_path), "on.ply")

    def never(*a, **kw):
        raise AssertionError("the normals ran with the knob off")
    with monkeypatch.context() as m:
        m.setattr(hb.HostDensifier, "estimate_normals", never)
        (rc, _), recs = gui_run(scene, off_out, mode, {})
        assert rc == 0
    spy = Spy(monkeypatch, recs)
    (rc, _), _ = gui_run(scene, on_out, mode, {**ON, "normal_radius_cells": 2})
    assert rc == 0 and spy.calls
    off, on = records(off_out, False), records(on_out, True)
    assert off["xyz"].tobytes() == on["xyz"].tobytes() and off["rgb"].tobytes() == on["rgb"].tobytes()
    # the file's normals: the calls' results in emission order, each equal to a direct call over the same points
    for c in spy.calls:
        assert c["radius"] == 2 and c["step"] == 0.05 and np.array_equal(bits(c["normals"]), bits(c["direct"]))
    used = [c for c in spy.calls if c["xyz"].shape[0]]
    assert np.array_equal(bits(np.concatenate([c["xyz"] for c in used])), bits(on["xyz"]))
    assert np.array_equal(bits(np.concatenate([c["normals"] for c in used])), bits(on["normal"]))
    status = np.concatenate([c["status"] for c in used])
    fitted = (status & 0x80) != 0
    print(f"{mode}: {on.shape[0]} points, {int(fitted.sum())} fitted")
    assert fitted.mean() > 0.5
    assert (np.abs(np.linalg.norm(on["normal"].astype(np.float64), axis=1) - 1.0) <= 2.0 ** -22).all()
    # the CLI entry point writes the same kind of file
    rc, cli_off = cli_run(scene, f"cli_off_{mode}.ply", mode, [])
    spy.calls.clear()
    rc2, cli_on = cli_run(scene, f"cli_on_{mode}.ply", mode, ["--estimate_normals", "--normal_radius_cells", "2"])
    assert rc == 0 and rc2 == 0
    c_off, c_on = records(cli_off, False), records(cli_on, True)
    assert c_off["xyz"].tobytes() == c_on["xyz"].tobytes() and c_off["rgb"].tobytes() == c_on["rgb"].tobytes()
    used = [c for c in spy.calls if c["xyz"].shape[0]]
    assert np.array_equal(bits(np.concatenate([c["normals"] for c in used])), bits(c_on["normal"]))


@pytest.mark.parametrize("mode", ["sampled", "dense"])
@pytest.mark.parametrize("what", ["max_points", "min_consensus_refs"])
def test_the_cap_and_the_consensus_filter_take_the_normals_along(scene, tmp_path, monkeypatch, mode, what):
    (rc, _), recs = gui_run(scene, os.path.join(str(tmp_path), "plain.ply"), mode, {})
    spy = Spy(monkeypatch, recs)
    out = os.path.join(str(tmp_path), "full.ply")
    assert gui_run(scene, out, mode, ON)[0][0] == 0
    full = records(out, True)
    table = spy.by_point()
    assert all(len(v) == 1 for v in table.values())             # a position names its normal
    out2 = os.path.join(str(tmp_path), "less.ply")
    if what == "max_points":
        assert gui_run(scene, out2, mode, ON, max_points=700)[0][0] == 0
    else:
        radius = 0.02 if mode == "sampled" else 0.005
        assert gui_run(scene, out2, mode, {**ON, "min_consensus_refs": 1, "consensus_radius": radius})[0][0] == 0
    less = records(out2, True)
    assert 0 < less.shape[0] < full.shape[0] and (what != "max_points" or less.shape[0] == 700)
    for x, n in zip(bits(less["xyz"]), bits(less["normal"])):
        assert table[x.tobytes()] == {n.tobytes()}
    # and the points are the knob-off run's under the same cap / filter
    out3 = os.path.join(str(tmp_path), "less_off.ply")
    exp3 = {} if what == "max_points" else {"min_consensus_refs": 1, "consensus_radius": radius}
    assert gui_run(scene, out3, mode, exp3, **({"max_points": 700} if what == "max_points" else {}))[0][0] == 0
    off = records(out3, False)
    assert off["xyz"].tobytes() == less["xyz"].tobytes() and off["rgb"].tobytes() == less["rgb"].tobytes()
