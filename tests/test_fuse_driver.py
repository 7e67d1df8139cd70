"""Oriented voxel fusion in the driver, on the host backend with the analytic matcher (core/types.py, densify.py): the knob and its refusals, the
CLI flag, the knob paired with every option tests/test_config_matrix.py pairs, and - through both entry points, in sampled and in dense mode -
the file of a knob-on run: the host writer's output of fuse_oriented applied to the cloud and the normals the knob-off run wrote (behind the cap,
behind the consensus filter), while the knob-off file is the one the normals alone give; the progress message, the log line and the refusal that
names the knob."""
import os

import numpy as np
import pytest
import torch

import cycle_scene
import lichtfeld_densification_plugin_amd as lfd
import test_config_matrix as matrix          # the table of options this file pairs the knob with is THAT file's
from lichtfeld_densification_plugin_amd import densify, synthetic
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from lichtfeld_densification_plugin_amd.core import pipeline as pl
from lichtfeld_densification_plugin_amd.core.image_io import to_uint8_rgb
from lichtfeld_densification_plugin_amd.core.types import EXPERIMENTAL_DEFAULTS
from lichtfeld_densification_plugin_amd.core.writers import write_ply

REC27 = np.dtype([("xyz", "<f4", 3), ("normal", "<f4", 3), ("rgb", "u1", 3)])
NORMALS = {"estimate_normals": True}
H = 0.05
ON = {**NORMALS, "fuse_voxel_size": H}


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
    return cycle_scene.make_scene(str(tmp_path_factory.mktemp("fuse_scene")), n_cams=4)


def records(path):
    head, body = open(path, "rb").read().split(b"end_header\n", 1)
    names = [l.split()[-1].decode() for l in head.split(b"\n") if l.startswith(b"property")]
    assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    rec = np.frombuffer(body, dtype=REC27)
    assert f"element vertex {rec.shape[0]}\n".encode() in head
    return rec


class Spy:
    """Every fuse_oriented call of a run: what went in, and what a DIRECT call of a context of its own gives for it."""

    def __init__(self, monkeypatch):
        self.calls = []
        plain = hb.HostDensifier.fuse_oriented
        spy = self

        def fuse(dens, xyz, normals, rgb, voxel_size, with_counts=False):
            rows = plain(dens, xyz, normals, rgb, voxel_size, with_counts=with_counts)
            own = hb.HostDensifier(1)
            try:
                direct = plain(own, xyz.clone(), normals.clone(), rgb.clone(), voxel_size)
                voxels = own.fuse_voxels
            finally:
                own.close()
            spy.calls.append(dict(xyz=xyz.numpy().copy(), normals=normals.numpy().copy(), rgb=rgb.numpy().copy(), h=voxel_size,
                                  direct=[r.numpy().copy() for r in direct], voxels=voxels))
            return rows
        monkeypatch.setattr(hb.HostDensifier, "fuse_oriented", fuse)


def gui_run(scene, out, mode, exp, msgs=None, **cfg_kw):
    nodes = [Node(c) for c in scene["cams"]]
    recs = densify.extract_cameras_from_lfs(nodes)
    matcher = synthetic.SyntheticMatcher(recs, setting="turbo", device="cpu", channels=2)
    cfg = lfd.DensePipelineConfig(output_path=out, num_refs=0.75, nns_per_ref=3, seed=3, viz_interval=0, matches_per_ref=2500, pack_workers=1,
                                  backend="host", triangulation_mode=mode, experimental=exp, **cfg_kw)
    cb = (lambda p, m: msgs.append((p, m))) if msgs is not None else None
    return densify.dense_init_from_lfs(nodes, cfg, progress_callback=cb, matcher=matcher)


def cli_run(scene, out_name, mode, extra, msgs=None):
    args = densify.build_argparser().parse_args(["--scene_root", scene["root"], "--images_subdir", "images_4", "--num_refs", "0.75", "--nns_per_ref", "3",
                                                 "--matches_per_ref", "2500", "--seed", "3", "--pack_workers", "1", "--backend", "host",
                                                 "--triangulation_mode", mode, "--out_name", out_name] + extra)
    matcher = synthetic.SyntheticMatcher(scene["cams"], setting="turbo", device="cpu", channels=2)
    cb = (lambda p, m: msgs.append((p, m))) if msgs is not None else None
    return densify.dense_init(args, progress_callback=cb, matcher=matcher), os.path.join(scene["root"], "sparse", "0", out_name)


def expected_file(call, path):
    """the host writer's file of the direct call's rows"""
    x, n, c = call["direct"]
    write_ply(path, x, to_uint8_rgb(c), n)
    return open(path, "rb").read()


def test_the_knob_is_experimental_off_by_default_and_validated():
    assert EXPERIMENTAL_DEFAULTS["fuse_voxel_size"] == 0.0
    cfg = lfd.DensePipelineConfig(output_path="a.bin")
    assert cfg.exp("fuse_voxel_size") == 0.0 and cfg.problem() is None
    for mode in ("sampled", "dense"):
        for backend in ("device", "host"):
            for exp in (ON, {**NORMALS, "fuse_voxel_size": 1}, {**NORMALS, "fuse_voxel_size": np.float32(0.25)}, {**NORMALS, "fuse_voxel_size": 0},
                        {**ON, "min_consensus_refs": 1, "consensus_radius": 0.1}, {**ON, "min_freespace_violations": 1},
                        {"fuse_voxel_size": 0.0}):
                assert lfd.DensePipelineConfig(output_path="a.PLY", triangulation_mode=mode, backend=backend, max_points=10, experimental=exp).problem() is None
    refused = [
        (dict(), {**NORMALS, "fuse_voxel_size": "wide"}, r"fuse_voxel_size'\] must be a number"),
        (dict(), {**NORMALS, "fuse_voxel_size": None}, r"fuse_voxel_size'\] must be a number"),
        (dict(), {**NORMALS, "fuse_voxel_size": True}, r"fuse_voxel_size'\] must be a number"),
        (dict(), {**NORMALS, "fuse_voxel_size": -0.1}, r"fuse_voxel_size'\] must be finite and >= 0"),
        (dict(), {**NORMALS, "fuse_voxel_size": float("inf")}, r"fuse_voxel_size'\] must be finite and >= 0"),
        (dict(), {**NORMALS, "fuse_voxel_size": float("nan")}, r"fuse_voxel_size'\] must be finite and >= 0"),
        (dict(), {"fuse_voxel_size": H}, r"fuse_voxel_size'\] merges points by the side their normals face: it needs experimental\['estimate_normals'\]"),
        (dict(), {"estimate_normals": False, "fuse_voxel_size": H}, r"fuse_voxel_size'\] .* needs experimental\['estimate_normals'\]"),
        # everything estimate_normals refuses stays refused through the knob
        (dict(no_filter=True), ON, r"estimate_normals'\] takes a window cell by the two-view tests; no_filter"),
        (dict(stream_output=True), ON, r"estimate_normals'\] writes 27-byte vertices .* stream_output"),
        (dict(triangulation_mode="dense"), {**ON, "dense_tile_segments": True}, r"estimate_normals'\] needs the ordered dense result"),
        (dict(), {**ON, "exchange_records": "ply"}, r"estimate_normals'\] adds a column to f32 rows"),
        (dict(voxel_size=0.05), ON, r"estimate_normals'\] cannot be combined with voxel_size"),
        (dict(output_path="points3D.bin"), ON, r"estimate_normals'\] writes the normals as PLY vertex properties: output_path must end in \.ply"),
    ]
    for kw, exp, text in refused:
        with pytest.raises(ValueError, match=text):
            lfd.DensePipelineConfig(**{"output_path": "a.ply", **kw}, experimental=exp)


def test_the_cli_flag_reaches_the_configuration():
    ap = densify.build_argparser()
    args = ap.parse_args(["--scene_root", "x", "--estimate_normals", "--fuse_voxel_size", "0.04"])
    assert densify._experimental_from_args(args) == {"estimate_normals": True, "fuse_voxel_size": 0.04}
    assert densify._experimental_from_args(ap.parse_args(["--scene_root", "x"])) == {}
    with pytest.raises(ValueError, match="needs experimental\\['estimate_normals'\\]"):
        lfd.DensePipelineConfig(output_path="a.ply", experimental=densify._experimental_from_args(ap.parse_args(["--scene_root", "x", "--fuse_voxel_size", "0.04"])))


def test_the_knob_paired_with_every_option_of_the_matrix(tmp_path_factory):
    """The stage runs behind the pipeline: a legal pair gives the pipeline result of the normals alone, a refused pair its message."""
    from PIL import Image
    from conftest import load_golden
    from helpers import oracle_cams
    g4 = load_golden("g4_pipeline.npz")
    tmp = str(tmp_path_factory.mktemp("fuse_matrix"))
    cams = []
    for i, c in enumerate(oracle_cams(g4)):
        path = os.path.join(tmp, f"im{i:02d}.png")
        Image.fromarray(g4["images"][i]).save(path)
        cams.append(lfd.CameraRecord(uid=int(g4["cam_uid"][i]), image_path=path, width=c.width, height=c.height, K=c.K, R=c.R, t=c.t, P=c.P, C=c.C))
    refs = [int(r) for r in g4["refs_local"]]
    table = [[(torch.from_numpy(g4[f"ref{r}_warp"][j]), torch.from_numpy(g4[f"ref{r}_cert"][j])) for j in range(2)] for r in refs]

    def run(names, exp, tag):
        kw = matrix._kwargs(names, "host", os.path.join(tmp, tag, "out.ply"))
        kw["experimental"].update(exp)
        return kw, (lambda: pl.run_dense_pipeline(cams, refs, g4["nn_table"], lfd.DensePipelineConfig(**kw), matcher=matrix._Replay(table)))

    expected_refusals = {"no_filter": "no_filter", "stream": "stream_output", "voxel": "voxel_size", "x:ply_records": "exchange_records"}
    outcomes = {}
    for name in sorted(matrix.OPTIONS):
        kw, go = run((name,), ON, "on_" + name.replace(":", ""))
        probe = lfd.DensePipelineConfig(output_path="probe.ply")
        for k, v in kw.items():
            setattr(probe, k, v)
        why = probe.problem()
        kw_n, go_n = run((name,), NORMALS, "nrm_" + name.replace(":", ""))
        probe_n = lfd.DensePipelineConfig(output_path="probe.ply")
        for k, v in kw_n.items():
            setattr(probe_n, k, v)
        assert why == probe_n.problem()                     # the knob adds no refusal of its own to a run that has the normals
        if why is not None:
            with pytest.raises(ValueError) as e1:
                lfd.DensePipelineConfig(**kw)
            assert str(e1.value) == why
            outcomes[name] = why
            continue
        res, plain = go(), go_n()
        bits = lambda a: np.ascontiguousarray(a).view(np.uint32)                         # noqa: E731
        assert np.array_equal(bits(res.xyz), bits(plain.xyz)) and np.array_equal(bits(res.rgb), bits(plain.rgb))
        assert np.array_equal(bits(res.normals), bits(plain.normals))
        outcomes[name] = "ran"
    for name, word in expected_refusals.items():
        assert outcomes[name] != "ran" and "estimate_normals" in outcomes[name] and word in outcomes[name], (name, outcomes[name])
    assert sum(1 for v in outcomes.values() if v == "ran") >= 10, outcomes


@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_both_entry_points_write_the_fused_rows_of_the_knob_off_cloud(scene, tmp_path, monkeypatch, mode):
    off_out, on_out = os.path.join(str(tmp_path), "off.ply"), os.path.join(str(tmp_path), "on.ply")

    def never(*a, **kw):
        raise AssertionError("the fusion ran with the knob off")
    with monkeypatch.context() as m:
        m.setattr(hb.HostDensifier, "fuse_oriented", never)
        m.setattr(densify, "_apply_oriented_fusion", never)
        msgs = []
        assert gui_run(scene, off_out, mode, NORMALS, msgs)[0] == 0
        assert not any("Fusing" in t for _, t in msgs)
        rc, cli_off = cli_run(scene, f"cli_off_{mode}.ply", mode, ["--estimate_normals"])
        assert rc == 0
    spy = Spy(monkeypatch)
    msgs, lines = [], []
    monkeypatch.setattr(densify.log, "info", lambda text: lines.append(text))
    assert gui_run(scene, on_out, mode, ON, msgs) == (0, on_out)
    assert len(spy.calls) == 1 and spy.calls[0]["h"] == H
    call = spy.calls[0]
    off = records(off_out)
    # what went in is what the knob-off run wrote: the same points and normals bit for bit, the colours it quantised
    assert off["xyz"].tobytes() == call["xyz"].tobytes() and off["normal"].tobytes() == call["normals"].tobytes()
    assert off["rgb"].tobytes() == to_uint8_rgb(call["rgb"]).tobytes()
    assert open(on_out, "rb").read() == expected_file(call, os.path.join(str(tmp_path), "want.ply"))
    on = records(on_out)
    n_in, n_rows, n_vox = off.shape[0], on.shape[0], call["voxels"]
    assert 0 < n_vox <= n_rows < n_in
    assert (94.0, "Fusing oriented points...") in msgs and msgs.index((94.0, "Fusing oriented points...")) < msgs.index((95.0, "Writing output PLY..."))
    line = [t for t in lines if t.startswith("Oriented fusion")]
    assert line == [f"Oriented fusion ({H:.4f}): {n_in:,} points in, {n_rows:,} rows out, {n_vox:,} voxels, {n_rows - n_vox:,} two-sided"]
    print(line[0])
    # the CLI entry point
    spy.calls.clear()
    msgs = []
    rc, cli_on = cli_run(scene, f"cli_on_{mode}.ply", mode, ["--estimate_normals", "--fuse_voxel_size", str(H)], msgs)
    assert rc == 0 and len(spy.calls) == 1 and any(t == "Fusing oriented points..." for _, t in msgs)
    c_off = records(cli_off)
    assert c_off["xyz"].tobytes() == spy.calls[0]["xyz"].tobytes() and c_off["normal"].tobytes() == spy.calls[0]["normals"].tobytes()
    assert open(cli_on, "rb").read() == expected_file(spy.calls[0], os.path.join(str(tmp_path), "want_cli.ply"))


@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_the_stage_runs_behind_the_consensus_filter_and_the_cap(scene, tmp_path, monkeypatch, mode):
    radius = 0.02 if mode == "sampled" else 0.005
    exp = {"min_consensus_refs": 1, "consensus_radius": radius}
    off_out, on_out = os.path.join(str(tmp_path), "off.ply"), os.path.join(str(tmp_path), "on.ply")
    assert gui_run(scene, off_out, mode, {**NORMALS, **exp}, max_points=700)[0] == 0
    spy = Spy(monkeypatch)
    assert gui_run(scene, on_out, mode, {**ON, **exp}, max_points=700)[0] == 0
    off = records(off_out)
    call = spy.calls[0]
    assert off.shape[0] == 700 == call["xyz"].shape[0]                       # the stage sees the capped cloud of the filtered one
    assert off["xyz"].tobytes() == call["xyz"].tobytes() and off["normal"].tobytes() == call["normals"].tobytes()
    assert open(on_out, "rb").read() == expected_file(call, os.path.join(str(tmp_path), "want.ply"))
    assert records(on_out).shape[0] < 700


def test_a_data_refusal_names_the_knob(scene, tmp_path, monkeypatch):
    def refuse(dens, *a, **kw):
        raise hb.FuseInputRefused("lfd_fuse_oriented_host refused its input (1): lfd_fuse_oriented_host: key range: the linear voxel key does not fit 63 bits")
    monkeypatch.setattr(hb.HostDensifier, "fuse_oriented", refuse)
    code, text = gui_run(scene, os.path.join(str(tmp_path), "refused.ply"), "sampled", ON)
    assert code == 1 and "experimental['fuse_voxel_size'] = 0.05" in text and "key range" in text
    with pytest.raises(RuntimeError, match=r"experimental\['fuse_voxel_size'\] = 0.05 cannot be applied"):
        cli_run(scene, "refused_cli.ply", "sampled", ["--estimate_normals", "--fuse_voxel_size", str(H)])
    # and the real thing: a voxel size the cloud's extent cannot be keyed with
    monkeypatch.undo()
    code, text = gui_run(scene, os.path.join(str(tmp_path), "refused2.ply"), "sampled", {**NORMALS, "fuse_voxel_size": 1e-30})
    assert code == 1 and "fuse_voxel_size" in text and "key range" in text
