"""The Gaussian-ready output in the driver, on the host backend with the analytic matcher (core/types.py, densify.py): the knobs
and their refusals, the CLI flags, and - through both entry points - the file of a knob-on run: the 17-property header and 68 bytes a vertex;
count, positions and normals of the estimate_normals-only run byte for byte; f_dc the formula applied to that file's u8 colours; the scales a
brute-force 3-nearest-neighbour search over the file's own positions gives; rot taking +z onto the file's normal - with and without the oriented
fusion and the point cap; gaussian_flatten changing scale_2 alone; the progress message, the log line, and the refusal that names the knob."""
import os

import numpy as np
import pytest

import cycle_scene
import knn_ref as kr
import lichtfeld_densification_plugin_amd as lfd
from lichtfeld_densification_plugin_amd import densify, synthetic
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from lichtfeld_densification_plugin_amd.core.types import EXPERIMENTAL_DEFAULTS
from test_fuse_driver import REC27, Node, cli_run, gui_run

NORMALS = {"estimate_normals": True}
ON = {**NORMALS, "gaussian_init": True}


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    return cycle_scene.make_scene(str(tmp_path_factory.mktemp("gauss_scene")), n_cams=4)


def points_file(path):
    head, body = open(path, "rb").read().split(b"end_header\n", 1)
    return np.frombuffer(body, dtype=REC27)


def gaussians_file(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    names = [l.split()[-1].decode() for l in head.split(b"\n") if l.startswith(b"property")]
    assert names == kr.PROPERTIES and all(l.startswith(b"property float ") for l in head.split(b"\n") if l.startswith(b"property"))
    rec = np.frombuffer(body, dtype=kr.REC68)
    assert f"element vertex {rec.shape[0]}\n".encode() in head and len(raw) == len(head) + len(b"end_header\n") + 68 * rec.shape[0]
    return rec


def check_against_the_points_file(rec, pts, flatten=1.0, opacity=0.1, max_scale=0.0):
    assert rec.shape[0] == pts.shape[0] > 4
    assert rec["xyz"].tobytes() == pts["xyz"].tobytes() and rec["normal"].tobytes() == pts["normal"].tobytes()
    assert rec["f_dc"].tobytes() == kr.dc_of_u8(pts["rgb"]).tobytes()
    assert np.array_equal(rec["opacity"], np.full(rec.shape[0], np.float32(np.log(opacity / (1.0 - opacity)))))
    # the scales: brute force over the file's own positions
    m = np.maximum(kr.brute_dist2(rec["xyz"]), np.float32(1e-7))
    if max_scale > 0:
        m = np.minimum(m, np.float32(max_scale * max_scale))
    ls = 0.5 * np.log(m.astype(np.float64))
    assert kr.ulp_distance(rec["scale"][:, 0], ls.astype(np.float32)).max() <= 1      # (NumPy's log against the C library's: see tests/test_knn_host.py)
    assert np.array_equal(rec["scale"][:, 0], rec["scale"][:, 1])
    assert kr.ulp_distance(rec["scale"][:, 2], (ls + np.log(flatten)).astype(np.float32)).max() <= 1
    # rot takes +z onto the normal
    unit = np.abs(np.linalg.norm(rec["rot"].astype(np.float64), axis=1) - 1.0)
    assert unit.max() < 1e-6 and np.all(rec["rot"][:, 3] == 0)
    err = np.abs(kr.rotate_z(rec["rot"]) - rec["normal"].astype(np.float64)).max()
    print("largest |R(q) z - n| component:", err, " smallest nz:", rec["normal"][:, 2].min())
    assert err <= 1e-6


def test_the_knobs_are_experimental_off_by_default_and_validated():
    assert EXPERIMENTAL_DEFAULTS["gaussian_init"] is False and EXPERIMENTAL_DEFAULTS["gaussian_flatten"] == 1.0
    assert EXPERIMENTAL_DEFAULTS["gaussian_opacity"] == 0.1 and EXPERIMENTAL_DEFAULTS["gaussian_max_scale"] == 0.0
    cfg = lfd.DensePipelineConfig(output_path="a.bin")
    assert cfg.exp("gaussian_init") is False and cfg.problem() is None
    for mode in ("sampled", "dense"):
        for backend in ("device", "host"):
            for exp in (ON, {**ON, "gaussian_flatten": 0.1}, {**ON, "gaussian_flatten": 1}, {**ON, "gaussian_opacity": np.float32(0.5)},
                        {**ON, "gaussian_max_scale": 2}, {**ON, "fuse_voxel_size": 0.05}, {**ON, "min_consensus_refs": 1, "consensus_radius": 0.1},
                        {**ON, "min_freespace_violations": 1}, {"gaussian_init": False}, {"gaussian_flatten": 1.0, "gaussian_opacity": 0.1, "gaussian_max_scale": 0},
                        {**NORMALS, "gaussian_init": False}):
                assert lfd.DensePipelineConfig(output_path="a.PLY", triangulation_mode=mode, backend=backend, max_points=10, experimental=exp).problem() is None
    refused = [
        (dict(), {**NORMALS, "gaussian_init": 1}, r"gaussian_init'\] must be True or False"),
        (dict(), {**NORMALS, "gaussian_init": "yes"}, r"gaussian_init'\] must be True or False"),
        (dict(), {**ON, "gaussian_flatten": 0.0}, r"gaussian_flatten'\] must be a number in \(0, 1\]"),
        (dict(), {**ON, "gaussian_flatten": 1.01}, r"gaussian_flatten'\] must be a number in \(0, 1\]"),
        (dict(), {**ON, "gaussian_flatten": "thin"}, r"gaussian_flatten'\] must be a number in \(0, 1\]"),
        (dict(), {**ON, "gaussian_flatten": True}, r"gaussian_flatten'\] must be a number in \(0, 1\]"),
        (dict(), {**ON, "gaussian_flatten": float("nan")}, r"gaussian_flatten'\] must be a number in \(0, 1\]"),
        (dict(), {**ON, "gaussian_opacity": 0.0}, r"gaussian_opacity'\] must be a number in \(0, 1\)"),
        (dict(), {**ON, "gaussian_opacity": 1.0}, r"gaussian_opacity'\] must be a number in \(0, 1\)"),
        (dict(), {**ON, "gaussian_opacity": None}, r"gaussian_opacity'\] must be a number in \(0, 1\)"),
        (dict(), {**ON, "gaussian_max_scale": -1.0}, r"gaussian_max_scale'\] must be a finite number >= 0"),
        (dict(), {**ON, "gaussian_max_scale": float("inf")}, r"gaussian_max_scale'\] must be a finite number >= 0"),
        (dict(), {**ON, "gaussian_max_scale": float("nan")}, r"gaussian_max_scale'\] must be a finite number >= 0"),
        (dict(), {**NORMALS, "gaussian_flatten": 0.5}, r"gaussian_flatten'\] is the flattening of the initial Gaussians: it needs experimental\['gaussian_init'\]"),
        (dict(), {**NORMALS, "gaussian_opacity": 0.2}, r"gaussian_opacity'\] is the opacity of the initial Gaussians: it needs experimental\['gaussian_init'\]"),
        (dict(), {"gaussian_max_scale": 0.5}, r"gaussian_max_scale'\] is the largest extent of the initial Gaussians: it needs experimental\['gaussian_init'\]"),
        (dict(), {"gaussian_init": True}, r"gaussian_init'\] orients the Gaussians by the points' normals: it needs experimental\['estimate_normals'\]"),
        (dict(), {"estimate_normals": False, "gaussian_init": True}, r"gaussian_init'\] .* needs experimental\['estimate_normals'\]"),
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


def test_the_cli_flags_reach_the_configuration():
    ap = densify.build_argparser()
    args = ap.parse_args(["--scene_root", "x", "--estimate_normals", "--gaussian_init", "--gaussian_flatten", "0.2", "--gaussian_opacity", "0.3",
                          "--gaussian_max_scale", "1.5"])
    assert densify._experimental_from_args(args) == {"estimate_normals": True, "gaussian_init": True, "gaussian_flatten": 0.2, "gaussian_opacity": 0.3,
                                                     "gaussian_max_scale": 1.5}
    assert densify._experimental_from_args(ap.parse_args(["--scene_root", "x"])) == {}
    assert densify._experimental_from_args(ap.parse_args(["--scene_root", "x", "--estimate_normals", "--gaussian_init"])) == ON
    with pytest.raises(ValueError, match="needs experimental\\['gaussian_init'\\]"):
        lfd.DensePipelineConfig(output_path="a.ply", experimental=densify._experimental_from_args(ap.parse_args(["--scene_root", "x", "--gaussian_flatten", "0.5"])))
    with pytest.raises(ValueError, match="needs experimental\\['estimate_normals'\\]"):
        lfd.DensePipelineConfig(output_path="a.ply", experimental=densify._experimental_from_args(ap.parse_args(["--scene_root", "x", "--gaussian_init"])))


@pytest.fixture(scope="module")
def plain_run(scene, tmp_path_factory):
    """the estimate_normals-only files of both entry points, shared by the tests below"""
    tmp = str(tmp_path_factory.mktemp("gauss_plain"))
    out = os.path.join(tmp, "off.ply")
    assert gui_run(scene, out, "sampled", NORMALS)[0] == 0
    rc, cli = cli_run(scene, "gauss_cli_off.ply", "sampled", ["--estimate_normals"])
    assert rc == 0
    return points_file(out), points_file(cli)


def test_both_entry_points_write_the_gaussians_of_the_knob_off_cloud(scene, tmp_path, monkeypatch, plain_run):
    off_gui, off_cli = plain_run
    with monkeypatch.context() as m:                          # the knob off: nothing of the stage runs
        def never(*a, **kw):
            raise AssertionError("the Gaussian stage ran with the knob off")
        m.setattr(hb.HostDensifier, "knn_dist2", never)
        m.setattr(hb.HostDensifier, "pack_gaussians", never)
        m.setattr(densify, "_write_gaussians", never)
        again = os.path.join(str(tmp_path), "off_again.ply")
        assert gui_run(scene, again, "sampled", NORMALS)[0] == 0
        assert points_file(again).tobytes() == off_gui.tobytes()
    msgs, lines = [], []
    monkeypatch.setattr(densify.log, "info", lambda text: lines.append(text))
    on_out = os.path.join(str(tmp_path), "on.ply")
    assert gui_run(scene, on_out, "sampled", ON, msgs) == (0, on_out)
    check_against_the_points_file(gaussians_file(on_out), off_gui)
    assert (96.0, "Initialising Gaussians...") in msgs and msgs.index((95.0, "Writing output PLY...")) < msgs.index((96.0, "Initialising Gaussians..."))
    line = [t for t in lines if t.startswith("Gaussian initialisation")]
    assert len(line) == 1 and line[0].startswith(f"Gaussian initialisation: {off_gui.shape[0]:,} points, cell size ") and "by brute force" in line[0]
    print(line[0])
    rc, cli_on = cli_run(scene, "gauss_cli_on.ply", "sampled", ["--estimate_normals", "--gaussian_init"])
    assert rc == 0
    check_against_the_points_file(gaussians_file(cli_on), off_cli)


def test_dense_mode(scene, tmp_path):
    off_out, on_out = os.path.join(str(tmp_path), "off.ply"), os.path.join(str(tmp_path), "on.ply")
    assert gui_run(scene, off_out, "dense", NORMALS, max_points=3000)[0] == 0
    assert gui_run(scene, on_out, "dense", ON, max_points=3000)[0] == 0
    off = points_file(off_out)
    assert off.shape[0] == 3000
    check_against_the_points_file(gaussians_file(on_out), off)


def test_the_stage_runs_behind_the_fusion_and_the_cap(scene, tmp_path):
    exp = {"fuse_voxel_size": 0.05, "min_consensus_refs": 1, "consensus_radius": 0.02}
    off_out, on_out = os.path.join(str(tmp_path), "off.ply"), os.path.join(str(tmp_path), "on.ply")
    assert gui_run(scene, off_out, "sampled", {**NORMALS, **exp}, max_points=700)[0] == 0
    assert gui_run(scene, on_out, "sampled", {**ON, **exp, "gaussian_max_scale": 0.04, "gaussian_opacity": 0.25}, max_points=700)[0] == 0
    off = points_file(off_out)
    assert 4 < off.shape[0] < 700                              # capped, then fused
    rec = gaussians_file(on_out)
    check_against_the_points_file(rec, off, opacity=0.25, max_scale=0.04)
    assert rec["scale"][:, 0].max() <= np.float32(np.log(0.04)) + 1e-6 and (rec["scale"][:, 0] < np.log(0.04) - 0.05).any()      # the cap acts on some


def test_flatten_changes_scale_2_only(scene, tmp_path, plain_run):
    a_out, b_out = os.path.join(str(tmp_path), "iso.ply"), os.path.join(str(tmp_path), "flat.ply")
    assert gui_run(scene, a_out, "sampled", ON)[0] == 0
    assert gui_run(scene, b_out, "sampled", {**ON, "gaussian_flatten": 0.1})[0] == 0
    a, b = gaussians_file(a_out), gaussians_file(b_out)
    for col in ("xyz", "normal", "f_dc", "opacity", "rot"):
        assert a[col].tobytes() == b[col].tobytes(), col
    assert a["scale"][:, :2].tobytes() == b["scale"][:, :2].tobytes()
    assert np.array_equal(a["scale"][:, 2], a["scale"][:, 0])                                  # 1.0: the isotropic 3DGS initialisation
    assert np.allclose(b["scale"][:, 2].astype(np.float64) - b["scale"][:, 0], np.log(0.1), atol=1e-5)
    check_against_the_points_file(b, plain_run[0], flatten=0.1)


def test_a_data_refusal_names_the_knob_and_writes_no_other_file(scene, tmp_path, monkeypatch):
    plain = hb.HostDensifier.knn_dist2
    monkeypatch.setattr(hb.HostDensifier, "knn_dist2", lambda dens, xyz, cell_size=0.0: plain(dens, xyz[:3], cell_size))       # a three-point cloud
    out = os.path.join(str(tmp_path), "refused.ply")
    code, text = gui_run(scene, out, "sampled", ON)
    assert code == 1 and "experimental['gaussian_init']" in text and "fewer than four points" in text
    assert not os.path.exists(out)
    with pytest.raises(RuntimeError, match=r"experimental\['gaussian_init'\] cannot be applied .* fewer than four points"):
        cli_run(scene, "refused_cli.ply", "sampled", ["--estimate_normals", "--gaussian_init"])
    assert not os.path.exists(os.path.join(scene["root"], "sparse", "0", "refused_cli.ply"))
    # and the real thing through the whole driver: a cap of three points
    monkeypatch.undo()
    code, text = gui_run(scene, out, "sampled", ON, max_points=3)
    assert code == 1 and "experimental['gaussian_init']" in text and "fewer than four points" in text and not os.path.exists(out)
