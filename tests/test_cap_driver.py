"""The spatial point cap in the driver, on the host backend with the analytic matcher (core/types.py, densify.py), on the generated scene of
tests/test_fuse_driver.py: the knob, its refusals and the CLI flag; 'random' is the run without the key, byte for byte; with 'spatial' the file has
exactly max_points vertices, each a byte-equal row of the uncapped file in that file's order - the rows the NumPy reference of tests/cap_ref.py
picks for the uncapped cloud -, through both entry points, in both modes, with and without normals, and in front of the oriented fusion, the
Gaussian output, the voxel filter and behind the consensus filter; the log line, the progress message and the refusal that names the knob."""
import os

import numpy as np
import pytest

import cap_ref as cr
import lichtfeld_densification_plugin_amd as lfd
import test_fuse_driver as tf
from lichtfeld_densification_plugin_amd import densify
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from lichtfeld_densification_plugin_amd.core.types import EXPERIMENTAL_DEFAULTS

REC15 = np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)])
SPATIAL = {"cap_mode": "spatial"}
NORMALS = {"estimate_normals": True}
M = 700


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    return tf.cycle_scene.make_scene(str(tmp_path_factory.mktemp("cap_scene")), n_cams=4)


def rows(path):
    """the vertices of a PLY, 15-byte or 27-byte ones"""
    head, body = open(path, "rb").read().split(b"end_header\n", 1)
    rec = np.frombuffer(body, dtype=tf.REC27 if b"property float nx" in head else REC15)
    assert f"element vertex {rec.shape[0]}\n".encode() in head
    return rec


class Spy:
    """Every cap_spatial call of a run on the host backend: what went in and what came out."""

    def __init__(self, monkeypatch):
        self.calls = []
        plain = hb.HostDensifier.cap_spatial
        spy = self

        def cap(dens, xyz, err, budget):
            keep = plain(dens, xyz, err, budget)
            spy.calls.append(dict(xyz=xyz.numpy().copy(), err=None if err is None else err.numpy().copy(), m=budget, keep=keep.numpy().copy(),
                                  stats=dens.cap_stats))
            return keep
        monkeypatch.setattr(hb.HostDensifier, "cap_spatial", cap)


def check_against_uncapped(call, capped, uncapped):
    """The one call of a run saw the uncapped cloud, chose what the reference chooses, and the file holds those rows in the uncapped file's order."""
    assert call["m"] == M and call["xyz"].tobytes() == np.ascontiguousarray(uncapped["xyz"]).tobytes()
    want, want_stats = cr.cap_ref(call["xyz"], call["err"], M)
    assert call["keep"].tolist() == want.tolist() and call["stats"] == want_stats
    assert capped.shape[0] == M and capped.tobytes() == uncapped[want].tobytes()


def test_the_knob_is_experimental_random_by_default_and_validated():
    assert EXPERIMENTAL_DEFAULTS["cap_mode"] == "random"
    cfg = lfd.DensePipelineConfig(output_path="a.bin")
    assert cfg.exp("cap_mode") == "random" and cfg.problem() is None
    for mode in ("sampled", "dense"):
        for backend in ("device", "host"):
            for kw, exp in ((dict(max_points=10), SPATIAL), (dict(max_points=10), {"cap_mode": "random"}), (dict(), {"cap_mode": "random"}),
                            (dict(max_points=10, voxel_size=0.1), SPATIAL), (dict(max_points=10), {**SPATIAL, **NORMALS, "fuse_voxel_size": 0.05}),
                            (dict(max_points=10), {**SPATIAL, **NORMALS, "gaussian_init": True}),
                            (dict(max_points=10), {**SPATIAL, "min_consensus_refs": 1, "consensus_radius": 0.1}),
                            (dict(max_points=10), {**SPATIAL, "min_freespace_violations": 1})):
                assert lfd.DensePipelineConfig(output_path="a.ply", triangulation_mode=mode, backend=backend, experimental=exp, **kw).problem() is None
    refused = [
        (dict(max_points=10), {"cap_mode": "grid"}, r"cap_mode'\] must be 'random' \(upstream's draw\) or 'spatial'"),
        (dict(max_points=10), {"cap_mode": None}, r"cap_mode'\] must be 'random' \(upstream's draw\) or 'spatial'"),
        (dict(max_points=10), {"cap_mode": True}, r"cap_mode'\] must be 'random' \(upstream's draw\) or 'spatial'"),
        (dict(max_points=10), {"cap_mode": 1}, r"cap_mode'\] must be 'random' \(upstream's draw\) or 'spatial'"),
        (dict(max_points=10), {"cap_mode": "Spatial"}, r"cap_mode'\] must be 'random' \(upstream's draw\) or 'spatial'"),
        (dict(), SPATIAL, r"cap_mode'\] = 'spatial' is how max_points chooses: it needs max_points > 0"),
        (dict(max_points=0), SPATIAL, r"cap_mode'\] = 'spatial' is how max_points chooses: it needs max_points > 0"),
        (dict(max_points=10, stream_output=True), SPATIAL, r"stream_output cannot be combined with max_points"),
    ]
    for kw, exp, text in refused:
        with pytest.raises(ValueError, match=text):
            lfd.DensePipelineConfig(**{"output_path": "a.ply", **kw}, experimental=exp)


def test_the_cli_flag_reaches_the_configuration():
    ap = densify.build_argparser()
    args = ap.parse_args(["--scene_root", "x", "--max_points", "5", "--cap_mode", "spatial"])
    assert densify._experimental_from_args(args) == {"cap_mode": "spatial"}
    assert densify._experimental_from_args(ap.parse_args(["--scene_root", "x"])) == {}
    assert densify._experimental_from_args(ap.parse_args(["--scene_root", "x", "--cap_mode", "random"])) == {}
    with pytest.raises(SystemExit):
        ap.parse_args(["--scene_root", "x", "--cap_mode", "grid"])
    with pytest.raises(ValueError, match="it needs max_points > 0"):
        lfd.DensePipelineConfig(output_path="a.ply", experimental=densify._experimental_from_args(ap.parse_args(["--scene_root", "x", "--cap_mode", "spatial"])))


def test_apply_point_cap_takes_the_mode_behind_its_five_arguments():
    xyz, err, _ = cr.two_density(0)
    rgb = np.random.default_rng(1).uniform(0, 1, xyz.shape).astype(np.float32)
    a, b, c = densify._apply_point_cap(xyz, rgb, err, 500, 3)
    keep = np.random.default_rng(3).choice(xyz.shape[0], size=500, replace=False)
    assert a.tobytes() == xyz[keep].tobytes() and b.tobytes() == rgb[keep].tobytes() and c.tobytes() == err[keep].tobytes()
    want = cr.cap_ref(xyz, err, 500)[0]
    for kw in (dict(cap_mode="spatial"), dict(cap_mode="spatial", host_threads=2)):
        a, b, c = densify._apply_point_cap(xyz, rgb, err, 500, 3, **kw)
        assert a.tobytes() == xyz[want].tobytes() and b.tobytes() == rgb[want].tobytes() and c.tobytes() == err[want].tobytes()
    assert densify._apply_point_cap(xyz, rgb, err, 0, 3, "spatial")[0] is xyz and densify._apply_point_cap(xyz, rgb, err, 10 ** 6, 3, "spatial")[0] is xyz


@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_random_is_the_run_without_the_key(scene, tmp_path, monkeypatch, mode):
    def never(*a, **kw):
        raise AssertionError("the spatial cap ran in random mode")
    monkeypatch.setattr(hb.HostDensifier, "cap_spatial", never)
    out = lambda name: os.path.join(str(tmp_path), name)                       # noqa: E731
    for exp in (dict(), NORMALS):
        assert tf.gui_run(scene, out("plain.ply"), mode, exp, max_points=M)[0] == 0
        assert tf.gui_run(scene, out("random.ply"), mode, {**exp, "cap_mode": "random"}, max_points=M)[0] == 0
        assert open(out("plain.ply"), "rb").read() == open(out("random.ply"), "rb").read() and rows(out("plain.ply")).shape[0] == M
    rc, plain = tf.cli_run(scene, f"plain_{mode}.ply", mode, ["--max_points", str(M)])
    rc2, rnd = tf.cli_run(scene, f"random_{mode}.ply", mode, ["--max_points", str(M), "--cap_mode", "random"])
    assert rc == 0 == rc2 and open(plain, "rb").read() == open(rnd, "rb").read()


@pytest.mark.parametrize("exp", [dict(), NORMALS], ids=["15-byte", "27-byte"])
@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_both_entry_points_keep_the_reference_rows_of_the_uncapped_file(scene, tmp_path, monkeypatch, mode, exp):
    out = lambda name: os.path.join(str(tmp_path), name)                       # noqa: E731
    flags = ["--estimate_normals"] if exp else []
    assert tf.gui_run(scene, out("all.ply"), mode, exp)[0] == 0
    rc, cli_all = tf.cli_run(scene, f"all_{mode}_{len(exp)}.ply", mode, flags)
    assert rc == 0
    spy = Spy(monkeypatch)
    msgs, lines = [], []
    monkeypatch.setattr(densify.log, "info", lambda text: lines.append(text))
    assert tf.gui_run(scene, out("cap.ply"), mode, {**exp, **SPATIAL}, msgs, max_points=M) == (0, out("cap.ply"))
    assert len(spy.calls) == 1
    uncapped, capped = rows(out("all.ply")), rows(out("cap.ply"))
    assert uncapped.shape[0] > M and capped.dtype.itemsize == (27 if exp else 15)
    check_against_uncapped(spy.calls[0], capped, uncapped)
    lev, cells, _above, _side = spy.calls[0]["stats"]
    line = [t for t in lines if t.startswith("Spatial cap")]
    assert line == [f"Spatial cap: {uncapped.shape[0]:,} points in, {M:,} kept, level {lev}, {cells:,} cells"]
    print(line[0])
    assert [t for _, t in msgs].count("Choosing points (spatial cap)...") == 1
    # the random cap of the same run permutes and picks other rows
    assert tf.gui_run(scene, out("rnd.ply"), mode, exp, max_points=M)[0] == 0
    assert rows(out("rnd.ply")).tobytes() != capped.tobytes()
    # the CLI entry point
    spy.calls.clear()
    msgs = []
    rc, cli_cap = tf.cli_run(scene, f"cap_{mode}_{len(exp)}.ply", mode, flags + ["--max_points", str(M), "--cap_mode", "spatial"], msgs)
    assert rc == 0 and len(spy.calls) == 1 and any(t == "Choosing points (spatial cap)..." for _, t in msgs)
    check_against_uncapped(spy.calls[0], rows(cli_cap), rows(cli_all))


def test_a_cap_that_does_not_act_runs_nothing(scene, tmp_path, monkeypatch):
    out = lambda name: os.path.join(str(tmp_path), name)                       # noqa: E731
    assert tf.gui_run(scene, out("all.ply"), "sampled", dict())[0] == 0
    n = rows(out("all.ply")).shape[0]
    spy = Spy(monkeypatch)
    assert tf.gui_run(scene, out("wide.ply"), "sampled", SPATIAL, max_points=n)[0] == 0
    assert spy.calls == [] and open(out("wide.ply"), "rb").read() == open(out("all.ply"), "rb").read()


@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_the_stages_behind_the_cap_see_the_spatially_capped_cloud(scene, tmp_path, monkeypatch, mode):
    out = lambda name: os.path.join(str(tmp_path), name)                       # noqa: E731
    assert tf.gui_run(scene, out("all.ply"), mode, NORMALS)[0] == 0
    uncapped = rows(out("all.ply"))
    spy = Spy(monkeypatch)
    # oriented fusion
    fuse = tf.Spy(monkeypatch)
    assert tf.gui_run(scene, out("fuse.ply"), mode, {**NORMALS, **SPATIAL, "fuse_voxel_size": tf.H}, max_points=M)[0] == 0
    keep = spy.calls[-1]["keep"]
    assert keep.tolist() == cr.cap_ref(spy.calls[-1]["xyz"], spy.calls[-1]["err"], M)[0].tolist()
    assert len(fuse.calls) == 1 and fuse.calls[0]["xyz"].tobytes() == uncapped["xyz"][keep].tobytes()
    assert fuse.calls[0]["normals"].tobytes() == uncapped["normal"][keep].tobytes()
    assert open(out("fuse.ply"), "rb").read() == tf.expected_file(fuse.calls[0], out("fuse_want.ply"))
    rc, cli = tf.cli_run(scene, f"fuse_{mode}.ply", mode, ["--estimate_normals", "--fuse_voxel_size", str(tf.H), "--max_points", str(M), "--cap_mode", "spatial"])
    cli_call = spy.calls[-1]                                               # (the CLI plans its own references: another cloud, the same rule)
    assert rc == 0 and cli_call["keep"].tolist() == cr.cap_ref(cli_call["xyz"], cli_call["err"], M)[0].tolist()
    assert len(fuse.calls) == 2 and fuse.calls[1]["xyz"].tobytes() == cli_call["xyz"][cli_call["keep"]].tobytes()
    assert open(cli, "rb").read() == tf.expected_file(fuse.calls[1], out("fuse_want_cli.ply"))
    # Gaussian-ready output: the 68-byte records of the kept points, in the uncapped file's order
    assert tf.gui_run(scene, out("gauss.ply"), mode, {**NORMALS, **SPATIAL, "gaussian_init": True}, max_points=M)[0] == 0
    body = open(out("gauss.ply"), "rb").read().split(b"end_header\n", 1)[1]
    g = np.frombuffer(body, dtype="<f4").reshape(-1, 17)
    assert g.shape[0] == M and g[:, :3].tobytes() == uncapped["xyz"][keep].tobytes() and g[:, 3:6].tobytes() == uncapped["normal"][keep].tobytes()
    # behind the consensus filter: the cap sees the filtered cloud
    radius = 0.02 if mode == "sampled" else 0.005
    cons = {"min_consensus_refs": 1, "consensus_radius": radius}
    assert tf.gui_run(scene, out("cons_all.ply"), mode, {**NORMALS, **cons})[0] == 0
    assert tf.gui_run(scene, out("cons_cap.ply"), mode, {**NORMALS, **cons, **SPATIAL}, max_points=M)[0] == 0
    filtered = rows(out("cons_all.ply"))
    assert M < filtered.shape[0] < uncapped.shape[0]
    check_against_uncapped(spy.calls[-1], rows(out("cons_cap.ply")), filtered)


def test_the_voxel_filter_sees_the_spatially_capped_cloud(scene, tmp_path, monkeypatch):
    out = lambda name: os.path.join(str(tmp_path), name)                       # noqa: E731
    assert tf.gui_run(scene, out("all.ply"), "sampled", dict())[0] == 0
    uncapped = rows(out("all.ply"))
    spy = Spy(monkeypatch)
    seen = []
    plain = densify._voxel_downsample
    monkeypatch.setattr(densify, "_voxel_downsample", lambda xyz, rgb, h: (seen.append(np.array(xyz)), plain(xyz, rgb, h))[1])
    assert tf.gui_run(scene, out("vox.ply"), "sampled", SPATIAL, max_points=M, voxel_size=0.05)[0] == 0
    keep = spy.calls[0]["keep"]
    assert len(spy.calls) == 1 and len(seen) == 1 and seen[0].tobytes() == uncapped["xyz"][keep].tobytes()
    assert 0 < rows(out("vox.ply")).shape[0] < M


def test_a_data_refusal_names_the_knob(scene, tmp_path, monkeypatch):
    def refuse(dens, *a, **kw):
        raise hb.CapInputRefused("lfd_cap_spatial_host refused its input (1): lfd_cap_spatial_host: non-finite coordinate in the input")
    monkeypatch.setattr(hb.HostDensifier, "cap_spatial", refuse)
    target = os.path.join(str(tmp_path), "refused.ply")
    code, text = tf.gui_run(scene, target, "sampled", SPATIAL, max_points=M)
    assert code == 1 and "experimental['cap_mode'] = 'spatial' cannot be applied" in text and "non-finite coordinate" in text
    assert not os.path.exists(target)
    code, text = tf.gui_run(scene, target, "sampled", SPATIAL, max_points=M, voxel_size=0.05)
    assert code == 1 and "experimental['cap_mode'] = 'spatial'" in text
    with pytest.raises(RuntimeError, match=r"experimental\['cap_mode'\] = 'spatial' cannot be applied"):
        tf.cli_run(scene, "refused_cli.ply", "sampled", ["--max_points", str(M), "--cap_mode", "spatial"])
