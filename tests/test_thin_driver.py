"""The footprint-adaptive thinning in the driver, on the host backend with the analytic matcher (core/types.py, densify.py, core/pipeline.py), on
the generated scene of tests/test_fuse_driver.py: the knob, its refusals, the sharded refusal and the CLI flag; off is the run without the key, byte
for byte; on, the file is the knob-off file under the mask that the reference of tests/thin_ref.py computes for the knob-off cloud - through both
entry points, in both modes, with and without normals -, from rows the test derives itself from the cameras and the matcher's grid; max_points in
both cap modes, the oriented fusion and the Gaussian output run behind it on the thinned cloud; the counts per reference add up to the file."""
import os

import numpy as np
import pytest

import lichtfeld_densification_plugin_amd as lfd
import test_fuse_driver as tf
import thin_ref as tr
from lichtfeld_densification_plugin_amd import densify
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from lichtfeld_densification_plugin_amd.core.types import EXPERIMENTAL_DEFAULTS

REC15 = np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)])
NORMALS = {"estimate_normals": True}
CELLS = 2.0
ON = {"footprint_thin_cells": CELLS}
M = 300


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    return tf.cycle_scene.make_scene(str(tmp_path_factory.mktemp("thin_scene")), n_cams=4)


def rows(path):
    """the vertices of a PLY, 15-byte or 27-byte ones"""
    head, body = open(path, "rb").read().split(b"end_header\n", 1)
    rec = np.frombuffer(body, dtype=tf.REC27 if b"property float nx" in head else REC15)
    assert f"element vertex {rec.shape[0]}\n".encode() in head
    return rec


class Spy:
    """Every thin_footprint call of a run on the host backend - what went in and what came out -, the (cameras, references, grid) its rows were
    made from and the result the stage handed on."""

    def __init__(self, monkeypatch):
        self.calls, self.made, self.results = [], [], []
        plain, plain_rows, plain_stage = hb.HostDensifier.thin_footprint, densify.footprint_rows, densify._apply_footprint_thin
        spy = self

        def thin(dens, xyz, err, counts, ref_rows, thin_cells):
            keep, kept = plain(dens, xyz, err, counts, ref_rows, thin_cells)
            spy.calls.append(dict(xyz=xyz.numpy().copy(), err=err.numpy().copy(), counts=np.array(counts), rows=np.array(ref_rows), cells=thin_cells,
                                  keep=keep.numpy().copy(), kept=np.array(kept), stats=dens.thin_stats))
            return keep, kept

        def make(records, refs_local, grid):
            spy.made.append((records, list(refs_local), tuple(grid)))
            return plain_rows(records, refs_local, grid)

        def stage(result, *a, **kw):
            out = plain_stage(result, *a, **kw)
            spy.results.append(out)
            return out
        monkeypatch.setattr(hb.HostDensifier, "thin_footprint", thin)
        monkeypatch.setattr(densify, "footprint_rows", make)
        monkeypatch.setattr(densify, "_apply_footprint_thin", stage)


def own_rows(records, refs_local, grid):
    """the five values per reference, from the issue's words: the third row of [R | t], max(w / (fx W), h / (fy H)) in f64"""
    out = []
    for r in refs_local:
        c = records[r]
        K, R, t = np.asarray(c.K, np.float64), np.asarray(c.R, np.float64), np.asarray(c.t, np.float64).reshape(3)
        out.append([R[2, 0], R[2, 1], R[2, 2], t[2], max(c.width / (K[0, 0] * grid[1]), c.height / (K[1, 1] * grid[0]))])
    return np.asarray(out, np.float64)


def check_against_off(spy, thinned, off):
    """The one call of a run saw the knob-off cloud and the rows of its references, chose what the reference chooses, and the file holds those
    rows of the knob-off file in that file's order; the counts handed on add up to the file."""
    assert len(spy.calls) == 1 and len(spy.made) == 1
    call = spy.calls[0]
    assert call["cells"] == CELLS and call["xyz"].tobytes() == np.ascontiguousarray(off["xyz"]).tobytes()
    assert call["rows"].tobytes() == own_rows(*spy.made[0]).tobytes() and call["rows"].shape == (call["counts"].size, 5)
    want, want_kept, want_stats = tr.thin_ref(call["xyz"], call["err"], call["counts"], call["rows"], CELLS)
    assert call["keep"].tolist() == want.tolist() and call["kept"].tolist() == want_kept.tolist()
    assert call["stats"][0].tolist() == want_stats[0].tolist() and call["stats"][1].tolist() == want_stats[1].tolist()
    assert 0 < want.size < off.shape[0]
    assert thinned.tobytes() == off[want].tobytes()                      # every column: the normals follow
    result = spy.results[-1]
    assert int(np.sum(result.points_per_reference)) == thinned.shape[0] == result.n_points
    return want


def test_the_knob_is_experimental_off_by_default_and_validated():
    assert EXPERIMENTAL_DEFAULTS["footprint_thin_cells"] == 0.0
    cfg = lfd.DensePipelineConfig(output_path="a.bin")
    assert cfg.exp("footprint_thin_cells") == 0.0 and cfg.problem() is None
    for mode in ("sampled", "dense"):
        for backend in ("device", "host"):
            for kw, exp in ((dict(), ON), (dict(), {"footprint_thin_cells": 1}), (dict(), {"footprint_thin_cells": np.float32(0.5)}),
                            (dict(max_points=10), ON), (dict(max_points=10), {**ON, "cap_mode": "spatial"}), (dict(voxel_size=0.1), ON),
                            (dict(), {**ON, **NORMALS, "fuse_voxel_size": 0.05}), (dict(), {**ON, **NORMALS, "gaussian_init": True}),
                            (dict(), {**ON, "min_freespace_violations": 1}), (dict(stream_output=True), {"footprint_thin_cells": 0.0})):
                assert lfd.DensePipelineConfig(output_path="a.ply", triangulation_mode=mode, backend=backend, experimental=exp, **kw).problem() is None
    number = r"footprint_thin_cells'\] must be a finite number >= 0"
    refused = [
        (dict(), {"footprint_thin_cells": -0.5}, number), (dict(), {"footprint_thin_cells": float("nan")}, number),
        (dict(), {"footprint_thin_cells": float("inf")}, number), (dict(), {"footprint_thin_cells": "2"}, number),
        (dict(), {"footprint_thin_cells": None}, number), (dict(), {"footprint_thin_cells": True}, number),
        (dict(stream_output=True), ON, r"footprint_thin_cells'\] has to see the whole cloud before anything is written; stream_output"),
        (dict(triangulation_mode="dense"), {**ON, "dense_tile_segments": True}, r"footprint_thin_cells'\] needs the cloud as arrays with per-reference counts"),
        (dict(), {**ON, "exchange_records": "ply"}, r"footprint_thin_cells'\] thins f32 rows; experimental\['exchange_records'\] must be 'f32'"),
    ]
    for kw, exp, text in refused:
        with pytest.raises(ValueError, match=text):
            lfd.DensePipelineConfig(**{"output_path": "a.ply", **kw}, experimental=exp)


def test_the_cli_flag_reaches_the_configuration():
    ap = densify.build_argparser()
    assert densify._experimental_from_args(ap.parse_args(["--scene_root", "x", "--footprint_thin_cells", "1.5"])) == {"footprint_thin_cells": 1.5}
    assert densify._experimental_from_args(ap.parse_args(["--scene_root", "x"])) == {}
    assert densify._experimental_from_args(ap.parse_args(["--scene_root", "x", "--footprint_thin_cells", "0"])) == {}
    with pytest.raises(ValueError, match="must be a finite number >= 0"):
        lfd.DensePipelineConfig(output_path="a.ply", experimental=densify._experimental_from_args(ap.parse_args(["--scene_root", "x", "--footprint_thin_cells", "-1"])))


def test_a_sharded_run_is_refused_by_name(scene, tmp_path, monkeypatch):
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    monkeypatch.setattr(dist, "get_rank", lambda *a: 0)
    cfg = lfd.DensePipelineConfig(output_path=os.path.join(str(tmp_path), "sharded.ply"), backend="host", experimental=ON)
    recs = densify.extract_cameras_from_lfs([tf.Node(c) for c in scene["cams"]])
    with pytest.raises(ValueError, match=r"footprint_thin_cells'\] cannot run sharded over several GPUs"):
        densify.run_dense_pipeline(recs, [0, 1], [[1], [0], [0], [0]], cfg)


def test_a_result_without_a_match_grid_is_refused_by_name():
    from lichtfeld_densification_plugin_amd.core.sinks import PipelineResult
    z = np.zeros((4, 3), np.float32)
    result = PipelineResult(xyz=z, rgb=z, err=np.zeros(4, np.float32), elapsed_seconds=0.0, pairs_processed=0, pairs_matched=0, points_per_reference=[4])
    cfg = lfd.DensePipelineConfig(output_path="a.ply", backend="host", experimental=ON)
    with pytest.raises(RuntimeError, match=r"footprint_thin_cells'\] sizes its cells by the matcher's grid"):
        densify._apply_footprint_thin(result, cfg, [], [0])
    off = lfd.DensePipelineConfig(output_path="a.ply", backend="host")
    assert densify._apply_footprint_thin(result, off, [], [0]) is result


@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_off_is_the_run_without_the_key(scene, tmp_path, monkeypatch, mode):
    def never(*a, **kw):
        raise AssertionError("the thinning ran with the knob off")
    monkeypatch.setattr(hb.HostDensifier, "thin_footprint", never)
    monkeypatch.setattr(densify, "footprint_rows", never)
    out = lambda name: os.path.join(str(tmp_path), name)                       # noqa: E731
    for exp in (dict(), NORMALS):
        assert tf.gui_run(scene, out("plain.ply"), mode, exp)[0] == 0
        assert tf.gui_run(scene, out("zero.ply"), mode, {**exp, "footprint_thin_cells": 0.0})[0] == 0
        assert open(out("plain.ply"), "rb").read() == open(out("zero.ply"), "rb").read()
    rc, plain = tf.cli_run(scene, f"plain_{mode}.ply", mode, [])
    rc2, zero = tf.cli_run(scene, f"zero_{mode}.ply", mode, ["--footprint_thin_cells", "0"])
    assert rc == 0 == rc2 and open(plain, "rb").read() == open(zero, "rb").read()


@pytest.mark.parametrize("exp", [dict(), NORMALS], ids=["15-byte", "27-byte"])
@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_both_entry_points_write_the_knob_off_cloud_under_the_reference_s_mask(scene, tmp_path, monkeypatch, mode, exp):
    out = lambda name: os.path.join(str(tmp_path), name)                       # noqa: E731
    flags = ["--estimate_normals"] if exp else []
    assert tf.gui_run(scene, out("off.ply"), mode, exp)[0] == 0
    rc, cli_off = tf.cli_run(scene, f"off_{mode}_{len(exp)}.ply", mode, flags)
    assert rc == 0
    spy = Spy(monkeypatch)
    msgs, lines = [], []
    monkeypatch.setattr(densify.log, "info", lambda text: lines.append(text))
    assert tf.gui_run(scene, out("on.ply"), mode, {**exp, **ON}, msgs) == (0, out("on.ply"))
    off, on = rows(out("off.ply")), rows(out("on.ply"))
    assert on.dtype.itemsize == (27 if exp else 15)
    want = check_against_off(spy, on, off)
    line = [t for t in lines if t.startswith("Footprint thinning")]
    assert len(line) == 1 and line[0].startswith(f"Footprint thinning (2 cells): {off.shape[0]:,} points in, {want.size:,} kept; level ")
    points, cells = spy.calls[0]["stats"][:2]
    for l in np.flatnonzero(points):
        assert f"level {l}: {int(points[l]):,} points in {int(cells[l]):,} cells" in line[0]
    print(line[0])
    assert [t for _, t in msgs].count("Thinning by camera footprint...") == 1
    # the CLI entry point plans its own references: another cloud, the same rule
    spy.calls.clear(), spy.made.clear()
    rc, cli_on = tf.cli_run(scene, f"on_{mode}_{len(exp)}.ply", mode, flags + ["--footprint_thin_cells", "2"])
    assert rc == 0
    check_against_off(spy, rows(cli_on), rows(cli_off))


@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_the_stages_behind_it_see_the_thinned_cloud(scene, tmp_path, monkeypatch, mode):
    out = lambda name: os.path.join(str(tmp_path), name)                       # noqa: E731
    spy = Spy(monkeypatch)
    assert tf.gui_run(scene, out("thin.ply"), mode, {**NORMALS, **ON})[0] == 0
    thinned = rows(out("thin.ply"))
    assert thinned.shape[0] > M
    # max_points, upstream's draw: the rows its generator picks of the thinned cloud, in the draw's order
    assert tf.gui_run(scene, out("random.ply"), mode, {**NORMALS, **ON}, max_points=M)[0] == 0
    draw = np.random.default_rng(3).choice(thinned.shape[0], size=M, replace=False)
    assert rows(out("random.ply")).tobytes() == thinned[draw].tobytes()
    # max_points, the spatial cap: it is handed the thinned cloud
    caps = []
    plain_cap = hb.HostDensifier.cap_spatial
    monkeypatch.setattr(hb.HostDensifier, "cap_spatial", lambda d, xyz, err, m: (caps.append(xyz.numpy().copy()), plain_cap(d, xyz, err, m))[1])
    assert tf.gui_run(scene, out("spatial.ply"), mode, {**NORMALS, **ON, "cap_mode": "spatial"}, max_points=M)[0] == 0
    assert len(caps) == 1 and caps[0].tobytes() == np.ascontiguousarray(thinned["xyz"]).tobytes() and rows(out("spatial.ply")).shape[0] == M
    # oriented fusion
    fuse = tf.Spy(monkeypatch)
    assert tf.gui_run(scene, out("fuse.ply"), mode, {**NORMALS, **ON, "fuse_voxel_size": tf.H})[0] == 0
    assert len(fuse.calls) == 1 and fuse.calls[0]["xyz"].tobytes() == np.ascontiguousarray(thinned["xyz"]).tobytes()
    assert fuse.calls[0]["normals"].tobytes() == np.ascontiguousarray(thinned["normal"]).tobytes()
    assert open(out("fuse.ply"), "rb").read() == tf.expected_file(fuse.calls[0], out("fuse_want.ply"))
    # Gaussian-ready output: the 68-byte records of the thinned points, in their order
    assert tf.gui_run(scene, out("gauss.ply"), mode, {**NORMALS, **ON, "gaussian_init": True})[0] == 0
    g = np.frombuffer(open(out("gauss.ply"), "rb").read().split(b"end_header\n", 1)[1], dtype="<f4").reshape(-1, 17)
    assert g[:, :3].tobytes() == np.ascontiguousarray(thinned["xyz"]).tobytes() and g[:, 3:6].tobytes() == np.ascontiguousarray(thinned["normal"]).tobytes()
    # the CLI entry point with a cap behind the thinning
    rc, cli = tf.cli_run(scene, f"cap_{mode}.ply", mode, ["--footprint_thin_cells", "2", "--max_points", str(M)])
    assert rc == 0 and rows(cli).shape[0] == M


def test_the_voxel_filter_sees_the_thinned_cloud(scene, tmp_path, monkeypatch):
    out = lambda name: os.path.join(str(tmp_path), name)                       # noqa: E731
    assert tf.gui_run(scene, out("thin.ply"), "sampled", ON)[0] == 0
    thinned = rows(out("thin.ply"))
    seen = []
    plain = densify._voxel_downsample
    monkeypatch.setattr(densify, "_voxel_downsample", lambda xyz, rgb, h: (seen.append(np.array(xyz)), plain(xyz, rgb, h))[1])
    assert tf.gui_run(scene, out("vox.ply"), "sampled", ON, voxel_size=0.05)[0] == 0
    assert len(seen) == 1 and seen[0].tobytes() == np.ascontiguousarray(thinned["xyz"]).tobytes()
    assert 0 < rows(out("vox.ply")).shape[0] < thinned.shape[0]


def test_a_data_refusal_names_the_knob(scene, tmp_path, monkeypatch):
    def refuse(dens, *a, **kw):
        raise hb.ThinInputRefused("lfd_thin_footprint_host refused its input (1): lfd_thin_footprint_host: non-finite coordinate in the input")
    monkeypatch.setattr(hb.HostDensifier, "thin_footprint", refuse)
    target = os.path.join(str(tmp_path), "refused.ply")
    code, text = tf.gui_run(scene, target, "sampled", ON)
    assert code == 1 and "experimental['footprint_thin_cells']" in text and "non-finite coordinate" in text and not os.path.exists(target)
    with pytest.raises(RuntimeError, match=r"experimental\['footprint_thin_cells'\]: .*non-finite coordinate"):
        tf.cli_run(scene, "refused_cli.ply", "sampled", ["--footprint_thin_cells", "2"])
