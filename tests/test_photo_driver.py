"""The photo-consistency gate in the driver, on the host backend with the analytic matcher (core/types.py, core/hotpath.py, core/pipeline.py,
densify.py): the knobs, their refusals and the CLI flags; with the knobs at their defaults no new code runs; in sampled and in dense mode the
knob-on cloud is the knob-off cloud under the mask tests/photo_ref.py gives for the points that reached the gate - same order, same bits, the
sampling stream where it was -; the gate sits behind the support filter, the re-triangulation and the depth-uncertainty gate and in front of
the multi-view colour, the gain statistics and the normals; the log line carries the five counts; a sharded run is refused when it starts."""
import contextlib
import logging
import os

import numpy as np
import pytest

import cycle_scene
import lichtfeld_densification_plugin_amd as lfd
import photo_ref
from lichtfeld_densification_plugin_amd import densify
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from lichtfeld_densification_plugin_amd.core import pipeline as pl
from lichtfeld_densification_plugin_amd.core.types import EXPERIMENTAL_DEFAULTS

bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
ON = {"min_photo_ncc": 0.8}


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    return cycle_scene.make_scene(str(tmp_path_factory.mktemp("photo_scene")), n_cams=4)      # three references, each with the three other cameras


@contextlib.contextmanager
def recorded_gates():
    """Every photo_gate call of a run, in order: the points that went in, the twin's status and ncc, the reference's verdicts for the same
    points from the batch the call was given, and the arguments.  Calls of the stages around it are noted in ``order``."""
    seen, order = [], []
    names = ("support_filter", "refine_multiview", "depth_sigma_filter", "colour_multiview", "gain_accumulate", "estimate_normals")
    plain = {n: getattr(hb.HostDensifier, n) for n in names + ("photo_gate",)}

    def gate(self, batch, out, window_cells, min_ncc, min_texture, with_status=False, with_ncc=False, counters=None, into=None):
        order.append("photo_gate")
        assert isinstance(out, hb.TriangulationOutput) and batch.nbr_images is not None
        res, status, ncc = plain["photo_gate"](self, batch, out, window_cells, min_ncc, min_texture, with_status=True, with_ncc=True,
                                               counters=counters, into=into)
        want, kept, want_ncc = photo_ref.batch_reference(batch.refs, int(batch.c.w_match), int(batch.c.h_match), out, window_cells, min_ncc, min_texture,
                                                         axes=[a.numpy() for a in batch.axes] if batch.axes is not None else None)
        seen.append(dict(xyz_in=out.xyz.numpy().copy(), rgb_in=out.rgb.numpy().copy(), err_in=out.err.numpy().copy(), status=status.numpy().copy(),
                         ncc=ncc.numpy().copy(), want=want, kept=kept, R=int(window_cells), min_ncc=float(min_ncc), tex=float(min_texture),
                         n_out=int(res.count)))
        extra = ((status,) if with_status else ()) + ((ncc,) if with_ncc else ())
        return (res,) + extra if extra else res

    def noted(name):
        def call(self, *a, **kw):
            order.append(name)
            return plain[name](self, *a, **kw)
        return call

    hb.HostDensifier.photo_gate = gate
    for n in names:
        setattr(hb.HostDensifier, n, noted(n))
    try:
        yield seen, order
    finally:
        for n, f in plain.items():
            setattr(hb.HostDensifier, n, f)


def joined(seen, name):
    return np.concatenate([s[name] for s in seen])


_thresholds = {}


def median_ncc(scene, mode, extra):
    """A threshold that refutes about half of the judged points: the median ZNCC of a run whose gate refutes next to nothing."""
    key = (mode, tuple(sorted(extra.items())))
    if key not in _thresholds:
        with recorded_gates() as (seen, _order):
            cycle_scene.run(scene, cycle_scene.matcher_for(scene), "probe.ply", triangulation_mode=mode, experimental={"min_photo_ncc": 1e-6, **extra})
        v = joined(seen, "ncc")
        _thresholds[key] = float(np.clip(np.median(v[np.isfinite(v) & (v > 0)]), 1e-3, 1.0))
    return _thresholds[key]


def test_the_knobs_are_experimental_off_by_default_and_validated():
    assert EXPERIMENTAL_DEFAULTS["min_photo_ncc"] == 0.0 and EXPERIMENTAL_DEFAULTS["photo_window_cells"] == 2
    assert EXPERIMENTAL_DEFAULTS["photo_min_texture"] == 2.0
    cfg = lfd.DensePipelineConfig(output_path="a.ply")
    assert cfg.exp("min_photo_ncc") == 0.0 and cfg.problem() is None
    for mode in ("sampled", "dense"):
        for backend in ("device", "host"):
            for extra in ({}, {"photo_window_cells": 1}, {"photo_window_cells": 3, "photo_min_texture": 0.0}, {"min_photo_ncc": 1.0},
                          {"min_support_views": 1, "multiview_refine": True, "max_depth_sigma_rel": 0.05, "match_sigma_px": 0.5},
                          {"multiview_colour": "median"}, {"gain_compensation": "luma"}, {"estimate_normals": True}, {"cycle_thresh_px": 1.0}):
                assert lfd.DensePipelineConfig(output_path="a.ply", triangulation_mode=mode, backend=backend, experimental={**ON, **extra}).problem() is None
    assert lfd.DensePipelineConfig(output_path="a.ply", nns_per_ref=1, experimental=ON).problem() is None       # the case the gate exists for
    refused = [
        (dict(), {"min_photo_ncc": -0.1}, r"min_photo_ncc'\] must be 0 \(off\) or in \(0, 1\]"),
        (dict(), {"min_photo_ncc": 1.01}, r"min_photo_ncc'\] must be 0 \(off\) or in \(0, 1\]"),
        (dict(), {"min_photo_ncc": float("nan")}, r"min_photo_ncc'\] must be 0 \(off\) or in \(0, 1\]"),
        (dict(), {"min_photo_ncc": float("inf")}, r"min_photo_ncc'\] must be 0 \(off\) or in \(0, 1\]"),
        (dict(), {"min_photo_ncc": "high"}, r"min_photo_ncc'\] must be a number"),
        (dict(), {"min_photo_ncc": None}, r"min_photo_ncc'\] must be a number"),
        (dict(), {**ON, "photo_window_cells": 0}, r"photo_window_cells'\] must be an integer in 1 \.\. 3"),
        (dict(), {**ON, "photo_window_cells": 4}, r"photo_window_cells'\] must be an integer in 1 \.\. 3"),
        (dict(), {**ON, "photo_window_cells": 2.0}, r"photo_window_cells'\] must be an integer in 1 \.\. 3"),
        (dict(), {**ON, "photo_window_cells": True}, r"photo_window_cells'\] must be an integer in 1 \.\. 3"),
        (dict(), {**ON, "photo_min_texture": -1.0}, r"photo_min_texture'\] must be finite and >= 0"),
        (dict(), {**ON, "photo_min_texture": float("inf")}, r"photo_min_texture'\] must be finite and >= 0"),
        (dict(), {**ON, "photo_min_texture": float("nan")}, r"photo_min_texture'\] must be finite and >= 0"),
        (dict(), {**ON, "photo_min_texture": "flat"}, r"photo_min_texture'\] must be a number"),
        (dict(), {"photo_window_cells": 3}, r"photo_window_cells'\] is the window of the photo-consistency gate: it needs experimental\['min_photo_ncc'\] > 0"),
        (dict(), {"photo_min_texture": 1.0}, r"photo_min_texture'\] is the texture floor of the photo-consistency gate: it needs experimental\['min_photo_ncc'\] > 0"),
        (dict(), {"photo_min_texture": 1.0, "min_photo_ncc": 0.0}, r"it needs experimental\['min_photo_ncc'\] > 0"),
        (dict(no_filter=True, nns_per_ref=1), ON, r"min_photo_ncc'\] is a filter: it cannot run with no_filter"),
        (dict(stream_output=True), ON, r"min_photo_ncc'\] filters points held as arrays .* stream_output"),
        (dict(triangulation_mode="dense", stream_output=True), ON, r"min_photo_ncc'\] filters points held as arrays .* stream_output"),
        (dict(triangulation_mode="dense"), {**ON, "dense_tile_segments": True}, r"min_photo_ncc'\] needs the ordered dense result"),
        (dict(), {**ON, "exchange_records": "ply"}, r"min_photo_ncc'\] filters f32 rows; experimental\['exchange_records'\] must be 'f32'"),
    ]
    for kw, exp, text in refused:
        with pytest.raises(ValueError, match=text):
            lfd.DensePipelineConfig(**{"output_path": "a.ply", **kw}, experimental=exp)
    for kw in (dict(stream_output=True), dict(no_filter=True, nns_per_ref=1), dict(experimental={"exchange_records": "ply"})):   # off: no route is refused
        exp = {**kw.pop("experimental", {}), "min_photo_ncc": 0.0, "photo_window_cells": 2, "photo_min_texture": 2.0}
        assert lfd.DensePipelineConfig(output_path="a.ply", experimental=exp, **kw).problem() is None


def test_the_cli_flags_reach_the_configuration():
    ap = densify.build_argparser()
    args = ap.parse_args(["--scene_root", "x", "--min_photo_ncc", "0.8", "--photo_window_cells", "3", "--photo_min_texture", "1.5"])
    assert densify._experimental_from_args(args) == {"min_photo_ncc": 0.8, "photo_window_cells": 3, "photo_min_texture": 1.5}
    assert densify._experimental_from_args(ap.parse_args(["--scene_root", "x", "--min_photo_ncc", "0.7"])) == {"min_photo_ncc": 0.7}
    assert densify._experimental_from_args(ap.parse_args(["--scene_root", "x"])) == {}
    cfg = lfd.DensePipelineConfig(output_path="a.ply", experimental=densify._experimental_from_args(args))
    assert cfg.exp("min_photo_ncc") == 0.8 and cfg.exp("photo_window_cells") == 3 and cfg.exp("photo_min_texture") == 1.5
    with pytest.raises(ValueError, match="photo_window_cells"):
        lfd.DensePipelineConfig(output_path="a.ply", experimental=densify._experimental_from_args(
            ap.parse_args(["--scene_root", "x", "--photo_window_cells", "1"])))


def test_a_sharded_run_is_refused_when_it_starts(scene, monkeypatch):
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    monkeypatch.setattr(dist, "get_rank", lambda *a: 0)
    cfg = lfd.DensePipelineConfig(output_path=os.path.join(scene["root"], "sharded.ply"), nns_per_ref=3, backend="host", experimental=ON)
    with pytest.raises(ValueError, match="min_photo_ncc'\\] cannot run sharded"):
        pl.run_dense_pipeline(scene["cams"], scene["refs"], scene["nn"], cfg, matcher=cycle_scene.matcher_for(scene))


def test_with_the_knobs_at_their_defaults_no_new_code_runs(scene, monkeypatch):
    def never(*a, **kw):
        raise AssertionError("the photo-consistency gate ran with the knob off")
    monkeypatch.setattr(hb.HostDensifier, "photo_gate", never)
    seen_inputs = []
    plain = hb.PreparedBatch.__init__

    def init(self, refs, *a, **kw):
        seen_inputs.extend(refs)
        plain(self, refs, *a, **kw)
    monkeypatch.setattr(hb.PreparedBatch, "__init__", init)
    a = cycle_scene.run(scene, cycle_scene.matcher_for(scene), "never.ply")
    b = cycle_scene.run(scene, cycle_scene.matcher_for(scene), "off.ply", experimental={"min_photo_ncc": 0.0, "photo_window_cells": 2,
                                                                                        "photo_min_texture": 2.0})
    assert cycle_scene.same_cloud(a, b) and a.xyz.shape[0] > 1000
    assert seen_inputs and all(r.nbr_images is None for r in seen_inputs)                  # and no neighbour image travels


@pytest.mark.parametrize("mode,group", [("sampled", 1), ("dense", 1), ("dense", 2)])
def test_the_cloud_is_the_knob_off_cloud_under_the_references_mask(scene, mode, group, caplog):
    t = median_ncc(scene, mode, {})
    with cycle_scene.recorded_cells() as cells_off:
        off = cycle_scene.run(scene, cycle_scene.matcher_for(scene), "off.ply", triangulation_mode=mode, refs_per_launch=group)
    with caplog.at_level(logging.INFO, logger="lfd_densify"), cycle_scene.recorded_cells() as cells_on, recorded_gates() as (seen, order):
        on = cycle_scene.run(scene, cycle_scene.matcher_for(scene), "on.ply", triangulation_mode=mode, refs_per_launch=group,
                             experimental={"min_photo_ncc": t, "photo_window_cells": 1})
    # what reached the gate is the knob-off run's cloud, bit for bit: no count and no draw of the sampling stream changed ...
    for name in ("xyz", "rgb", "err"):
        assert np.array_equal(bits(joined(seen, name + "_in")), bits(getattr(off, name))), name
    assert all(s["R"] == 1 and s["min_ncc"] == t and s["tex"] == 2.0 for s in seen) and set(order) == {"photo_gate"}
    status, want, keep = joined(seen, "status"), joined(seen, "want"), joined(seen, "kept")
    assert np.array_equal(status, want)                                                    # the twin's verdicts are the reference's
    # ... and what the run emits is that cloud under the reference's mask, in order
    assert 0.1 * keep.size < (~keep).sum() < 0.9 * keep.size
    for name in ("xyz", "rgb", "err"):
        assert np.array_equal(bits(getattr(on, name)), bits(getattr(off, name))[keep]), name
    per_ref = np.add.reduceat(keep, np.concatenate([[0], np.cumsum(off.points_per_reference)[:-1]]))
    assert np.array_equal(on.points_per_reference, per_ref)
    assert len(cells_off) == len(scene["refs"]) and len(cells_on) >= len(cells_off)
    lines = [r.getMessage() for r in caplog.records if r.getMessage().startswith("Photo-consistency gate:")]
    c = np.bincount(status, minlength=5)
    assert lines == [f"Photo-consistency gate: ZNCC at least {t:g} over 3 x 3 cells, texture floor 2 grey levels: {c[0]} points guarded, {c[1]} with "
                     f"under half a window, {c[2]} untextured, {c[3]} consistent, {c[4]} refuted and dropped"]


AROUND = {"min_support_views": 1, "multiview_refine": True, "max_depth_sigma_rel": 1e30, "match_sigma_px": 0.5, "multiview_colour": "mean",
          "estimate_normals": True, "normal_radius_cells": 2}


@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_it_sits_between_the_depth_gate_and_the_colour(scene, mode):
    """Behind support filter, re-triangulation and depth-uncertainty gate; in front of the multi-view colour and the normals, which are per
    point: the knob-on cloud is still the knob-off cloud under the mask, normals included."""
    t = median_ncc(scene, mode, AROUND)
    off = cycle_scene.run(scene, cycle_scene.matcher_for(scene), "off.ply", triangulation_mode=mode, experimental=AROUND)
    with recorded_gates() as (seen, order):
        on = cycle_scene.run(scene, cycle_scene.matcher_for(scene), "on.ply", triangulation_mode=mode, experimental={**AROUND, "min_photo_ncc": t})
    per_call = ["support_filter", "refine_multiview", "depth_sigma_filter", "photo_gate", "colour_multiview", "estimate_normals"]
    assert order == per_call * (len(order) // len(per_call)) and seen
    assert all(s["R"] == 2 for s in seen) and np.array_equal(joined(seen, "status"), joined(seen, "want"))
    keep = joined(seen, "kept")
    assert np.array_equal(bits(joined(seen, "xyz_in")), bits(off.xyz)) and 0 < (~keep).sum() < keep.size
    for name in ("xyz", "rgb", "err", "normals"):
        assert np.array_equal(bits(getattr(on, name)), bits(getattr(off, name))[keep]), name


def test_the_gain_statistics_see_only_what_the_gate_kept(scene):
    t = median_ncc(scene, "sampled", {})
    off = cycle_scene.run(scene, cycle_scene.matcher_for(scene), "off.ply", experimental={"gain_compensation": "luma"})
    with recorded_gates() as (seen, order):
        on = cycle_scene.run(scene, cycle_scene.matcher_for(scene), "on.ply", experimental={"gain_compensation": "luma", "min_photo_ncc": t})
    assert order == ["photo_gate", "gain_accumulate"] * (len(order) // 2) and seen
    keep = joined(seen, "kept")
    assert np.array_equal(bits(on.xyz), bits(off.xyz)[keep]) and np.array_equal(bits(on.err), bits(off.err)[keep])
