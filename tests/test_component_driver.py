"""The connected-component filter in the driver, on the host backend with the analytic matcher (core/types.py, densify.py), on the scene of
tests/test_consensus_driver.py: the knobs and their refusals, the CLI flags, and - through both entry points - the file of a knob-on run: the
knob-off cloud under the mask the brute-force reference computes from the knob-off points, same order, same bits; the normals follow; the
components.json is the reference's summary."""
import json
import logging
import os

import numpy as np
import pytest

import component_ref as cr
import lichtfeld_densification_plugin_amd as lfd
from lichtfeld_densification_plugin_amd import densify
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from lichtfeld_densification_plugin_amd.core.types import EXPERIMENTAL_DEFAULTS
from test_consensus_driver import Spy, cli_run, gui_run, scene, written  # noqa: F401  (the fixture: the consensus driver test's scene)
from test_normals_driver import records

# a sample spacing of the 4-camera scene's sampled cloud (6 647 points): at this radius the middle of the surface is one component of some 4 700
# points and the sparse rim falls apart into several hundred small ones
RADIUS, MIN_POINTS = 0.025, 30
ON = {"min_component_points": MIN_POINTS, "component_radius": RADIUS}


def reference(cloud, radius=RADIUS, min_points=MIN_POINTS):
    xyz, _rgb, _err, counts = cloud
    return cr.filter_cloud(xyz, counts, radius, min_points)


def test_the_knobs_are_experimental_off_by_default_and_validated():
    assert EXPERIMENTAL_DEFAULTS["min_component_points"] == 0 and EXPERIMENTAL_DEFAULTS["component_radius"] == 0.0
    cfg = lfd.DensePipelineConfig(output_path="a.ply")
    assert cfg.exp("min_component_points") == 0 and cfg.exp("component_radius") == 0.0
    for mode in ("sampled", "dense"):
        for backend in ("device", "host"):
            for extra in ({}, {"estimate_normals": True}, {"min_consensus_refs": 1, "consensus_radius": 0.1}, {"footprint_thin_cells": 1.0},
                          {"min_freespace_violations": 1}):
                assert lfd.DensePipelineConfig(output_path="a.ply", triangulation_mode=mode, backend=backend, experimental={**ON, **extra}).problem() is None
    assert lfd.DensePipelineConfig(output_path="a.bin", max_points=10, voxel_size=0.1, no_filter=True, experimental=ON).problem() is None
    assert lfd.DensePipelineConfig(output_path="a.ply", experimental={**ON, "min_component_points": np.int64(2 ** 31 - 1)}).problem() is None
    refused = [
        (dict(), {**ON, "min_component_points": -1}, r"min_component_points'\] must be an integer in 0 \.\. 2\^31 - 1"),
        (dict(), {**ON, "min_component_points": 2 ** 31}, r"min_component_points'\] must be an integer in 0 \.\. 2\^31 - 1"),
        (dict(), {**ON, "min_component_points": 2.0}, r"min_component_points'\] must be an integer"),
        (dict(), {**ON, "min_component_points": True}, r"min_component_points'\] must be an integer"),
        (dict(), {"min_component_points": "ten"}, r"min_component_points'\] must be an integer"),
        (dict(), {**ON, "min_component_points": 1}, r"min_component_points'\] = 1 keeps every point"),
        (dict(), {**ON, "component_radius": -0.1}, r"component_radius'\] must be finite and >= 0"),
        (dict(), {**ON, "component_radius": float("inf")}, r"component_radius'\] must be finite and >= 0"),
        (dict(), {**ON, "component_radius": float("nan")}, r"component_radius'\] must be finite and >= 0"),
        (dict(), {**ON, "component_radius": "wide"}, r"component_radius'\] must be a number"),
        (dict(), {"min_component_points": 5}, r"min_component_points'\] needs a distance"),
        (dict(), {"min_component_points": 5, "component_radius": 0.0}, r"min_component_points'\] needs a distance"),
        (dict(), {"component_radius": 0.05}, r"component_radius'\] is the link distance of the component filter"),
        (dict(stream_output=True), ON, r"min_component_points'\] has to see the whole cloud"),
        (dict(triangulation_mode="dense", stream_output=True), ON, r"min_component_points'\] has to see the whole cloud"),
        (dict(), {**ON, "exchange_records": "ply"}, r"min_component_points'\] filters f32 rows"),
        (dict(triangulation_mode="dense"), {**ON, "dense_tile_segments": True}, r"min_component_points'\] needs the cloud as arrays"),
    ]
    for kw, exp, text in refused:
        with pytest.raises(ValueError, match=text):
            lfd.DensePipelineConfig(output_path="a.ply", experimental=exp, **kw)
    # switched off, none of the routes is refused
    for kw, exp in ((dict(stream_output=True), {}), (dict(triangulation_mode="dense"), {"dense_tile_segments": True})):
        assert lfd.DensePipelineConfig(output_path="a.ply", experimental={**exp, "min_component_points": 0}, **kw).problem() is None


def test_a_sharded_run_is_refused(scene, monkeypatch):  # noqa: F811
    import torch.distributed as dist
    from lichtfeld_densification_plugin_amd.core import pipeline as pl
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    monkeypatch.setattr(dist, "get_rank", lambda *a: 0)
    cfg = lfd.DensePipelineConfig(output_path="a.ply", backend="host", experimental=ON)
    with pytest.raises(ValueError, match=r"min_component_points'\] cannot run sharded over several GPUs"):
        pl.run_dense_pipeline(scene["cams"], scene["refs"], scene["nn"], cfg)


def test_the_cli_flags_reach_the_configuration():
    ap = densify.build_argparser()
    args = ap.parse_args(["--scene_root", "x", "--min_component_points", "50", "--component_radius", "0.05"])
    assert (args.min_component_points, args.component_radius) == (50, 0.05)
    assert densify._experimental_from_args(args) == {"min_component_points": 50, "component_radius": 0.05}
    off = ap.parse_args(["--scene_root", "x"])
    assert (off.min_component_points, off.component_radius) == (0, 0.0) and densify._experimental_from_args(off) == {}
    with pytest.raises(ValueError, match="needs a distance"):
        lfd.DensePipelineConfig(output_path="a.ply", experimental=densify._experimental_from_args(ap.parse_args(["--scene_root", "x", "--min_component_points", "5"])))


def test_both_entry_points_write_the_knob_off_cloud_under_the_reference_mask(scene, tmp_path, monkeypatch, caplog):  # noqa: F811
    spy = Spy(monkeypatch)

    def never(*a, **kw):
        raise AssertionError("the filter ran with the knob off")
    off_out, on_out = os.path.join(str(tmp_path), "off.ply"), os.path.join(str(tmp_path), "on.ply")
    with monkeypatch.context() as m:
        m.setattr(hb.HostDensifier, "component_filter", never)
        off_msgs = []
        assert gui_run(scene, off_out, "sampled", {}, off_msgs) == (0, off_out)
    assert not os.path.exists(off_out + ".components.json")
    msgs = []
    with caplog.at_level(logging.INFO, logger="lfd_densify"):
        assert gui_run(scene, on_out, "sampled", ON, msgs) == (0, on_out)
    off_cloud, on_cloud = spy.results
    for a, b in zip(off_cloud, on_cloud):                                  # what the pipeline returns does not know the knob
        assert np.array_equal(a, b)
    xyz, rgb, err, counts = on_cloud
    assert open(off_out, "rb").read() == written(os.path.join(str(tmp_path), "off_ref.ply"), xyz, rgb, err)
    keep, size, label, _kept, summ = reference(on_cloud)
    n, k = xyz.shape[0], int(keep.sum())
    print(f"{n} points in {summ[0]} components, {k} kept at radius {RADIUS} with at least {MIN_POINTS} points; largest {summ[1]}")
    assert 0.05 * n < k < 0.95 * n                                         # both happen: the comparison below can fail
    assert open(on_out, "rb").read() == written(os.path.join(str(tmp_path), "on_ref.ply"), xyz[keep], rgb[keep], err[keep])
    assert (93.5, "Applying component filter...") in msgs and [p for p, _m in msgs if p != 93.5] == [p for p, _m in off_msgs]
    # the report is the reference's summary, and holds no timing
    report = json.load(open(on_out + ".components.json"))
    assert report == densify.component_report(RADIUS, MIN_POINTS, n, k, summ)
    assert report["n_components"] == int(summ[0]) and report["largest_component"] == int(summ[1]) and report["points_in"] == n and report["points_out"] == k
    assert sum(b["components"] for b in report["bins"]) == int(summ[0]) and sum(b["points"] for b in report["bins"]) == n
    assert [b["components"] for b in report["bins"]] == summ[2:2 + len(report["bins"])].tolist() and not summ[2 + len(report["bins"]):34].any()
    assert set(report) == {"component_radius", "min_component_points", "points_in", "points_out", "n_components", "largest_component", "bins"}
    dropped = int(((label == np.arange(n)) & ~keep).sum())
    lines = [r.getMessage() for r in caplog.records if r.getMessage().startswith("Component filter")]
    assert len(lines) == 1 and f"{n - k:,} points in {dropped:,} components dropped" in lines[0]
    # dense_init (the CLI entry point) likewise: its own knob-off cloud (it loads the cameras from the scene's files) under the reference's mask
    rc, cli_path = cli_run(scene, "on_cli.ply", "sampled", ["--min_component_points", str(MIN_POINTS), "--component_radius", str(RADIUS)])
    cxyz, crgb, cerr, _ccounts = spy.results[2]
    ckeep, _s, _l, _k, csumm = reference(spy.results[2])
    assert rc == 0 and 0.05 * cxyz.shape[0] < ckeep.sum() < 0.95 * cxyz.shape[0]
    assert open(cli_path, "rb").read() == written(os.path.join(str(tmp_path), "cli_ref.ply"), cxyz[ckeep], crgb[ckeep], cerr[ckeep])
    assert json.load(open(cli_path + ".components.json")) == densify.component_report(RADIUS, MIN_POINTS, cxyz.shape[0], int(ckeep.sum()), csumm)


def test_the_normals_follow_the_points(scene, tmp_path, monkeypatch):  # noqa: F811
    spy = Spy(monkeypatch)
    full_out, on_out = os.path.join(str(tmp_path), "full.ply"), os.path.join(str(tmp_path), "on.ply")
    assert gui_run(scene, full_out, "sampled", {"estimate_normals": True}) == (0, full_out)
    assert gui_run(scene, on_out, "sampled", {"estimate_normals": True, **ON}) == (0, on_out)
    keep = reference(spy.results[1])[0]
    full, less = records(full_out, True), records(on_out, True)
    assert 0 < less.shape[0] < full.shape[0] and full.shape[0] == keep.shape[0]
    assert full[keep].tobytes() == less.tobytes()                          # positions, normals and colours of the kept rows, nothing else


def test_behind_the_consensus_filter_and_in_front_of_cap_and_voxel_filter(scene, tmp_path, monkeypatch):  # noqa: F811
    spy = Spy(monkeypatch)
    out = os.path.join(str(tmp_path), "chain.ply")
    front = {"min_consensus_refs": 1, "consensus_radius": 0.02}
    msgs = []
    assert gui_run(scene, out, "sampled", {**front, **ON}, msgs, max_points=900) == (0, out)
    xyz, rgb, err, counts = spy.results[0]
    twin = hb.HostDensifier(2)
    try:
        import torch
        t = torch.from_numpy
        cx, cc, ce, ckept, _cons = twin.consensus_filter(t(xyz), t(rgb), t(err), counts, 0.02, 1)
    finally:
        twin.close()
    after = (cx.numpy(), cc.numpy(), ce.numpy(), ckept)
    keep = reference(after)[0]
    assert 0 < keep.sum() < after[0].shape[0] < xyz.shape[0] and keep.sum() > 900
    px, pc, pe = densify._apply_point_cap(after[0][keep], after[1][keep], after[2][keep], 900, 3)
    assert open(out, "rb").read() == written(os.path.join(str(tmp_path), "chain_ref.ply"), px, pc, pe)
    steps = [m for _p, m in msgs if m.startswith("Applying")]
    assert steps[:2] == ["Applying consensus filter...", "Applying component filter..."]


def test_a_cloud_too_wide_for_the_radius_names_the_knob(scene, tmp_path):  # noqa: F811
    code, msg = gui_run(scene, os.path.join(str(tmp_path), "refused.ply"), "sampled", {"min_component_points": 2, "component_radius": 1e-12})
    assert code == 1 and "component_radius" in msg and "key range" in msg
