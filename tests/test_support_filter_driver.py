"""The multi-view support filter in the driver, on the host backend (core/types.py, core/hotpath.py, core/strategies.py, core/pipeline.py,
densify.py) with the analytic matcher: the knob-on cloud is the knob-off cloud restricted to the f64 reference's decisions - same order, same bits,
points with a test inside the rounding band left out of the comparison - in sampled and in dense mode; an enormous threshold keeps exactly the
points that have a live other neighbour; a pair the forward-backward gate rejected does not vouch; the refusals of ``problem()``; the CLI flags."""
import contextlib
import logging

import numpy as np
import pytest

import cycle_ref
import cycle_scene
import support_ref
import support_scene as sc
import lichtfeld_densification_plugin_amd as lfd
from lichtfeld_densification_plugin_amd import densify
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from lichtfeld_densification_plugin_amd.core.types import EXPERIMENTAL_DEFAULTS

GRID_W = 320          # the "turbo" grid of the analytic matcher


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    return cycle_scene.make_scene(str(tmp_path_factory.mktemp("support_scene")), n_cams=4)      # three references, each with the three other cameras


@contextlib.contextmanager
def collected():
    """Every result a run collects from the twin's output buffers, in order: (cell, slot, xyz, ref_offsets) arrays."""
    seen = []
    plain = hb.OutputBuffers.collect

    def collect(self, *a, **kw):
        res = plain(self, *a, **kw)
        seen.append((res.cell.numpy().copy(), res.slot.numpy().copy(), res.xyz.numpy().copy(), np.asarray(res.ref_offsets).copy()))
        return res

    hb.OutputBuffers.collect = collect
    try:
        yield seen
    finally:
        hb.OutputBuffers.collect = plain


def per_reference(seen):
    out = []
    for cell, slot, xyz, off in seen:
        for r in range(len(off) - 1):
            out.append((cell[off[r]:off[r + 1]], slot[off[r]:off[r + 1]], xyz[off[r]:off[r + 1]]))
    return out


def reference_of(scene, matcher, r, cell, slot, xyz, tau, certs=None):
    nbrs = [int(n) for n in scene["nn"][r][:3]]
    _key, fields = matcher.fields(r, nbrs)
    cert = certs if certs is not None else [f[1].numpy() for f in fields]
    return support_ref.reference(scene["cams"], r, nbrs, cert, [f[0].numpy() for f in fields], None, matcher.w_resized, matcher.h_resized, cell, slot,
                                 xyz, tau)


def test_the_knobs_are_experimental_off_by_default_and_validated():
    assert EXPERIMENTAL_DEFAULTS["min_support_views"] == 0 and EXPERIMENTAL_DEFAULTS["support_thresh_px"] == 0.0
    cfg = lfd.DensePipelineConfig(output_path="a.ply")
    assert cfg.exp("min_support_views") == 0 and cfg.support_threshold() == pytest.approx(1.6)
    assert lfd.DensePipelineConfig(output_path="a.ply", reproj_thresh=1.25, experimental={"min_support_views": 1}).support_threshold() == 2.5
    assert lfd.DensePipelineConfig(output_path="a.ply", experimental={"min_support_views": 2, "support_thresh_px": 3.0}).support_threshold() == 3.0
    for mode in ("sampled", "dense"):
        for backend in ("device", "host"):
            assert lfd.DensePipelineConfig(output_path="a.ply", triangulation_mode=mode, backend=backend,
                                           experimental={"min_support_views": 2}).problem() is None
    assert lfd.DensePipelineConfig(output_path="a.ply", stream_output=True, experimental={"min_support_views": 1}).problem() is None     # sampled mode streams arrays
    assert lfd.DensePipelineConfig(output_path="a.ply", nns_per_ref=8, experimental={"min_support_views": 7}).problem() is None
    refused = [
        (dict(triangulation_mode="dense", stream_output=True), {"min_support_views": 1}, "stream_output"),
        (dict(triangulation_mode="dense"), {"min_support_views": 1, "dense_tile_segments": True}, "dense_tile_segments"),
        (dict(), {"min_support_views": 1, "exchange_records": "ply"}, "exchange_records"),
        (dict(), {"min_support_views": 3}, "nns_per_ref - 1"),
        (dict(nns_per_ref=1), {"min_support_views": 1}, "nns_per_ref - 1"),
        (dict(), {"min_support_views": -1}, "non-negative integer"),
        (dict(), {"min_support_views": 1.5}, "non-negative integer"),
        (dict(), {"min_support_views": True}, "non-negative integer"),
        (dict(), {"min_support_views": "two"}, "non-negative integer"),
        (dict(), {"support_thresh_px": -1.0}, "support_thresh_px"),
        (dict(), {"support_thresh_px": float("inf")}, "support_thresh_px"),
        (dict(), {"support_thresh_px": float("nan")}, "support_thresh_px"),
        (dict(), {"support_thresh_px": "wide"}, "support_thresh_px"),
        (dict(reproj_thresh=0.0), {"min_support_views": 1}, "needs a threshold"),
    ]
    for kw, exp, text in refused:
        with pytest.raises(ValueError, match=text):
            lfd.DensePipelineConfig(output_path="a.ply", experimental=exp, **kw)
    # switched off, none of the routes is refused and the threshold alone is harmless
    assert lfd.DensePipelineConfig(output_path="a.ply", triangulation_mode="dense", stream_output=True,
                                   experimental={"support_thresh_px": 2.0}).problem() is None


def test_the_cli_flags_reach_the_configuration():
    ap = densify.build_argparser()
    args = ap.parse_args(["--scene_root", "x", "--min_support_views", "2", "--support_thresh_px", "2.5", "--cycle_thresh_px", "1.25"])
    assert (args.min_support_views, args.support_thresh_px) == (2, 2.5)
    assert densify._experimental_from_args(args) == {"min_support_views": 2, "support_thresh_px": 2.5, "cycle_thresh_px": 1.25}
    off = ap.parse_args(["--scene_root", "x"])
    assert (off.min_support_views, off.support_thresh_px) == (0, 0.0) and densify._experimental_from_args(off) == {}
    cfg = lfd.DensePipelineConfig(output_path="a.ply", nns_per_ref=off.nns_per_ref, experimental=densify._experimental_from_args(args))
    assert cfg.exp("min_support_views") == 2 and cfg.support_threshold() == 2.5


@pytest.mark.parametrize("mode", ["sampled"])
def test_with_the_knob_off_no_new_code_runs(scene, mode, monkeypatch):
    def never(*a, **kw):
        raise AssertionError("the filter ran with the knob off")
    monkeypatch.setattr(hb.HostDensifier, "support_filter", never)
    plain = cycle_scene.run(scene, cycle_scene.matcher_for(scene), "plain.ply", triangulation_mode=mode)
    zero = cycle_scene.run(scene, cycle_scene.matcher_for(scene), "zero.ply", triangulation_mode=mode,
                           experimental={"min_support_views": 0, "support_thresh_px": 3.0})
    assert plain.xyz.shape[0] > 1000 and cycle_scene.same_cloud(plain, zero)


@pytest.mark.parametrize("mode,group,m", [("sampled", 1, 1), ("dense", 1, 1), ("dense", 2, 2)])
def test_the_cloud_is_the_knob_off_cloud_restricted_to_the_reference_s_mask(scene, mode, group, m, caplog):
    """Sampled mode on the host backend takes one reference per call (several per fused call need the device: tests/test_gpu_support_filter.py);
    dense mode is run with one and with two references per launch (of three: a full and a short group)."""
    matcher = cycle_scene.matcher_for(scene)
    with collected() as seen_off:
        off = cycle_scene.run(scene, cycle_scene.matcher_for(scene), "off.ply", triangulation_mode=mode, refs_per_launch=group)
    with caplog.at_level(logging.INFO, logger="lfd_densify"), collected() as seen_on:
        on = cycle_scene.run(scene, matcher, "on.ply", triangulation_mode=mode, refs_per_launch=group, experimental={"min_support_views": m})
    refs_off = per_reference(seen_off)
    assert len(refs_off) == len(scene["refs"]) and sum(len(c) for c, _s, _x in refs_off) == off.xyz.shape[0]
    tau = 1.6
    want_keep, clean = [], []
    tests = in_band = 0
    for r, (cell, slot, xyz) in zip(scene["refs"], refs_off):
        ref = reference_of(scene, matcher, r, cell, slot, xyz, tau)
        want_keep.append(ref["support"] >= m)
        clean.append(ref["clean"])
        counted = ref["tested"] & ref["live"]
        tests += int(counted.sum())
        in_band += int((counted & ref["band"]).sum())
    want_keep, clean = np.concatenate(want_keep), np.concatenate(clean)
    assert in_band / tests <= sc.BAND_CAP
    # the knob-on cloud: the knob-off cloud restricted to a mask, in order, bit for bit.  (The host backend collects a launch's points and then
    # the filter's result: every second collected buffer is what the run emits; a (cell, slot) pair is unique inside a reference.)
    refs_on = per_reference(seen_on[1::2])
    assert len(refs_on) == len(refs_off)
    kept = np.concatenate([np.isin(c.astype(np.int64) * 16 + s, c_on.astype(np.int64) * 16 + s_on) for (c, s, _x), (c_on, s_on, _y) in zip(refs_off, refs_on)])
    for (c, s, _x), (c_on, s_on, _y), lo in zip(refs_off, refs_on, np.concatenate([[0], np.cumsum([len(c) for c, _s, _x in refs_off])])):
        k_r = kept[lo:lo + len(c)]
        assert np.array_equal(c[k_r], c_on) and np.array_equal(s[k_r], s_on)
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    for name in ("xyz", "rgb", "err"):
        assert np.array_equal(bits(getattr(on, name)), bits(getattr(off, name))[kept]), name
    assert np.array_equal(kept[clean], want_keep[clean])
    dropped = off.xyz.shape[0] - on.xyz.shape[0]
    print(f"{mode} x{group} m={m}: {off.xyz.shape[0]} points, {dropped} dropped, {in_band} of {tests} tests in band, {int((~clean).sum())} points left out")
    assert 0 < dropped < 0.5 * off.xyz.shape[0]
    offs = np.concatenate([[0], np.cumsum([len(c) for c, _s, _x in refs_off])])
    assert np.array_equal(on.points_per_reference, [int(kept[offs[i]:offs[i + 1]].sum()) for i in range(len(refs_off))])
    lines = [r.getMessage() for r in caplog.records if "Multi-view support filter" in r.getMessage()]
    assert lines == [f"Multi-view support filter: threshold 1.6 px, at least {m} other view(s), {off.xyz.shape[0]} points in, {dropped} dropped"]


@pytest.mark.parametrize("mode", ["dense"])
def test_a_pair_the_cycle_gate_rejected_does_not_vouch(scene, mode):
    """Depth steps and out-of-range columns, the forward-backward gate at 1 px, the support threshold enormous: what decides is who is LIVE.  A
    point is kept iff some other neighbour's GATED certainty at its cell is not 0 (cells inside the gate's own rounding band may go either way)."""
    kw = dict(occlusion_steps=True, out_of_range=0.3)
    gate = {"cycle_thresh_px": 1.0}
    with collected() as seen_off:
        off = cycle_scene.run(scene, cycle_scene.matcher_for(scene, **kw), "gate.ply", triangulation_mode=mode, experimental=gate)
    matcher = cycle_scene.matcher_for(scene, **kw)
    with collected() as seen_on:
        on = cycle_scene.run(scene, matcher, "gate_support.ply", triangulation_mode=mode,
                             experimental={**gate, "min_support_views": 1, "support_thresh_px": 1e9})
    refs_off, refs_on = per_reference(seen_off), per_reference(seen_on)[1::2]          # (the host backend collects the points, then the filter's result)
    n = len(scene["refs"])
    assert len(refs_off) == n and len(refs_on) == n
    matcher.set_backward_warp(True)
    kept_total = dropped_total = 0
    for r, (cell, slot, xyz), (cell_on, slot_on, _x) in zip(scene["refs"], refs_off, refs_on):
        nbrs = [int(v) for v in scene["nn"][r][:3]]
        _key, fields = matcher.fields(r, nbrs)
        gated = [cycle_ref.reference(c.numpy(), w.numpy(), b.numpy(), matcher.w_resized, matcher.h_resized, 0.2, 1.0) for w, c, b in fields]
        alive = np.stack([g["keep"].reshape(-1)[cell] for g in gated], axis=1)               # (n, 3): the pair survives the gate at the point's cell
        unsure = np.stack([g["band"].reshape(-1)[cell] for g in gated], axis=1)
        others = np.arange(3)[None, :] != slot[:, None]
        ref = reference_of(scene, matcher, r, cell, slot, xyz, 1e9, certs=[g["cert_out"] for g in gated])
        agree = ref["agree"]                                                             # at 1e9 px: the point is in front of the neighbour
        must_keep = (others & alive & ~unsure & agree).any(axis=1)
        must_drop = ~(others & (alive | unsure) & agree).any(axis=1)
        on_set = set(zip(cell_on.tolist(), slot_on.tolist()))
        was_kept = np.array([(c, s) in on_set for c, s in zip(cell.tolist(), slot.tolist())], bool)
        assert was_kept[must_keep].all() and not was_kept[must_drop].any()
        assert on_set <= set(zip(cell.tolist(), slot.tolist()))
        kept_total += int(was_kept.sum())
        dropped_total += int((~was_kept).sum())
    assert kept_total == on.xyz.shape[0] and kept_total + dropped_total == off.xyz.shape[0]
    assert dropped_total > 0.01 * off.xyz.shape[0] and kept_total > 0.02 * off.xyz.shape[0]       # both happen: the test can fail


def test_an_enormous_threshold_keeps_every_point_with_a_live_other_neighbour(scene):
    """Without the gate every certainty of the analytic matcher is > 0: nothing is dropped, the clouds are the same bit for bit."""
    off = cycle_scene.run(scene, cycle_scene.matcher_for(scene), "all_off.ply", triangulation_mode="dense")
    on = cycle_scene.run(scene, cycle_scene.matcher_for(scene), "all_on.ply", triangulation_mode="dense",
                         experimental={"min_support_views": 1, "support_thresh_px": 1e9})
    assert off.xyz.shape[0] > 1000 and cycle_scene.same_cloud(off, on)
