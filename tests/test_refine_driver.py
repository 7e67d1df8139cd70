"""The multi-view re-triangulation in the driver, on the host backend (core/types.py, core/hotpath.py, core/pipeline.py, densify.py) with the
analytic matcher: the knob-on cloud is the knob-off cloud - same (cell, slot) per reference in the same order, hence the same position of the
sampling stream, same colours and counts - with the coordinates of exactly the accepted points replaced, in sampled and in dense mode; behind the
support filter it is the filtered cloud that is refined; a pair the forward-backward gate rejected is never a candidate; the refusals of
``problem()``; the CLI flag."""
import contextlib
import logging

import numpy as np
import pytest

import cycle_ref
import cycle_scene
import support_ref
import lichtfeld_densification_plugin_amd as lfd
from lichtfeld_densification_plugin_amd import densify
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from lichtfeld_densification_plugin_amd.core.types import EXPERIMENTAL_DEFAULTS

bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    return cycle_scene.make_scene(str(tmp_path_factory.mktemp("refine_scene")), n_cams=4)      # three references, each with the three other cameras


@contextlib.contextmanager
def recorded_refines():
    """Every call of the twin's refine_multiview a run makes, in order: what went in, what came out and the status byte of every point."""
    seen = []
    plain = hb.HostDensifier.refine_multiview

    def refine(self, batch, out, tau, thr, with_status=False, counters=None):
        res, st = plain(self, batch, out, tau, thr, with_status=True, counters=counters)
        seen.append(dict(cell=out.cell.numpy().copy(), slot=out.slot.numpy().copy(), xyz_in=out.xyz.numpy().copy(), xyz_out=res.xyz.numpy().copy(),
                         err_in=out.err.numpy().copy(), err_out=res.err.numpy().copy(), status=st.numpy().copy(),
                         off=np.asarray(out.ref_offsets).copy(), tau=float(tau), thr=float(thr)))
        return (res, st) if with_status else res

    hb.HostDensifier.refine_multiview = refine
    try:
        yield seen
    finally:
        hb.HostDensifier.refine_multiview = plain


def joined(seen, name):
    return np.concatenate([s[name] for s in seen])


def test_the_knob_is_experimental_off_by_default_and_validated():
    assert EXPERIMENTAL_DEFAULTS["multiview_refine"] is False
    assert lfd.DensePipelineConfig(output_path="a.ply").exp("multiview_refine") is False
    on = {"multiview_refine": True}
    for mode in ("sampled", "dense"):
        for backend in ("device", "host"):
            for extra in ({}, {"min_support_views": 1}, {"min_support_views": 0, "support_thresh_px": 3.0}, {"cycle_thresh_px": 1.0}):
                assert lfd.DensePipelineConfig(output_path="a.ply", triangulation_mode=mode, backend=backend, experimental={**on, **extra}).problem() is None
    assert lfd.DensePipelineConfig(output_path="a.ply", stream_output=True, experimental=on).problem() is None          # sampled mode streams arrays
    assert lfd.DensePipelineConfig(output_path="a.ply", nns_per_ref=2, experimental=on).problem() is None
    assert lfd.DensePipelineConfig(output_path="a.ply", experimental={**on, "support_thresh_px": 2.5}).support_threshold() == 2.5
    refused = [
        (dict(no_filter=True), on, "no_filter"),
        (dict(reproj_thresh=0.0), on, "reproj_thresh must be > 0"),
        (dict(reproj_thresh=-1.0), on, "reproj_thresh must be > 0"),
        (dict(nns_per_ref=1), on, "nns_per_ref must be at least 2"),
        (dict(triangulation_mode="dense", stream_output=True), on, "stream_output"),
        (dict(triangulation_mode="dense"), {**on, "dense_tile_segments": True}, "dense_tile_segments"),
        (dict(), {**on, "exchange_records": "ply"}, "exchange_records"),
        (dict(), {"multiview_refine": 1}, "True or False"),
        (dict(), {"multiview_refine": "yes"}, "True or False"),
        (dict(), {"multiview_refine": None}, "True or False"),
    ]
    for kw, exp, text in refused:
        with pytest.raises(ValueError, match=text):
            lfd.DensePipelineConfig(output_path="a.ply", experimental=exp, **kw)
    # switched off, none of the routes is refused
    for kw in (dict(no_filter=True), dict(nns_per_ref=1), dict(triangulation_mode="dense", stream_output=True)):
        assert lfd.DensePipelineConfig(output_path="a.ply", experimental={"multiview_refine": False}, **kw).problem() is None


def test_the_cli_flag_reaches_the_configuration():
    ap = densify.build_argparser()
    args = ap.parse_args(["--scene_root", "x", "--multiview_refine", "--support_thresh_px", "2.5"])
    assert args.multiview_refine is True
    assert densify._experimental_from_args(args) == {"multiview_refine": True, "support_thresh_px": 2.5}
    off = ap.parse_args(["--scene_root", "x"])
    assert off.multiview_refine is False and densify._experimental_from_args(off) == {}
    cfg = lfd.DensePipelineConfig(output_path="a.ply", nns_per_ref=off.nns_per_ref, experimental=densify._experimental_from_args(args))
    assert cfg.exp("multiview_refine") is True and cfg.support_threshold() == 2.5


def test_with_the_knob_off_no_new_code_runs(scene, monkeypatch):
    def never(*a, **kw):
        raise AssertionError("the re-triangulation ran with the knob off")
    monkeypatch.setattr(hb.HostDensifier, "refine_multiview", never)
    plain = cycle_scene.run(scene, cycle_scene.matcher_for(scene), "plain.ply", triangulation_mode="sampled")
    off = cycle_scene.run(scene, cycle_scene.matcher_for(scene), "off.ply", triangulation_mode="sampled",
                          experimental={"multiview_refine": False, "min_support_views": 1})
    assert plain.xyz.shape[0] > 1000 and 0 < off.xyz.shape[0] < plain.xyz.shape[0]


@pytest.mark.parametrize("mode,group", [("sampled", 1), ("dense", 1), ("dense", 2)])
def test_the_cloud_is_the_knob_off_cloud_with_the_accepted_points_moved(scene, mode, group, caplog):
    """Sampled mode on the host backend takes one reference per call (several per fused call need the device: tests/test_gpu_refine.py); dense
    mode is run with one and with two references per launch (of three: a full and a short group)."""
    with cycle_scene.recorded_cells() as cells_off:
        off = cycle_scene.run(scene, cycle_scene.matcher_for(scene), "off.ply", triangulation_mode=mode, refs_per_launch=group)
    with caplog.at_level(logging.INFO, logger="lfd_densify"), cycle_scene.recorded_cells() as cells_on, recorded_refines() as seen:
        on = cycle_scene.run(scene, cycle_scene.matcher_for(scene), "on.ply", triangulation_mode=mode, refs_per_launch=group,
                             experimental={"multiview_refine": True})
    n = len(scene["refs"])
    # the same (cell, slot) per reference: every reference drew the same cells, so the sampling stream stood where it stands with the knob off
    assert len(cells_off) == n and cells_on == cells_off
    assert sum(len(s["off"]) - 1 for s in seen) == n and all(s["tau"] == pytest.approx(1.6) and s["thr"] == pytest.approx(0.8) for s in seen)
    status, xyz_in, xyz_out = joined(seen, "status"), joined(seen, "xyz_in"), joined(seen, "xyz_out")
    assert on.xyz.shape == off.xyz.shape and np.array_equal(on.points_per_reference, off.points_per_reference)
    assert np.array_equal(bits(off.xyz), bits(xyz_in)) and np.array_equal(bits(on.xyz), bits(xyz_out))          # the order, too
    assert np.array_equal(bits(on.rgb), bits(off.rgb))
    accepted = (status & 0x80) != 0
    assert np.array_equal((bits(on.xyz) != bits(off.xyz)).any(axis=1), accepted)
    assert np.array_equal(bits(on.err)[~accepted], bits(off.err)[~accepted]) and (on.err <= np.float32(0.8)).all()
    fallback = ((status & 0x7f) != 0) & ~accepted
    print(f"{mode} x{group}: {off.xyz.shape[0]} points, {int(accepted.sum())} refined, {int(fallback.sum())} fallen back")
    assert accepted.sum() > 0.5 * off.xyz.shape[0] and fallback.sum() > 0
    lines = [r.getMessage() for r in caplog.records if "Multi-view re-triangulation" in r.getMessage()]
    assert lines == [f"Multi-view re-triangulation: threshold 1.6 px, {int(accepted.sum())} points refined, {int(fallback.sum())} confirmed points "
                     f"kept their two-view position"]


@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_behind_the_support_filter_the_filtered_cloud_is_refined(scene, mode):
    only_filter = cycle_scene.run(scene, cycle_scene.matcher_for(scene), "f.ply", triangulation_mode=mode, experimental={"min_support_views": 1})
    with recorded_refines() as seen:
        both = cycle_scene.run(scene, cycle_scene.matcher_for(scene), "fr.ply", triangulation_mode=mode,
                               experimental={"min_support_views": 1, "multiview_refine": True})
    status = joined(seen, "status")
    assert np.array_equal(bits(joined(seen, "xyz_in")), bits(only_filter.xyz)) and np.array_equal(bits(joined(seen, "xyz_out")), bits(both.xyz))
    assert np.array_equal(both.points_per_reference, only_filter.points_per_reference) and np.array_equal(bits(both.rgb), bits(only_filter.rgb))
    assert ((status & 0x7f) >= 1).all()                                          # what the filter kept has a candidate, by definition
    accepted = (status & 0x80) != 0
    assert np.array_equal((bits(both.xyz) != bits(only_filter.xyz)).any(axis=1), accepted) and 0 < accepted.sum() < status.size


def test_a_pair_the_cycle_gate_rejected_is_never_a_candidate(scene):
    """Depth steps and out-of-range columns, the forward-backward gate at 1 px, the support threshold enormous: what decides is who is LIVE.  The
    number of candidates of a point lies between the other neighbours whose gated certainty at its cell is surely not 0 and those where it may
    not be (cells inside the gate's own rounding band may go either way)."""
    kw = dict(occlusion_steps=True, out_of_range=0.3)
    matcher = cycle_scene.matcher_for(scene, **kw)
    with recorded_refines() as seen:
        cycle_scene.run(scene, matcher, "gate_refine.ply", triangulation_mode="dense",
                        experimental={"cycle_thresh_px": 1.0, "multiview_refine": True, "support_thresh_px": 1e9})
    assert len(seen) == len(scene["refs"])
    matcher.set_backward_warp(True)
    fewer = 0
    for r, s in zip(scene["refs"], seen):
        nbrs = [int(v) for v in scene["nn"][r][:3]]
        _key, fields = matcher.fields(r, nbrs)
        gated = [cycle_ref.reference(c.numpy(), w.numpy(), b.numpy(), matcher.w_resized, matcher.h_resized, 0.2, 1.0) for w, c, b in fields]
        cell, slot = s["cell"], s["slot"]
        alive = np.stack([g["keep"].reshape(-1)[cell] for g in gated], axis=1)
        unsure = np.stack([g["band"].reshape(-1)[cell] for g in gated], axis=1)
        others = np.arange(3)[None, :] != slot[:, None]
        ref = support_ref.reference(scene["cams"], r, nbrs, [g["cert_out"] for g in gated], [f[0].numpy() for f in fields], None, matcher.w_resized,
                                    matcher.h_resized, cell, slot, s["xyz_in"], 1e9)
        agree = ref["agree"]                                                     # at 1e9 px: the point is in front of the neighbour
        n_extra = (s["status"] & 0x7f).astype(np.int64)
        lo = (others & alive & ~unsure & agree).sum(axis=1)
        hi = (others & (alive | unsure) & agree).sum(axis=1)
        assert (lo <= n_extra).all() and (n_extra <= hi).all()
        fewer += int((hi < 2).sum())
    assert fewer > 100                                                           # the gate took candidates away: the test can fail
