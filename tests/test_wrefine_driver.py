"""The precision-weighted re-triangulation in the driver, on the host backend (core/types.py, core/hotpath.py, core/pipeline.py, densify.py) with
the analytic matcher under heteroscedastic noise: the knob-on cloud is the ``multiview_refine`` cloud - same (cell, slot) per reference in the
same order, same colours and counts - in sampled mode and in dense mode with one and two references per launch; it combines with the support
filter and the forward-backward gate; the refusals of ``problem()``; the CLI flag; an injected matcher without the planes is refused, one that
declared them and returns none raises, and with the knob off the matcher is never asked for them."""
import contextlib
import logging

import numpy as np
import pytest

import cycle_scene
import lichtfeld_densification_plugin_amd as lfd
from lichtfeld_densification_plugin_amd import densify, synthetic
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from lichtfeld_densification_plugin_amd.core.types import EXPERIMENTAL_DEFAULTS

bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
ON = {"multiview_refine": True, "precision_weighted_refine": True}
HETERO = dict(noise_model="hetero")


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    return cycle_scene.make_scene(str(tmp_path_factory.mktemp("wrefine_scene")), n_cams=4)      # three references, each with the three other cameras


@contextlib.contextmanager
def recorded_refines():
    """Every call of the twin's refine_multiview a run makes, in order: its input, its output, the status bytes and whether it was weighted."""
    seen = []
    plain = hb.HostDensifier.refine_multiview

    def refine(self, batch, out, tau, thr, with_status=False, counters=None, precision=False):
        res, st = plain(self, batch, out, tau, thr, with_status=True, counters=counters, precision=precision)
        seen.append(dict(xyz_in=out.xyz.numpy().copy(), xyz_out=res.xyz.numpy().copy(), status=st.numpy().copy(), precision=bool(precision),
                         planes=batch.precision is not None, n_counters=None if counters is None else int(counters.numel())))
        return (res, st) if with_status else res

    hb.HostDensifier.refine_multiview = refine
    try:
        yield seen
    finally:
        hb.HostDensifier.refine_multiview = plain


def joined(seen, name):
    return np.concatenate([s[name] for s in seen])


def test_the_knob_is_experimental_off_by_default_and_validated():
    assert EXPERIMENTAL_DEFAULTS["precision_weighted_refine"] is False
    assert lfd.DensePipelineConfig(output_path="a.ply").exp("precision_weighted_refine") is False
    for mode in ("sampled", "dense"):
        for backend in ("device", "host"):
            for extra in ({}, {"min_support_views": 1}, {"support_thresh_px": 3.0}, {"cycle_thresh_px": 1.0}):
                assert lfd.DensePipelineConfig(output_path="a.ply", triangulation_mode=mode, backend=backend, experimental={**ON, **extra}).problem() is None
    assert lfd.DensePipelineConfig(output_path="a.ply", stream_output=True, experimental=ON).problem() is None          # sampled mode streams arrays
    refused = [
        (dict(), {"precision_weighted_refine": True}, "needs experimental\\['multiview_refine'\\]"),
        (dict(), {"precision_weighted_refine": True, "multiview_refine": False}, "needs experimental\\['multiview_refine'\\]"),
        (dict(), {**ON, "precision_weighted_refine": 1}, "precision_weighted_refine'\\] must be True or False"),
        (dict(), {**ON, "precision_weighted_refine": "yes"}, "precision_weighted_refine'\\] must be True or False"),
        (dict(), {**ON, "precision_weighted_refine": None}, "precision_weighted_refine'\\] must be True or False"),
        # everything that refuses multiview_refine refuses it too
        (dict(no_filter=True), ON, "no_filter"),
        (dict(reproj_thresh=0.0), ON, "reproj_thresh must be > 0"),
        (dict(nns_per_ref=1), ON, "nns_per_ref must be at least 2"),
        (dict(triangulation_mode="dense", stream_output=True), ON, "stream_output"),
        (dict(triangulation_mode="dense"), {**ON, "dense_tile_segments": True}, "dense_tile_segments"),
        (dict(), {**ON, "exchange_records": "ply"}, "exchange_records"),
    ]
    for kw, exp, text in refused:
        with pytest.raises(ValueError, match=text):
            lfd.DensePipelineConfig(output_path="a.ply", experimental=exp, **kw)
    for kw in (dict(no_filter=True), dict(nns_per_ref=1), dict(triangulation_mode="dense", stream_output=True)):
        assert lfd.DensePipelineConfig(output_path="a.ply", experimental={"precision_weighted_refine": False}, **kw).problem() is None


def test_the_cli_flag_reaches_the_configuration():
    ap = densify.build_argparser()
    args = ap.parse_args(["--scene_root", "x", "--multiview_refine", "--precision_weighted_refine"])
    assert args.precision_weighted_refine is True
    assert densify._experimental_from_args(args) == ON
    off = ap.parse_args(["--scene_root", "x"])
    assert off.precision_weighted_refine is False and densify._experimental_from_args(off) == {}
    cfg = lfd.DensePipelineConfig(output_path="a.ply", nns_per_ref=off.nns_per_ref, experimental=densify._experimental_from_args(args))
    assert cfg.exp("precision_weighted_refine") is True
    with pytest.raises(ValueError, match="multiview_refine"):
        lfd.DensePipelineConfig(output_path="a.ply", experimental=densify._experimental_from_args(ap.parse_args(["--scene_root", "x",
                                                                                                                  "--precision_weighted_refine"])))


class AskedMatcher(synthetic.SyntheticMatcher):
    """Records what the driver asks of it."""

    def set_precision(self, on):
        self.asked = getattr(self, "asked", []) + [bool(on)]
        super().set_precision(on)


def test_with_the_knob_off_the_matcher_is_never_asked_for_precision_and_no_new_code_runs(scene):
    m = AskedMatcher(scene["cams"], setting="turbo", **HETERO)
    with recorded_refines() as seen:
        res = cycle_scene.run(scene, m, "off.ply", triangulation_mode="sampled", experimental={"multiview_refine": True})
    assert m.asked == [False] and res.xyz.shape[0] > 1000
    assert seen and not any(s["precision"] or s["planes"] for s in seen) and all(s["n_counters"] == 2 for s in seen)
    tuples = m.match_grids_batch(None, None, keys=(scene["refs"][0], [int(v) for v in scene["nn"][scene["refs"][0]][:3]]))
    assert all(len(t) == 2 for t in tuples)


@pytest.mark.parametrize("mode,group", [("sampled", 1), ("dense", 1), ("dense", 2)])
def test_the_cloud_is_the_unweighted_run_s_cloud_with_other_positions(scene, mode, group, caplog):
    with cycle_scene.recorded_cells() as cells_off, recorded_refines() as seen_off:
        off = cycle_scene.run(scene, cycle_scene.matcher_for(scene, **HETERO), "unw.ply", triangulation_mode=mode, refs_per_launch=group,
                              experimental={"multiview_refine": True})
    with caplog.at_level(logging.INFO, logger="lfd_densify"), cycle_scene.recorded_cells() as cells_on, recorded_refines() as seen:
        on = cycle_scene.run(scene, cycle_scene.matcher_for(scene, **HETERO), "w.ply", triangulation_mode=mode, refs_per_launch=group,
                             experimental=ON)
    n = len(scene["refs"])
    assert len(cells_off) == n and cells_on == cells_off                         # the same (cell, slot) per reference: no count, no draw changed
    assert all(s["precision"] and s["planes"] and s["n_counters"] == 3 for s in seen) and len(seen) == len(seen_off)
    status, st_off = joined(seen, "status"), joined(seen_off, "status")
    xyz_in = joined(seen, "xyz_in")                                             # the two-view cloud: what the knob-off runs emit
    assert on.xyz.shape == off.xyz.shape == xyz_in.shape and np.array_equal(on.points_per_reference, off.points_per_reference)
    assert np.array_equal(bits(xyz_in), bits(joined(seen_off, "xyz_in"))) and np.array_equal(bits(on.xyz), bits(joined(seen, "xyz_out")))
    assert np.array_equal(bits(on.rgb), bits(off.rgb))
    assert np.array_equal(status & 0x3f, st_off & 0x7f)                         # the candidates are the unweighted run's
    accepted, weighted = (status & 0x80) != 0, (status & 0x40) != 0
    assert np.array_equal(weighted, (status & 0x3f) != 0)                       # the analytic planes are valid everywhere
    assert np.array_equal((bits(on.xyz) != bits(xyz_in)).any(axis=1), accepted)
    acc_off = (st_off & 0x80) != 0
    assert np.array_equal(bits(on.err)[~accepted & ~acc_off], bits(off.err)[~accepted & ~acc_off]) and (on.err <= np.float32(0.8)).all()
    fallback = ((status & 0x3f) != 0) & ~accepted
    print(f"{mode} x{group}: {xyz_in.shape[0]} points, {int(accepted.sum())} refined, {int(fallback.sum())} fallen back, {int(weighted.sum())} weighted")
    assert accepted.sum() > 0.3 * xyz_in.shape[0] and fallback.sum() > 0
    assert (bits(on.xyz) != bits(off.xyz)).any(axis=1).sum() > 0.3 * xyz_in.shape[0]         # the weights move points
    lines = [r.getMessage() for r in caplog.records if "Precision-weighted re-triangulation" in r.getMessage()]
    assert lines == [f"Precision-weighted re-triangulation: {int(accepted.sum())} points refined, {int(fallback.sum())} confirmed points kept their "
                     f"two-view position, {int(weighted.sum())} points solved with weighted rows"]


@pytest.mark.parametrize("mode,extra", [("sampled", {"min_support_views": 1}), ("dense", {"cycle_thresh_px": 1.0})], ids=["support_sampled", "cycle_dense"])
def test_it_combines_with_the_support_filter_and_the_cycle_gate(scene, mode, extra):
    with cycle_scene.recorded_cells() as cells_off:
        unw = cycle_scene.run(scene, cycle_scene.matcher_for(scene, **HETERO), "u.ply", triangulation_mode=mode,
                              experimental={"multiview_refine": True, **extra})
    with cycle_scene.recorded_cells() as cells_on, recorded_refines() as seen:
        w = cycle_scene.run(scene, cycle_scene.matcher_for(scene, **HETERO), "w.ply", triangulation_mode=mode, experimental={**ON, **extra})
    assert cells_on == cells_off and w.xyz.shape == unw.xyz.shape and w.xyz.shape[0] > 300
    assert np.array_equal(w.points_per_reference, unw.points_per_reference) and np.array_equal(bits(w.rgb), bits(unw.rgb))
    status = joined(seen, "status")
    assert all(s["precision"] for s in seen) and ((status & 0xc0) == 0xc0).sum() > 100
    if "min_support_views" in extra:
        assert ((status & 0x3f) >= 1).all()                                  # what the filter kept has a candidate, by definition


class NoPrecisionMatcher:
    """An injected matcher of the time before the planes: it declares nothing."""
    sample_thresh = 0.9
    w_resized = h_resized = 64


class ForgetfulMatcher(synthetic.SyntheticMatcher):
    """Declares the planes and hands out none."""

    def match_grids_batch(self, imA, imB_list, keys=None):
        return [t[:2] for t in super().match_grids_batch(imA, imB_list, keys=keys)]


def test_a_matcher_without_the_planes_is_refused_and_one_that_forgets_them_raises(scene):
    with pytest.raises(ValueError, match="does not declare supports_precision"):
        cycle_scene.run(scene, NoPrecisionMatcher(), "no.ply", experimental=ON)
    with pytest.raises(RuntimeError, match="returned no precision plane"):
        cycle_scene.run(scene, ForgetfulMatcher(scene["cams"], setting="turbo", **HETERO), "forget.ply", experimental=ON)
