"""The depth-uncertainty gate in the driver, on the host backend (core/types.py, core/hotpath.py, core/pipeline.py, densify.py) with the analytic
matcher: the knob-on cloud is the knob-off cloud restricted by a mask - same order, same bits - in sampled mode and in dense mode with one and
two references per launch; it runs last, behind the support filter and the (weighted) re-triangulation, whose status it is handed; it combines
with the forward-backward gate; the refusals of ``problem()``; the CLI flags; an injected matcher without the planes is refused, one that
declared them and returns none raises, and with the knob off the matcher is never asked for them on its account."""
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
ISO = 0.5
HETERO = dict(noise_model="hetero")


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    return cycle_scene.make_scene(str(tmp_path_factory.mktemp("sigma_scene")), n_cams=4)      # three references, each with the three other cameras


@contextlib.contextmanager
def recorded_gates():
    """Every call of the twin's depth_sigma_filter a run makes, in order: its input, sigma_rel of the input and the arguments.  Calls of the
    other two stages are noted in ``order``."""
    seen, order = [], []
    plain, plain_sup, plain_ref = hb.HostDensifier.depth_sigma_filter, hb.HostDensifier.support_filter, hb.HostDensifier.refine_multiview

    def gate(self, batch, out, max_rel_sigma, iso_sigma_px=0.0, refine_status=None, support_thresh_px=0.0, with_sigma=False, into=None):
        order.append("gate")
        res, sigma, sigma_out = plain(self, batch, out, max_rel_sigma, iso_sigma_px=iso_sigma_px, refine_status=refine_status,
                                      support_thresh_px=support_thresh_px, with_sigma=True, into=into)
        seen.append(dict(xyz_in=out.xyz.numpy().copy(), rgb_in=out.rgb.numpy().copy(), err_in=out.err.numpy().copy(), sigma=sigma.numpy().copy(),
                         max=float(max_rel_sigma), iso=float(iso_sigma_px), tau=float(support_thresh_px), planes=batch.precision is not None,
                         status=None if refine_status is None else refine_status.numpy().copy(), kept=int(res.count),
                         offsets_in=np.asarray(out.ref_offsets).copy()))
        return (res, sigma, sigma_out) if with_sigma else res

    def sup(self, *a, **kw):
        order.append("support")
        return plain_sup(self, *a, **kw)

    def ref(self, *a, **kw):
        order.append("refine")
        return plain_ref(self, *a, **kw)

    hb.HostDensifier.depth_sigma_filter, hb.HostDensifier.support_filter, hb.HostDensifier.refine_multiview = gate, sup, ref
    try:
        yield seen, order
    finally:
        hb.HostDensifier.depth_sigma_filter, hb.HostDensifier.support_filter, hb.HostDensifier.refine_multiview = plain, plain_sup, plain_ref


def joined(seen, name):
    return np.concatenate([s[name] for s in seen])


_thresholds = {}


def median_sigma(scene, mode, extra, iso):
    """A threshold that keeps about half of a run's points: the median sigma of a run whose gate keeps every finite one."""
    key = (mode, tuple(sorted(extra.items())), iso)
    if key not in _thresholds:
        with recorded_gates() as (seen, _order):
            cycle_scene.run(scene, cycle_scene.matcher_for(scene, **HETERO), "probe.ply", triangulation_mode=mode,
                            experimental={"max_depth_sigma_rel": 1e30, "match_sigma_px": iso, **extra})
        sg = joined(seen, "sigma")
        _thresholds[key] = float(np.median(sg[np.isfinite(sg)]))
    return _thresholds[key]


def test_the_knobs_are_experimental_off_by_default_and_validated():
    assert EXPERIMENTAL_DEFAULTS["max_depth_sigma_rel"] == 0.0 and EXPERIMENTAL_DEFAULTS["match_sigma_px"] == 0.0
    cfg = lfd.DensePipelineConfig(output_path="a.ply")
    assert cfg.exp("max_depth_sigma_rel") == 0.0 and cfg.exp("match_sigma_px") == 0.0
    on = {"max_depth_sigma_rel": 0.05}
    for mode in ("sampled", "dense"):
        for backend in ("device", "host"):
            for extra in ({}, {"match_sigma_px": 0.5}, {"min_support_views": 1}, {"multiview_refine": True},
                          {"multiview_refine": True, "precision_weighted_refine": True}, {"cycle_thresh_px": 1.0}):
                assert lfd.DensePipelineConfig(output_path="a.ply", triangulation_mode=mode, backend=backend, experimental={**on, **extra}).problem() is None
    assert lfd.DensePipelineConfig(output_path="a.ply", stream_output=True, experimental=on).problem() is None          # sampled mode streams arrays
    assert lfd.DensePipelineConfig(output_path="a.ply", no_filter=True, nns_per_ref=1, experimental=on).problem() is None
    refused = [
        (dict(), {"max_depth_sigma_rel": -0.01}, "max_depth_sigma_rel'\\] must be finite and >= 0"),
        (dict(), {"max_depth_sigma_rel": float("inf")}, "max_depth_sigma_rel'\\] must be finite and >= 0"),
        (dict(), {"max_depth_sigma_rel": float("nan")}, "max_depth_sigma_rel'\\] must be finite and >= 0"),
        (dict(), {"max_depth_sigma_rel": "tight"}, "max_depth_sigma_rel'\\] must be a number"),
        (dict(), {"max_depth_sigma_rel": None}, "max_depth_sigma_rel'\\] must be a number"),
        (dict(), {**on, "match_sigma_px": -1.0}, "match_sigma_px'\\] must be finite and >= 0"),
        (dict(), {**on, "match_sigma_px": float("inf")}, "match_sigma_px'\\] must be finite and >= 0"),
        (dict(), {**on, "match_sigma_px": float("nan")}, "match_sigma_px'\\] must be finite and >= 0"),
        (dict(), {**on, "match_sigma_px": "half"}, "match_sigma_px'\\] must be a number"),
        (dict(), {"match_sigma_px": 0.5}, "needs experimental\\['max_depth_sigma_rel'\\] > 0"),
        (dict(), {"match_sigma_px": 0.5, "max_depth_sigma_rel": 0.0}, "needs experimental\\['max_depth_sigma_rel'\\] > 0"),
        (dict(triangulation_mode="dense", stream_output=True), on, "max_depth_sigma_rel'\\] filters points held as arrays"),
        (dict(triangulation_mode="dense"), {**on, "dense_tile_segments": True}, "max_depth_sigma_rel'\\] needs the ordered dense result"),
        (dict(), {**on, "exchange_records": "ply"}, "max_depth_sigma_rel'\\] filters f32 rows"),
    ]
    for kw, exp, text in refused:
        with pytest.raises(ValueError, match=text):
            lfd.DensePipelineConfig(output_path="a.ply", experimental=exp, **kw)
    for kw in (dict(triangulation_mode="dense", stream_output=True), dict(experimental={"exchange_records": "ply"})):
        exp = {**kw.pop("experimental", {}), "max_depth_sigma_rel": 0.0}
        assert lfd.DensePipelineConfig(output_path="a.ply", experimental=exp, **kw).problem() is None


def test_the_cli_flags_reach_the_configuration():
    ap = densify.build_argparser()
    args = ap.parse_args(["--scene_root", "x", "--max_depth_sigma_rel", "0.05", "--match_sigma_px", "0.7"])
    assert args.max_depth_sigma_rel == 0.05 and args.match_sigma_px == 0.7
    assert densify._experimental_from_args(args) == {"max_depth_sigma_rel": 0.05, "match_sigma_px": 0.7}
    only = ap.parse_args(["--scene_root", "x", "--max_depth_sigma_rel", "0.1"])
    assert densify._experimental_from_args(only) == {"max_depth_sigma_rel": 0.1}
    off = ap.parse_args(["--scene_root", "x"])
    assert off.max_depth_sigma_rel == 0.0 and off.match_sigma_px == 0.0 and densify._experimental_from_args(off) == {}
    cfg = lfd.DensePipelineConfig(output_path="a.ply", experimental=densify._experimental_from_args(args))
    assert cfg.exp("max_depth_sigma_rel") == 0.05 and cfg.exp("match_sigma_px") == 0.7
    with pytest.raises(ValueError, match="max_depth_sigma_rel"):
        lfd.DensePipelineConfig(output_path="a.ply", experimental=densify._experimental_from_args(ap.parse_args(["--scene_root", "x", "--match_sigma_px",
                                                                                                                  "0.5"])))


class AskedMatcher(synthetic.SyntheticMatcher):
    """Records what the driver asks of it."""

    def set_precision(self, on):
        self.asked = getattr(self, "asked", []) + [bool(on)]
        super().set_precision(on)


def test_with_the_knob_off_the_matcher_is_never_asked_and_no_new_code_runs(scene):
    m = AskedMatcher(scene["cams"], setting="turbo", **HETERO)
    with recorded_gates() as (seen, order):
        res = cycle_scene.run(scene, m, "off.ply", triangulation_mode="sampled", experimental={"multiview_refine": True})
    assert m.asked == [False] and res.xyz.shape[0] > 1000 and not seen and "gate" not in order and "refine" in order
    # the isotropic form does not ask either; the plane form does
    m = AskedMatcher(scene["cams"], setting="turbo", **HETERO)
    with recorded_gates() as (seen, _order):
        cycle_scene.run(scene, m, "iso.ply", experimental={"max_depth_sigma_rel": 1e30, "match_sigma_px": ISO})
    assert m.asked == [False] and seen and not any(s["planes"] for s in seen) and all(s["iso"] == ISO for s in seen)
    m = AskedMatcher(scene["cams"], setting="turbo", **HETERO)
    with recorded_gates() as (seen, _order):
        cycle_scene.run(scene, m, "planes.ply", experimental={"max_depth_sigma_rel": 1e30})
    assert m.asked == [True] and seen and all(s["planes"] and s["iso"] == 0.0 for s in seen)


@pytest.mark.parametrize("iso", [ISO, 0.0], ids=["iso", "planes"])
@pytest.mark.parametrize("mode,group", [("sampled", 1), ("dense", 1), ("dense", 2)])
def test_the_cloud_is_the_knob_off_cloud_restricted_by_a_mask(scene, mode, group, iso, caplog):
    mx = median_sigma(scene, mode, {}, iso)
    with cycle_scene.recorded_cells() as cells_off:
        off = cycle_scene.run(scene, cycle_scene.matcher_for(scene, **HETERO), "off.ply", triangulation_mode=mode, refs_per_launch=group)
    with caplog.at_level(logging.INFO, logger="lfd_densify"), cycle_scene.recorded_cells() as cells_on, recorded_gates() as (seen, order):
        on = cycle_scene.run(scene, cycle_scene.matcher_for(scene, **HETERO), "on.ply", triangulation_mode=mode, refs_per_launch=group,
                             experimental={"max_depth_sigma_rel": mx, "match_sigma_px": iso})
    # what reached the gate is the knob-off run's cloud, bit for bit: no count and no draw of the sampling stream changed ...
    for name in ("xyz", "rgb", "err"):
        assert np.array_equal(bits(joined(seen, name + "_in")), bits(getattr(off, name))), name
    sg = joined(seen, "sigma")
    keep = sg <= np.float32(mx)
    assert all(s["max"] == mx and s["iso"] == iso and s["status"] is None and s["tau"] == 0.0 for s in seen) and set(order) == {"gate"}
    # ... and what the run emits is that cloud under the mask, in order
    assert 0.3 * sg.size < keep.sum() < 0.7 * sg.size
    for name in ("xyz", "rgb", "err"):
        assert np.array_equal(bits(getattr(on, name)), bits(getattr(off, name))[keep]), name
    per_ref = np.add.reduceat(keep, np.concatenate([[0], np.cumsum(off.points_per_reference)[:-1]])) if sg.size else []
    assert np.array_equal(on.points_per_reference, per_ref)
    assert len(cells_off) == len(scene["refs"]) and len(cells_on) >= len(cells_off)
    lines = [r.getMessage() for r in caplog.records if "Depth-uncertainty gate" in r.getMessage()]
    noise = f"isotropic match noise {ISO:g} px" if iso else "the matcher's precision planes"
    assert lines == [f"Depth-uncertainty gate: relative depth sigma at most {mx:g} ({noise}), {sg.size} points in, {int(keep.sum())} kept"]


@pytest.mark.parametrize("mode,extra", [("sampled", {"min_support_views": 1}), ("dense", {"multiview_refine": True}),
                                        ("sampled", {"multiview_refine": True, "precision_weighted_refine": True, "min_support_views": 1}),
                                        ("dense", {"cycle_thresh_px": 1.0})], ids=["support", "refine", "support_wrefine", "cycle"])
def test_it_runs_last_and_combines_with_the_other_stages(scene, mode, extra, caplog):
    iso = 0.0 if extra.get("precision_weighted_refine") else ISO
    mx = median_sigma(scene, mode, extra, iso)
    off = cycle_scene.run(scene, cycle_scene.matcher_for(scene, **HETERO), "off.ply", triangulation_mode=mode, experimental=extra)
    with caplog.at_level(logging.INFO, logger="lfd_densify"), recorded_gates() as (seen, order):
        on = cycle_scene.run(scene, cycle_scene.matcher_for(scene, **HETERO), "on.ply", triangulation_mode=mode,
                             experimental={"max_depth_sigma_rel": mx, "match_sigma_px": iso, **extra})
    for name in ("xyz", "rgb", "err"):                                       # the other stages' result reaches the gate untouched
        assert np.array_equal(bits(joined(seen, name + "_in")), bits(getattr(off, name))), name
    keep = joined(seen, "sigma") <= np.float32(mx)
    assert 0 < keep.sum() < keep.size and np.array_equal(bits(on.xyz), bits(off.xyz)[keep]) and np.array_equal(bits(on.rgb), bits(off.rgb)[keep])
    stages = [s for s in ("support", "refine") if (s == "support" and extra.get("min_support_views")) or (s == "refine" and extra.get("multiview_refine"))]
    per_call = stages + ["gate"]
    assert order == per_call * (len(order) // len(per_call)) and len(seen) >= 1          # support filter, then refine, then the gate
    if extra.get("multiview_refine"):
        st = joined(seen, "status")
        assert all(s["tau"] == 1.6 for s in seen) and ((st & 0x80) != 0).sum() > 100       # the refinement's status, its threshold (2 x reproj_thresh)
    else:
        assert all(s["status"] is None for s in seen)
    if extra.get("min_support_views"):
        sup = [r.getMessage() for r in caplog.records if "Multi-view support filter" in r.getMessage()]
        assert len(sup) == 1 and f"{keep.size} dropped" not in sup[0]
        n_in = int(sup[0].split(" points in")[0].split()[-1])
        assert n_in - int(sup[0].split(" dropped")[0].split()[-1]) == keep.size           # the filter's own totals do not see the gate


class NoPrecisionMatcher:
    """An injected matcher of the time before the planes: it declares nothing."""
    sample_thresh = 0.9
    w_resized = h_resized = 64


class ForgetfulMatcher(synthetic.SyntheticMatcher):
    """Declares the planes and hands out none."""

    def match_grids_batch(self, imA, imB_list, keys=None):
        return [t[:2] for t in super().match_grids_batch(imA, imB_list, keys=keys)]


def test_a_matcher_without_the_planes_is_refused_and_one_that_forgets_them_raises(scene):
    with pytest.raises(ValueError, match="max_depth_sigma_rel.*does not declare supports_precision"):
        cycle_scene.run(scene, NoPrecisionMatcher(), "no.ply", experimental={"max_depth_sigma_rel": 0.05})
    with pytest.raises(RuntimeError, match="max_depth_sigma_rel.*returned no precision plane"):
        cycle_scene.run(scene, ForgetfulMatcher(scene["cams"], setting="turbo", **HETERO), "forget.ply", experimental={"max_depth_sigma_rel": 0.05})
