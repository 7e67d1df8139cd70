"""The pair coverage of tests/test_config_matrix.py for the epipolar audit's knobs: every pair of an audit setting with every
setting of that table - and with each other - either works together, and then gives the point sequence of the same run without the audit
(the statistics are read-only: they move no point) with the run's histograms beside it, or is refused with a message
(DensePipelineConfig.problem()), at construction and by the driver alike.  Host backend; same scene, same matcher."""
import os

import numpy as np
import pytest

import lichtfeld_densification_plugin_amd as lfd
from lichtfeld_densification_plugin_amd.core import pipeline as pl
from test_config_matrix import OPTIONS, _Replay, scene  # noqa: F401  (the fixture)

AUDIT = {
    "x:audit": ("epipolar_audit", "report"),
    "x:audit_cert": ("audit_certainty", 0.7),
    "x:audit_min": ("audit_min_samples", 16),
    "x:audit_warn": ("audit_warn_px", 1.5),
    "x:audit_maps": ("audit_maps_dir", "epi"),
}
ALL = {**OPTIONS, **AUDIT}


def _kwargs(names, out):
    kw = dict(output_path=out, nns_per_ref=2, seed=5, viz_interval=0, matches_per_ref=1200, pack_workers=1, backend="host", experimental={})
    for n in names:
        field, value = ALL[n]
        if n.startswith("x:"):
            kw["experimental"][field] = value
        else:
            kw[field] = value
    return kw


def _run(scene, kw):
    cfg = lfd.DensePipelineConfig(**kw)
    return pl.run_dense_pipeline(scene["cams"], scene["refs"], scene["nn"], cfg, matcher=_Replay(scene["table"]))


def _check_pair(scene, a, b, plain):
    names = tuple(sorted({a, b}))
    out = os.path.join(scene["tmp"], "audit_" + "_".join(n.replace(":", "") for n in names), "out.ply")
    kw = _kwargs(names, out)
    probe = lfd.DensePipelineConfig(output_path="probe.ply")
    for k, v in kw.items():
        setattr(probe, k, v)
    why = probe.problem()
    if why is not None:
        with pytest.raises(ValueError) as e1:
            lfd.DensePipelineConfig(**kw)
        assert str(e1.value) == why
        with pytest.raises(ValueError) as e2:
            pl.run_dense_pipeline(scene["cams"], scene["refs"], scene["nn"], probe, matcher=_Replay(scene["table"]))
        assert why in str(e2.value)
        return "refused"
    res = _run(scene, kw)
    base = tuple(n for n in names if n not in AUDIT)
    if base not in plain:
        plain[base] = _run(scene, _kwargs(base, os.path.join(scene["tmp"], "auditplain_" + "_".join(n.replace(":", "") for n in base), "out.ply")))
    want = plain[base]
    np.testing.assert_array_equal(res.points_per_reference, want.points_per_reference)
    np.testing.assert_array_equal(res.xyz, want.xyz)
    np.testing.assert_array_equal(res.rgb, want.rgb)
    np.testing.assert_array_equal(res.err, want.err)
    assert want.epipolar_audit is None and res.epipolar_audit is not None
    rows = res.epipolar_audit["rows"]
    assert len(rows) >= len(scene["refs"]) and all(len(r) == 66 and sum(r[2:]) == r[0] for r in rows.values())
    assert sum(r[0] for r in rows.values()) > 0 and len(res.epipolar_audit["report"]["pairs"]) == len(rows)
    assert (res.epipolar_audit["maps"] is not None) == ("x:audit_maps" in names)
    return "ran"


def test_every_pair_with_an_audit_setting_runs_as_the_plain_sequence_or_is_refused_with_a_message(scene):  # noqa: F811
    outcomes, plain = {}, {}
    for a in sorted(AUDIT):
        for b in sorted(ALL):
            outcomes[(a, b)] = _check_pair(scene, a, b, plain)
    ran = sum(1 for v in outcomes.values() if v == "ran")
    refused = sum(1 for v in outcomes.values() if v == "refused")
    assert ran >= 20 and refused >= 40, (ran, refused)
    # a few verdicts spelled out, so that a rule that silently disappears is noticed
    assert outcomes[("x:audit", "x:audit")] == "ran"
    for b in ("dense", "no_filter", "cap", "voxel"):
        assert outcomes[("x:audit", b)] == "ran", b
    for b in ("stream", "x:segments", "x:ply_records"):
        assert outcomes[("x:audit", b)] == "refused", b
    for knob in ("x:audit_cert", "x:audit_min", "x:audit_warn", "x:audit_maps"):
        assert outcomes[("x:audit", knob)] == "ran"
        assert outcomes[(knob, knob)] == "refused" and outcomes[(knob, "dense")] == "refused"       # a knob without the audit
