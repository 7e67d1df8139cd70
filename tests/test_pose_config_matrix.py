"""The pair coverage of tests/test_config_matrix.py for the pose refinement's five knobs: every pair of a pose setting with
every setting of that table - and with each other - either works together, and then gives the point sequence of the same run without the
pose setting (the statistics are read-only: they move no point; pose_corrections acts on the records in densify.py, in front of the
pipeline, which sees the knob and does nothing with it) with the run's normal equations beside it, or is refused with a message
(DensePipelineConfig.problem()), at construction and by the driver alike.  Host backend; same scene, same matcher."""
import os

import numpy as np
import pytest

import lichtfeld_densification_plugin_amd as lfd
from lichtfeld_densification_plugin_amd.core import pipeline as pl
from test_config_matrix import OPTIONS, _Replay, scene  # noqa: F401  (the fixture)

POSE = {
    "x:pose": ("pose_refine", "report"),
    "x:pose_cert": ("pose_certainty", 0.7),
    "x:pose_px": ("pose_inlier_px", 4.0),
    "x:pose_min": ("pose_min_samples", 16),
    "x:pose_corr": ("pose_corrections", "earlier.ply.poses.json"),
}
ALL = {**OPTIONS, **POSE}


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
    out = os.path.join(scene["tmp"], "pose_" + "_".join(n.replace(":", "") for n in names), "out.ply")
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
    base = tuple(n for n in names if n not in POSE)
    if base not in plain:
        plain[base] = _run(scene, _kwargs(base, os.path.join(scene["tmp"], "poseplain_" + "_".join(n.replace(":", "") for n in base), "out.ply")))
    want = plain[base]
    np.testing.assert_array_equal(res.points_per_reference, want.points_per_reference)
    np.testing.assert_array_equal(res.xyz, want.xyz)
    np.testing.assert_array_equal(res.rgb, want.rgb)
    np.testing.assert_array_equal(res.err, want.err)
    assert want.pose_refine is None and (res.pose_refine is not None) == ("x:pose" in names)
    if res.pose_refine is not None:
        rows = res.pose_refine["rows"]
        assert len(rows) >= len(scene["refs"]) and all(len(r) == 32 and r[31] == 0 and min(r[:4]) >= 0 for r in rows.values())
        assert sum(r[0] for r in rows.values()) > 0 and len(res.pose_refine["report"]["pairs"]) == len(rows)
        assert len(res.pose_refine["report"]["cameras"]) == len(scene["cams"])
    return "ran"


def test_every_pair_with_a_pose_setting_runs_as_the_plain_sequence_or_is_refused_with_a_message(scene):  # noqa: F811
    outcomes, plain = {}, {}
    for a in sorted(POSE):
        for b in sorted(ALL):
            outcomes[(a, b)] = _check_pair(scene, a, b, plain)
    ran = sum(1 for v in outcomes.values() if v == "ran")
    refused = sum(1 for v in outcomes.values() if v == "refused")
    assert ran >= 30 and refused >= 30, (ran, refused)
    # a few verdicts spelled out, so that a rule that silently disappears is noticed
    assert outcomes[("x:pose", "x:pose")] == "ran"
    for b in ("dense", "no_filter", "cap", "voxel"):
        assert outcomes[("x:pose", b)] == "ran", b
    for b in ("stream", "x:segments", "x:ply_records"):
        assert outcomes[("x:pose", b)] == "refused", b
    for knob in ("x:pose_cert", "x:pose_px", "x:pose_min"):
        assert outcomes[("x:pose", knob)] == "ran"
        assert outcomes[(knob, knob)] == "refused" and outcomes[(knob, "dense")] == "refused"       # a knob without the refinement
    # the corrections file is a knob of its own: a second run takes it with or without another refinement
    assert outcomes[("x:pose_corr", "x:pose_corr")] == "ran" and outcomes[("x:pose", "x:pose_corr")] == "ran"
    for b in ("dense", "stream", "no_filter"):
        assert outcomes[("x:pose_corr", b)] == "ran", b
