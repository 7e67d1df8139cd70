"""The pair coverage of tests/test_config_matrix.py for the connected-component filter's two knobs, in the style of
tests/test_pose_config_matrix.py: each knob alone, the two together ("x:cmp": the filter switched on the only way it can be) against every
setting of that table - and against each other - either works, and then the pipeline gives the point sequence of the same run without the
knobs (the filter is a stage of densify.py behind the pipeline, which sees the knobs and does nothing with them), or is refused with a
message (DensePipelineConfig.problem()), at construction and by the driver alike.  Host backend; same scene, same matcher."""
import os

import numpy as np
import pytest

import lichtfeld_densification_plugin_amd as lfd
from lichtfeld_densification_plugin_amd.core import pipeline as pl
from test_config_matrix import OPTIONS, _Replay, scene  # noqa: F401  (the fixture)

COMPONENT = {
    "x:cmp": {"min_component_points": 20, "component_radius": 0.05},
    "x:cmp_points": {"min_component_points": 20},
    "x:cmp_radius": {"component_radius": 0.05},
}
ALL = {**OPTIONS, **COMPONENT}


def _kwargs(names, out):
    kw = dict(output_path=out, nns_per_ref=2, seed=5, viz_interval=0, matches_per_ref=1200, pack_workers=1, backend="host", experimental={})
    for n in names:
        if n in COMPONENT:
            kw["experimental"].update(COMPONENT[n])
            continue
        field, value = ALL[n]
        if n.startswith("x:"):
            kw["experimental"][field] = value
        else:
            kw[field] = value
    return kw


def _run(scene, kw):  # noqa: F811
    cfg = lfd.DensePipelineConfig(**kw)
    return pl.run_dense_pipeline(scene["cams"], scene["refs"], scene["nn"], cfg, matcher=_Replay(scene["table"]))


def _check_pair(scene, a, b, plain):  # noqa: F811
    names = tuple(sorted({a, b}))
    out = os.path.join(scene["tmp"], "cmp_" + "_".join(n.replace(":", "") for n in names), "out.ply")
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
    base = tuple(n for n in names if n not in COMPONENT)
    if base not in plain:
        plain[base] = _run(scene, _kwargs(base, os.path.join(scene["tmp"], "cmpplain_" + "_".join(n.replace(":", "") for n in base), "out.ply")))
    want = plain[base]
    np.testing.assert_array_equal(res.points_per_reference, want.points_per_reference)
    np.testing.assert_array_equal(res.xyz, want.xyz)
    np.testing.assert_array_equal(res.rgb, want.rgb)
    np.testing.assert_array_equal(res.err, want.err)
    return "ran"


def test_every_pair_with_a_component_setting_runs_as_the_plain_sequence_or_is_refused_with_a_message(scene):  # noqa: F811
    outcomes, plain = {}, {}
    for a in sorted(COMPONENT):
        for b in sorted(ALL):
            outcomes[(a, b)] = _check_pair(scene, a, b, plain)
    ran = sum(1 for v in outcomes.values() if v == "ran")
    refused = sum(1 for v in outcomes.values() if v == "refused")
    assert ran >= 10 and refused >= 40, (ran, refused)
    # the verdicts spelled out, so that a rule that silently disappears is noticed
    assert outcomes[("x:cmp", "x:cmp")] == "ran"
    for b in ("dense", "no_filter", "cap", "voxel"):
        assert outcomes[("x:cmp", b)] == "ran", b
    for b in ("stream", "x:segments", "x:ply_records"):
        assert outcomes[("x:cmp", b)] == "refused", b
    # a knob alone is refused - the filter without its radius, the radius without the filter - whatever it is paired with, except with the other
    assert outcomes[("x:cmp_points", "x:cmp_radius")] == "ran" and outcomes[("x:cmp_radius", "x:cmp_points")] == "ran"
    for knob in ("x:cmp_points", "x:cmp_radius"):
        assert outcomes[(knob, knob)] == "refused"
        for b in OPTIONS:
            assert outcomes[(knob, b)] == "refused", (knob, b)
        assert outcomes[("x:cmp", knob)] == "ran"
