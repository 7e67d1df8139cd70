"""The pair coverage of tests/test_config_matrix.py for the far-field shell's knobs: every pair of a far-shell setting with
every setting of that table - and with each other - either works together, and then gives the point sequence of the same run without the
shell (the statistics are read-only: they move no point) with the run's direction table beside it, or is refused with a message
(DensePipelineConfig.problem()), at construction and by the driver alike.  Host backend; same scene, same matcher."""
import os

import numpy as np
import pytest

import lichtfeld_densification_plugin_amd as lfd
from lichtfeld_densification_plugin_amd.core import pipeline as pl
from test_config_matrix import OPTIONS, _Replay, scene  # noqa: F401  (the fixture)

FAR = {
    "x:far_file": ("far_shell", "file"),
    "x:far_merge": ("far_shell", "merge"),
    "x:far_cells": ("far_shell_cells", 64),
    "x:far_views": ("far_min_views", 1),
}
ALL = {**OPTIONS, **FAR}


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
    out = os.path.join(scene["tmp"], "far_" + "_".join(n.replace(":", "") for n in names), "out.ply")
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
    base = tuple(n for n in names if n not in FAR)
    if base not in plain:
        plain[base] = _run(scene, _kwargs(base, os.path.join(scene["tmp"], "farplain_" + "_".join(n.replace(":", "") for n in base), "out.ply")))
    want = plain[base]
    np.testing.assert_array_equal(res.points_per_reference, want.points_per_reference)
    np.testing.assert_array_equal(res.xyz, want.xyz)
    np.testing.assert_array_equal(res.rgb, want.rgb)
    np.testing.assert_array_equal(res.err, want.err)
    S = 64 if "x:far_cells" in names else 256
    assert want.far_shell is None and res.far_shell is not None and tuple(res.far_shell["table"].shape) == (6 * S * S, 7)
    assert sum(res.far_shell["far_cells"].values()) == int(res.far_shell["table"][:, 6].sum())
    return "ran"


def test_every_pair_with_a_far_shell_setting_runs_as_the_plain_sequence_or_is_refused_with_a_message(scene):  # noqa: F811
    outcomes, plain = {}, {}
    for a in sorted(FAR):
        for b in sorted(ALL):
            outcomes[(a, b)] = _check_pair(scene, a, b, plain)
    ran = sum(1 for v in outcomes.values() if v == "ran")
    refused = sum(1 for v in outcomes.values() if v == "refused")
    assert ran >= 20 and refused >= 40, (ran, refused)
    # a few verdicts spelled out, so that a rule that silently disappears is noticed
    assert outcomes[("x:far_file", "x:far_file")] == "ran" and outcomes[("x:far_merge", "x:far_merge")] == "ran"
    assert outcomes[("x:far_file", "dense")] == "ran" and outcomes[("x:far_merge", "cap")] == "ran" and outcomes[("x:far_file", "voxel")] == "ran"
    assert outcomes[("x:far_file", "x:far_cells")] == "ran" and outcomes[("x:far_merge", "x:far_views")] == "ran"
    assert outcomes[("x:far_file", "x:far_merge")] == "ran"                        # (one key: the later value holds)
    assert outcomes[("x:far_cells", "x:far_cells")] == "refused" and outcomes[("x:far_views", "dense")] == "refused"      # a knob without the shell
    for far in ("x:far_file", "x:far_merge"):
        assert outcomes[(far, "no_filter")] == "refused" and outcomes[(far, "stream")] == "refused"
        assert outcomes[(far, "x:segments")] == "refused" and outcomes[(far, "x:ply_records")] == "refused"
