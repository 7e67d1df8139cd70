"""The pose refinement's solve and report (core/poses.py) on the CPU: the dequantisation of a hand-made row, a hand-made
two-camera system whose answer is known, the gauge columns as null vectors of the assembled matrix at consistent poses, a camera without a
usable pair, the warning about a step too large for one linear step, the JSON round trip, and apply_corrections with its refusals."""
import dataclasses
import json

import numpy as np
import pytest

import pose_scene as ps
from lichtfeld_densification_plugin_amd.core import colmap_io
from lichtfeld_densification_plugin_amd.core import poses as pose_report
from lichtfeld_densification_plugin_amd.core.types import CameraRecord
from test_pose_host import CERT, INLIER_PX, K, MIN_SAMPLES, PAIRS, WRONG, rig


def row_from(J, r, outliers=0, degenerate=0):
    """A table row from un-quantised samples J (n, 6), r (n,), quantised as the library does."""
    q = np.concatenate([np.rint(8.0 * np.asarray(J)), np.rint(1024.0 * np.asarray(r))[:, None]], axis=1).astype(np.int64)
    row = [len(q), outliers, degenerate, int((q[:, 6] ** 2).sum())] + [int((q[:, i] * q[:, 6]).sum()) for i in range(6)]
    row += [int((q[:, i] * q[:, j]).sum()) for i in range(6) for j in range(i, 6)]
    return row + [0]


def test_a_row_is_dequantised_by_64_and_8192():
    row = [5, 1, 2, 3 * 1048576] + [8192 * (i + 1) for i in range(6)] + [64 * (10 * i + j) for i in range(6) for j in range(i, 6)] + [77]
    H, g, rr = pose_report.pair_system(row)
    assert rr == 3.0 and g.tolist() == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
    assert all(H[i, j] == H[j, i] == 10 * min(i, j) + max(i, j) for i in range(6) for j in range(6))
    with pytest.raises(ValueError, match="32 entries"):
        pose_report.pair_system(row[:-1])


def test_a_hand_made_system_gives_the_least_squares_step_in_the_gauge_free_space():
    """Two cameras at (0, 0, 0) and (1, 0, 0), identity rotations, and samples r = J x for a known relative twist x: the step's relative
    twist delta_B - Ad delta_A must equal -x in every direction the samples determine, and the step is orthogonal to the seven gauge columns."""
    rng = np.random.default_rng(7)
    J = rng.normal(0.0, 200.0, (4000, 6))
    J[:, 3] = 0.0                                                      # tau along the baseline: the scale direction, which no sample sees
    x = np.array([2e-3, -1e-3, 1.5e-3, 0.0, 2e-3, -3e-3])
    r = J @ x
    recs = [CameraRecord.from_krt(1, np.eye(3), np.eye(3), np.zeros(3), 10, 10), CameraRecord.from_krt(2, np.eye(3), np.eye(3), [-1.0, 0.0, 0.0], 10, 10)]
    rows = {(1, 2): row_from(J, r)}
    poses = {int(c.uid): pose_report.pose_of(c) for c in recs}
    sol = pose_report.solve(rows, poses, 256)
    assert sol["uids"] == [1, 2] and sol["dropped"] == 0       # 12 parameters, 7 gauge, 5 determined: nothing is dropped
    delta = np.concatenate([sol["delta"][1], sol["delta"][2]])
    _a, _b, M, _H, _g, _rr, tn = sol["parts"][0]
    assert tn == 1.0
    rel = M @ delta
    assert np.abs(rel[[0, 1, 2, 4, 5]] + x[[0, 1, 2, 4, 5]]).max() <= 2e-5      # Jq = rint(8 J) on |J| ~ 200: a relative 3e-4 of |x| ~ 3e-3; rq: 1e-3 px / 200
    G = pose_report.gauge_columns([poses[1], poses[2]])
    assert np.abs(G.T @ delta).max() <= 1e-12
    rep = pose_report.build_report(rows, recs, 256, CERT, INLIER_PX)
    assert rep["pairs"][0]["predicted_rms_px"] < 1e-2 * rep["pairs"][0]["rms_px"] and rep["scene"]["usable_pairs"] == 1


@pytest.fixture(scope="module")
def true_rows():
    records = ps.cameras()
    return records, rig(records)[1]


def test_the_gauge_columns_are_null_vectors_of_the_assembled_matrix_at_consistent_poses(true_rows):
    """Exact matches, true records: H G = 0 up to the quantisation of J (steps of 1 / 8 against entries of 1e2 .. 1e3 px per radian, so a
    relative 1e-3 per sample at the most, and the errors of the samples do not add up coherently)."""
    records, rows = true_rows
    poses = {int(c.uid): pose_report.pose_of(c) for c in records}
    uids, H, g, parts = pose_report.assemble(rows, poses, MIN_SAMPLES)
    assert len(uids) == ps.N_CAMS and len(parts) == len(PAIRS)
    G = pose_report.gauge_columns([poses[u] for u in uids])
    G = G / np.linalg.norm(G, axis=0)
    top = np.linalg.eigvalsh(H)[-1]
    worst = np.abs(H @ G).max() / top
    print("|H G| / lambda_max =", worst)
    assert worst <= 1e-3
    Q2, Hr = pose_report.reduced(H, G)
    assert Q2.shape == (6 * ps.N_CAMS, 6 * ps.N_CAMS - 7) and np.abs(Q2.T @ G).max() <= 1e-12
    lam = np.linalg.eigvalsh(Hr)
    assert lam[0] >= 1e-6 * lam[-1]                                    # the scene fixes everything but the gauge


def test_a_camera_without_a_usable_pair_is_left_out_and_reported_unchanged(true_rows):
    records, rows = true_rows
    uid = lambda i: int(records[i].uid)                                # noqa: E731
    thin = {p: (list(r) if uid(7) not in p else [MIN_SAMPLES - 1] + list(r[1:])) for p, r in rows.items()}
    rep = pose_report.build_report(thin, records[:ps.N_CAMS], MIN_SAMPLES, CERT, INLIER_PX, {uid(i): f"view_{i}.png" for i in range(ps.N_CAMS)})
    assert rep["scene"]["cameras_left_out"] == [uid(7)] and rep["scene"]["cameras_corrected"] == ps.N_CAMS - 1
    last = [c for c in rep["cameras"] if c["uid"] == uid(7)][0]
    assert not last["corrected"] and last["qvec"] == last["input_qvec"] and last["tvec"] == last["input_tvec"] and last["usable_pairs"] == 0
    assert last["rotation_step_deg"] == 0.0 and last["name"] == "view_7.png"
    ignored = [tuple(p) for p in rep["scene"]["pairs_ignored"]]
    assert sorted(ignored) == sorted(p for p in rows if uid(7) in p) and len(ignored) >= 3
    assert all(p["usable"] == (uid(7) not in (p["reference_uid"], p["neighbour_uid"])) for p in rep["pairs"])
    # nothing usable at all: every camera is reported unchanged
    none = pose_report.build_report(rows, records[:ps.N_CAMS], 10 ** 9)
    assert none["scene"]["cameras_corrected"] == 0 and len(none["scene"]["cameras_left_out"]) == ps.N_CAMS and none["scene"]["rms_px"] is None


def test_the_report_and_its_round_trip():
    records = ps.cameras(WRONG)
    rows = rig(records)[1]
    names = {int(c.uid): f"view_{i:04d}.png" for i, c in enumerate(records)}
    rep = pose_report.build_report(rows, records[:ps.N_CAMS], MIN_SAMPLES, CERT, INLIER_PX, names)
    text = pose_report.to_json(rep)
    assert pose_report.to_json(pose_report.from_json(text)) == text and json.loads(text) == rep
    assert rep["knobs"] == {"pose_certainty": CERT, "pose_inlier_px": INLIER_PX, "pose_min_samples": MIN_SAMPLES}
    assert [c["name"] for c in rep["cameras"]] == [names[int(c.uid)] for c in records[:ps.N_CAMS]]
    assert not any("time" in k or "seconds" in k for k in text.split('"'))
    wrong = rep["cameras"][WRONG[0]]
    assert 0.35 < wrong["rotation_step_deg"] < 0.5 and wrong["usable_pairs"] >= 4      # (1 - 1 / N) of the 0.5 degrees, the rest on the others
    assert all(c["rotation_step_deg"] < 0.15 for c in rep["cameras"] if c is not wrong)
    for p in rep["pairs"]:
        assert p["usable"] and p["inliers"] > 1000 and p["predicted_rms_px"] < 0.05
        assert (p["rms_px"] > 0.5) == (records[WRONG[0]].uid in (p["reference_uid"], p["neighbour_uid"]))
    s = rep["scene"]
    assert s["usable_pairs"] == len(PAIRS) == K * ps.N_CAMS and s["dropped_directions"] == 0 and s["predicted_rms_px"] < 0.02 < 0.5 < s["rms_px"]
    assert "8 cameras corrected from 24 usable pairs" in pose_report.summary_line(rep) and pose_report.warnings(rep) == []
    with pytest.raises(ValueError, match="not a poses.json"):
        pose_report.from_json("[1, 2]")


def test_a_step_above_two_degrees_is_reported_with_one_warning_per_camera():
    records = ps.cameras((5, (0.0, 3.0, 0.0), (0.0, 0.0, 0.0)))
    rows = rig(records)[1]
    rep = pose_report.build_report(rows, records[:ps.N_CAMS], MIN_SAMPLES, CERT, INLIER_PX)
    lines = pose_report.warnings(rep)
    assert len(lines) == 1 and f"uid {records[5].uid}" in lines[0] and "one linear step cannot be trusted" in lines[0]


def test_apply_corrections_and_its_refusals():
    records = ps.cameras(WRONG)[:ps.N_CAMS]
    rep = pose_report.from_json(pose_report.to_json(pose_report.build_report(rig(ps.cameras(WRONG))[1], records, MIN_SAMPLES, CERT, INLIER_PX)))

    class Log:
        lines = []

        def info(self, msg):
            self.lines.append(str(msg))

    out = pose_report.apply_corrections(records, rep, Log())
    assert Log.lines == [] and len(out) == len(records)
    for rec, new, c in zip(records, out, rep["cameras"]):
        assert new.uid == rec.uid and new.image_path == rec.image_path and new.width == rec.width and np.array_equal(new.K, rec.K)
        assert new.R.dtype == np.float32 and new.t.shape == (3, 1) and new.P.shape == (3, 4)
        assert np.abs(new.R - colmap_io._Rotation(c["qvec"]).matrix()).max() < 1e-6 and np.abs(new.t.reshape(3) - np.asarray(c["tvec"])).max() < 1e-6
        assert np.abs(new.C - (-new.R.T @ new.t).reshape(3)).max() < 1e-6
    before = ps.worst_relative_rotation_deg({i: pose_report.pose_of(r) for i, r in enumerate(records)}, PAIRS)
    after = ps.worst_relative_rotation_deg({i: pose_report.pose_of(r) for i, r in enumerate(out)}, PAIRS)
    assert before > 0.49 and after < 0.01
    # the corrected records are not the poses the file was computed for
    with pytest.raises(ValueError, match="computed for other poses"):
        pose_report.apply_corrections(out, rep)
    with pytest.raises(ValueError, match="computed for other poses"):
        pose_report.apply_corrections(ps.cameras()[:ps.N_CAMS], rep)
    moved = [dataclasses.replace(r, t=r.t + np.float32(1e-3)) if i == 4 else r for i, r in enumerate(records)]
    with pytest.raises(ValueError, match=f"uid {records[4].uid}.*computed for other poses"):
        pose_report.apply_corrections(moved, rep)
    # cameras the file does not name stay as they are, and one line counts them
    extra = ps.cameras(WRONG)[ps.N_CAMS:]
    out = pose_report.apply_corrections(records + extra, rep, Log())
    assert out[-1] is extra[-1] and out[-2] is extra[-2] and len(Log.lines) == 1 and "2 of 10 cameras are not named" in Log.lines[0]
