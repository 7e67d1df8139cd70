"""CPU tier of the pose refinement's statistics: the twin (lfd_pose_accumulate_host) against the NumPy reference of
tests/pose_ref.py - every integer of the table - on the analytic rig of tests/pose_scene.py; the Jacobian against central differences of the
residual in all twelve parameters of the two cameras; the order of the slots; the table is added to; a residual exactly at pose_inlier_px; and
what the feature is for: one step from the matches brings a wrong pose back."""
import dataclasses
import types

import numpy as np
import pytest
import torch

import pose_ref
import pose_scene as ps
from lichtfeld_densification_plugin_amd.core import colmap_io
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from lichtfeld_densification_plugin_amd.core import poses as pose_report

CERT, INLIER_PX, MIN_SAMPLES = 0.5, 8.0, 256                           # the knobs' defaults (core/types.py)
MATCH = 64
RECORDS = ps.cameras(ps.TABLE_WRONG)
TABLE_PX = 1.5                                                         # the table tests' pose_inlier_px: inliers and outliers in every pair


@pytest.fixture(scope="module")
def twin():
    d = hb.HostDensifier(2)
    d.upload_cameras(RECORDS)
    yield d
    d.close()


@pytest.mark.parametrize("H,W,k,channels,masks,poisoned", [(16, 16, 3, 2, False, False), (24, 20, 3, 4, True, True), (24, 20, 5, 2, True, True),
                                                           (16, 16, 9, 4, False, True), (24, 20, 9, 2, False, False),
                                                           (16, 16, 5, 4, True, False)])
def test_twin_equals_the_reference_on_every_integer(twin, H, W, k, channels, masks, poisoned):
    cams = RECORDS
    refs = ps.batch_case(H, W, k, channels, masks, poisoned)
    want, per = pose_ref.table(cams, refs, k, MATCH, MATCH, CERT, TABLE_PX)
    table = twin.pose_accumulate(hb.PreparedBatch(refs, MATCH, MATCH, cameras=cams), CERT, TABLE_PX)
    assert table.dtype == torch.int64 and tuple(table.shape) == (3 * k, 32)
    assert np.array_equal(table.numpy(), want)
    assert want[:, 0].sum() > 100 * k and (want[:, 31] == 0).all()
    assert (want[2 * k - 1] == 0).all()                                # the row of the slot the second reference does not have
    assert (want[:, 3] > 0).sum() >= 2 * k and (want[:, 4:10] < 0).any() and (want[:, 4:10] > 0).any() and want[:, 1].sum() > 0
    if poisoned:
        assert want[k - 1, 0] == 0 and want[k - 1, 1] == 0 and want[k - 1, 2] == per[0][k - 1]["conf"].sum() > 50      # coincident centres
        if not masks:
            plain = pose_ref.table(cams, ps.batch_case(H, W, k, channels, masks, False), k, MATCH, MATCH, CERT, TABLE_PX)[1]
            conf0, was0 = per[0][0]["conf"].reshape(H, W), plain[0][0]["conf"].reshape(H, W)
            assert was0[2, 3:9].all() and not conf0[2, 3:9].any()      # NaN certainty
            assert was0[3, 5:11].all() and not conf0[3, 5:11].any()    # NaN observation
            assert was0[5, 2:8].all() and not conf0[5, 2:8].any()      # outside the neighbour
            assert conf0[6, 1:15].all()                                # a certainty exactly at the threshold is confident
            assert not per[0][k - 1]["conf"].reshape(H, W)[4, 7:13].any()      # an infinite observation is not inside the neighbour's grid


def test_the_table_is_added_to_and_nothing_behind_it_is_touched(twin):
    cams = RECORDS
    refs = ps.batch_case(24, 20, 3, 2, True, True)
    want, _per = pose_ref.table(cams, refs, 3, MATCH, MATCH, CERT, TABLE_PX)
    batch = hb.PreparedBatch(refs, MATCH, MATCH, cameras=cams)
    whole = torch.arange(10 * 32, dtype=torch.int64).reshape(10, 32) - 90
    pre = whole.clone()
    twin.pose_accumulate(batch, CERT, TABLE_PX, table=whole[:9])
    assert np.array_equal(whole[:9].numpy(), pre[:9].numpy() + want) and torch.equal(whole[9], pre[9])
    assert torch.equal(whole[:9, 31], pre[:9, 31]) and torch.equal(whole[5], pre[5])      # column 31 and the rows of unused slots
    # two calls of one reference each give the rows of one call of three
    parts = [twin.pose_accumulate(hb.PreparedBatch([r], MATCH, MATCH, cameras=cams), CERT, TABLE_PX).numpy() for r in refs]
    assert parts[1].shape == (2, 32)
    assert np.array_equal(parts[0], want[0:3]) and np.array_equal(parts[1], want[3:5]) and np.array_equal(parts[2], want[6:9])


def test_two_accumulations_in_opposite_slot_order_agree(twin):
    cams = RECORDS
    H, W = 24, 20
    fwd = ps.make(3, [2, 4, 1, 5, 0], H, W, match=MATCH).inputs
    rev = dataclasses.replace(fwd, nbr_cams=fwd.nbr_cams[::-1], cert=fwd.cert[::-1], warp=fwd.warp[::-1])
    a = twin.pose_accumulate(hb.PreparedBatch([fwd], MATCH, MATCH, cameras=cams), CERT, TABLE_PX).numpy()
    b = twin.pose_accumulate(hb.PreparedBatch([rev], MATCH, MATCH, cameras=cams), CERT, TABLE_PX).numpy()
    assert a[:, 0].min() > 100 and np.array_equal(a, b[::-1])


def test_a_residual_exactly_at_pose_inlier_px_is_an_outlier():
    recs, ri, deltas = ps.exact_rig()
    want, per = pose_ref.table(recs, [ri], 1, 65, 65, CERT, ps.EXACT_PX)
    c = per[0][0]
    W = 8
    r = c["r"].reshape(len(deltas), W)
    assert c["conf"].all() and np.array_equal(r, np.tile(np.asarray(deltas)[:, None], (1, W)))      # the rig's arithmetic is exact
    kinds = c["kind"].reshape(len(deltas), W)
    assert [int(k) for k in kinds[:, 0]] == [pose_ref.OUTLIER, pose_ref.OUTLIER, pose_ref.INLIER, pose_ref.INLIER, pose_ref.INLIER,
                                             pose_ref.OUTLIER, pose_ref.INLIER, pose_ref.INLIER]
    assert want[0, :3].tolist() == [5 * W, 3 * W, 0]
    assert want[0, 3] == W * sum(int(round(1024 * d)) ** 2 for d in deltas if abs(d) < ps.EXACT_PX)
    d = hb.HostDensifier(1)
    try:
        d.upload_cameras(recs)
        table = d.pose_accumulate(hb.PreparedBatch([ri], 65, 65, cameras=recs), CERT, ps.EXACT_PX)
    finally:
        d.close()
    assert np.array_equal(table.numpy(), want)


def test_the_jacobian_against_central_differences_through_the_adjoint():
    """r as a function of the two cameras' left twists, T_i -> exp(delta_i) T_i: its derivative is J S [-Ad(R, t) | I] with S the 1 / tn on
    the translation part.  Exact matches (r = 0: the foot point IS the observation), f64 poses, steps of 1e-6: central differences carry a
    relative error of 1e-12 from truncation and 1e-16 |r| / 1e-6 = 1e-8 px per radian or unit from rounding, against entries of 1e2 .. 1e3."""
    A, B = 3, 5
    cams = ps.cameras()
    ri = ps.make(A, [B], 12, 16, match=MATCH).inputs
    base = pose_ref.cells(cams, ri, MATCH, MATCH, CERT, INLIER_PX)[0]
    pick = np.flatnonzero(base["conf"] & (base["kind"] == pose_ref.INLIER))[::7]
    assert len(pick) >= 10
    n = 12 * 16
    warp = ri.warp[0].numpy().reshape(n, 2)
    ax, ay = pose_ref.audit_ref.far_ref.axis(16), pose_ref.audit_ref.far_ref.axis(12)
    yy, xx = np.divmod(np.arange(n), 16)
    sx, sy = pose_ref.support_ref.pixel_scale(ps.WIDTH, MATCH), pose_ref.support_ref.pixel_scale(ps.HEIGHT, MATCH)
    px = lambda v, s: (pose_ref.colour_ref.match_px(v, MATCH - 1) * s)[pick]      # noqa: E731
    ua, va, ub, vb = px(ax[xx], sx), px(ay[yy], sy), px(warp[:, 0], sx), px(warp[:, 1], sy)
    poses = {i: (np.asarray(ps.true_pose(i)[0]), -ps.true_pose(i)[0] @ ps.true_pose(i)[1]) for i in (A, B)}

    def residual(delta_a, delta_b):
        rec = {}
        for i, d in ((A, delta_a), (B, delta_b)):
            E = pose_ref.expm_so3(np.asarray(d[:3]))
            rec[i] = types.SimpleNamespace(K=cams[i].K, R=E @ poses[i][0], t=E @ poses[i][1] + np.asarray(d[3:]))
        return pose_ref.samples(pose_ref.pair_const(rec[A], rec[B], dtype=np.float64), ua, va, ub, vb, INLIER_PX)

    zero = np.zeros(6)
    at = residual(zero, zero)
    assert np.abs(at["r"]).max() < 1e-3                                # exact matches through f32 coordinates
    pc = pose_ref.pair_const(types.SimpleNamespace(K=cams[A].K, R=poses[A][0], t=poses[A][1]),
                             types.SimpleNamespace(K=cams[B].K, R=poses[B][0], t=poses[B][1]), dtype=np.float64)
    Js = at["J"].copy()
    Js[:, 3:] /= pc["tn"]
    want = np.concatenate([-Js @ pose_report.adjoint(pc["R"], pc["t"]), Js], axis=1)      # (n, 12)
    eps = 1e-6
    got = np.zeros_like(want)
    for e in range(12):
        d = np.zeros(12)
        d[e] = eps
        got[:, e] = (residual(d[:6], d[6:])["r"] - residual(-d[:6], -d[6:])["r"]) / (2 * eps)
    # J is taken at the foot point, the differences at the observation |r| < 1e-3 px away: a relative difference of that over the 240 px focal length
    scale = np.abs(want).max()
    assert scale > 100 and np.abs(got - want).max() <= 1e-4 * scale, (np.abs(got - want).max(), scale)


# ---- what the feature is for -----------------------------------------------------------------------------------------------------------------
EH, EW, K = 48, 64, 3
WRONG = (2, (0.5, 0.0, 0.0), (0.0, 0.0, 0.0))


def rig(records, noise_px=0.0):
    """All eight cameras as references with their K nearest neighbours against ``records``: (refs, rows of the twin by (uid, uid))."""
    refs = [ps.make(r, ps.neighbours(r, K), EH, EW, match=MATCH, noise_px=noise_px).inputs for r in range(ps.N_CAMS)]
    d = hb.HostDensifier(2)
    try:
        d.upload_cameras(records)
        table = d.pose_accumulate(hb.PreparedBatch(refs, MATCH, MATCH, cameras=records), CERT, INLIER_PX)
    finally:
        d.close()
    rows = {(records[r].uid, records[n].uid): table[r * K + j].tolist() for r in range(ps.N_CAMS) for j, n in enumerate(ps.neighbours(r, K))}
    return refs, rows


def library_poses(report):
    return {c["uid"] - 1: (colmap_io._Rotation(c["qvec"]).matrix(), np.asarray(c["tvec"])) for c in report["cameras"]}


PAIRS = [(r, n) for r in range(ps.N_CAMS) for n in ps.neighbours(r, K)]


def test_the_scene_fixes_the_poses_and_one_step_of_the_reference_brings_a_wrong_pose_back():
    """The two conditions the scene has to satisfy (asserted here, on the CPU): the reduced normal matrix's smallest eigenvalue is at least
    1e-6 of its largest, and the reference's own single step cuts the worst pair's median distance at least tenfold for a 0.5 degree
    rotation of one camera."""
    records = ps.cameras(WRONG)
    refs, _rows = rig(records)
    gn = pose_ref.gn_step(records, refs, MATCH, MATCH, CERT, INLIER_PX, MIN_SAMPLES)
    assert gn["eig_min_rel"] >= 1e-6
    from lichtfeld_densification_plugin_amd.core.types import CameraRecord
    moved = [CameraRecord.from_krt(c.uid, c.K, gn["poses"][i][0], gn["poses"][i][1], c.width, c.height) for i, c in enumerate(records[:ps.N_CAMS])]
    again = pose_ref.gn_step(moved + records[ps.N_CAMS:], refs, MATCH, MATCH, CERT, INLIER_PX, MIN_SAMPLES)
    before, after = max(gn["median"].values()), max(again["median"].values())
    print("worst pair's median distance:", before, "->", after)
    assert before > 1.5 and after <= before / 10.0


@pytest.mark.parametrize("noise_px", [0.0, 0.5])
def test_effect(noise_px):
    """Eight references of 48 x 64 cells with three neighbours each, every knob at its default, the record of camera 2 rotated by 0.5 degrees
    about its x axis.  The library's step (integer tables, core/poses.py) against the reference's un-quantised step from the same matches:
    the worst relative rotation of a matched pair drops from 0.5 degrees to within the reference's own result plus the quantisation
    allowance QUANT_DEG; from the TRUE records no camera moves by more than the reference's own step does, plus the allowance.  The
    allowance: the largest difference between the two figures measured on this scene was 8.7e-4 degrees (0.5 px of noise,
    true records; 3.8e-4 with the wrong record, 7e-6 and 2e-6 without noise), and the allowance is twice that."""
    QUANT_DEG = 1.8e-3
    records = ps.cameras(WRONG)
    refs, rows = rig(records, noise_px)
    assert np.array_equal(np.asarray([rows[(records[r].uid, records[n].uid)] for r, n in PAIRS]),
                          pose_ref.table(records, refs, K, MATCH, MATCH, CERT, INLIER_PX)[0])
    rep = pose_report.build_report(rows, records[:ps.N_CAMS], MIN_SAMPLES, CERT, INLIER_PX)
    gn = pose_ref.gn_step(records, refs, MATCH, MATCH, CERT, INLIER_PX, MIN_SAMPLES)
    start = ps.worst_relative_rotation_deg({i: pose_ref.pose64(records[i]) for i in range(ps.N_CAMS)}, PAIRS)
    ref_after = ps.worst_relative_rotation_deg(gn["poses"], PAIRS)
    lib_after = ps.worst_relative_rotation_deg(library_poses(rep), PAIRS)
    print("noise", noise_px, "worst relative rotation:", start, "-> reference", ref_after, "library", lib_after)
    lib = library_poses(rep)
    print("largest angle between the library's and the reference's corrected rotation:",
          max(ps.rotation_angle_deg(lib[i][0] @ gn["poses"][i][0].T) for i in range(ps.N_CAMS)))
    assert 0.49 < start < 0.51 and ref_after < 0.05
    assert lib_after <= ref_after + QUANT_DEG
    assert rep["scene"]["dropped_directions"] == 0 and rep["scene"]["cameras_left_out"] == [] and rep["scene"]["usable_pairs"] == len(PAIRS)
    assert rep["scene"]["predicted_rms_px"] < rep["scene"]["rms_px"]
    # from the true records
    true = ps.cameras()
    refs, rows = rig(true, noise_px)
    rep = pose_report.build_report(rows, true[:ps.N_CAMS], MIN_SAMPLES, CERT, INLIER_PX)
    gn = pose_ref.gn_step(true, refs, MATCH, MATCH, CERT, INLIER_PX, MIN_SAMPLES)
    lib_step, ref_step = max(c["rotation_step_deg"] for c in rep["cameras"]), max(gn["step_deg"].values())
    print("noise", noise_px, "largest step from the true records: reference", ref_step, "library", lib_step)
    assert lib_step <= ref_step + QUANT_DEG
