"""CPU tier of the epipolar audit: the twin (lfd_epipolar_audit_host) against the NumPy reference of tests/audit_ref.py -
every element of the table and of the cell map - on the analytic rig of tests/audit_scene.py, and what the feature is for: one wrong pose
among six is named, a region that moved shows in the maps."""
import dataclasses
import math

import numpy as np
import pytest
import torch

import audit_ref
import audit_scene as asc
from lichtfeld_densification_plugin_amd.core import audit as audit_report
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

CERT, MIN_SAMPLES, WARN_PX = 0.5, 256, 0.8                            # the knobs' defaults (core/types.py; audit_warn_px 0 = reproj_thresh = 0.8)
MATCH = 64
H, W = 24, 20                                                          # 480 cells: no multiple of 64 or 256


@pytest.fixture(scope="module")
def twin():
    d = hb.HostDensifier(2)
    d.upload_cameras(asc.cameras())
    yield d
    d.close()


def u64(t):
    return t.cpu().numpy().view(np.uint64)


_made = {}


def case(channels, masks):
    """Two references with 3 and 1 neighbours (k = 3)."""
    key = (channels, masks)
    if key not in _made:
        _made[key] = [asc.make(r, asc.neighbours(r, n), H, W, match=MATCH, channels=channels, masks=masks) for r, n in ((1, 3), (4, 1))]
    return _made[key]


def poisoned(scenes):
    """The references of ``scenes`` with every kind of entry the rule singles out."""
    cams = asc.cameras()
    refs = []
    for s in scenes:
        ri = s.inputs
        cert, warp = [c.clone() for c in ri.cert], [w.clone() for w in ri.warp]
        cert[0][2, 3:9] = float("nan")
        cert[0][6, 1:15] = CERT                                        # exactly the threshold: counts
        warp[0][3, 5:11, -2] = float("nan")
        warp[-1][4, 7:13, -1] = float("inf")
        warp[0][5, 2:8, -2] = 1.5                                      # outside the neighbour's grid
        fund = [np.asarray(hb.fundamental_from_world2cam(cams[ri.ref_cam].K, cams[ri.ref_cam].R, cams[ri.ref_cam].t, cams[n].K, cams[n].R,
                                                         cams[n].t), np.float32) for n in ri.nbr_cams]
        fund[-1] = fund[-1].copy()
        fund[-1][:2, :] = 0.0                                          # rows 0 and 1 zero: every sample of the pair is degenerate
        refs.append(dataclasses.replace(ri, cert=cert, warp=warp, fundamental=fund))
    return refs


@pytest.mark.parametrize("channels,masks", [(2, False), (4, True), (2, True), (4, False)])
def test_twin_equals_the_reference_element_for_element(twin, channels, masks):
    cams = asc.cameras()
    refs = [s.inputs for s in case(channels, masks)]
    batch = hb.PreparedBatch(refs, MATCH, MATCH, cameras=cams)
    best = torch.full((2, H * W), 7, dtype=torch.uint8)
    table = twin.epipolar_audit(batch, CERT, best=best)
    want, want_best, per = audit_ref.audit(cams, refs, 3, MATCH, MATCH, CERT)
    assert table.dtype == torch.int64 and tuple(table.shape) == (6, 66)
    assert np.array_equal(u64(table), want) and np.array_equal(best.numpy(), want_best)
    assert want[:4, 0].min() > 100 and (want[4:, :] == 0).all()        # rows of slots >= n_slots stay zero
    assert (want_best == 255).sum() > 0 and (want_best == 0).sum() > 100
    # a table that holds something is added to; rows of unused slots are untouched; best = None gives the same table
    pre = torch.arange(6 * 66, dtype=torch.int64).reshape(6, 66) + 5
    again = twin.epipolar_audit(batch, CERT, table=pre.clone())
    assert np.array_equal(again.numpy(), pre.numpy() + want.view(np.int64))
    assert np.array_equal(again.numpy()[4:], pre.numpy()[4:])
    # two calls of one reference each give the rows of one call of two
    t0 = twin.epipolar_audit(hb.PreparedBatch(refs[:1], MATCH, MATCH, cameras=cams), CERT)
    t1 = twin.epipolar_audit(hb.PreparedBatch(refs[1:], MATCH, MATCH, cameras=cams), CERT)
    assert tuple(t0.shape) == (3, 66) and tuple(t1.shape) == (1, 66)
    assert np.array_equal(u64(t0), want[:3]) and np.array_equal(u64(t1)[0], want[3])


@pytest.mark.parametrize("channels,masks", [(2, False), (4, True)])
def test_poisoned_entries(twin, channels, masks):
    cams = asc.cameras()
    scenes = case(channels, masks)
    refs = poisoned(scenes)
    batch = hb.PreparedBatch(refs, MATCH, MATCH)
    best = torch.zeros((2, H * W), dtype=torch.uint8)
    table = twin.epipolar_audit(batch, CERT, best=best)
    want, want_best, per = audit_ref.audit(cams, refs, 3, MATCH, MATCH, CERT)
    assert np.array_equal(u64(table), want) and np.array_equal(best.numpy(), want_best)
    plain = audit_ref.audit(cams, [s.inputs for s in scenes], 3, MATCH, MATCH, CERT)[2]
    conf0, was0 = per[0]["conf"][:, 0].reshape(H, W), plain[0]["conf"][:, 0].reshape(H, W)
    if not masks:
        assert was0[2, 3:9].all() and not conf0[2, 3:9].any()          # NaN certainty
        assert was0[3, 5:11].all() and not conf0[3, 5:11].any()        # NaN observation
        assert was0[5, 2:8].all() and not conf0[5, 2:8].any()          # outside the neighbour
        assert conf0[6, 1:15].all()                                    # a certainty exactly at the threshold is confident
    # the pair with the zeroed F rows: every confident sample is degenerate and none is usable
    assert want[2, 0] == 0 and want[2, 1] == per[0]["conf"][:, 2].sum() > 100
    assert want[3, 0] == 0 and want[3, 1] > 100 and (want_best[1] == 255).all()
    # an infinite observation is not inside the neighbour's grid
    assert not per[0]["conf"][:, 2].reshape(H, W)[4, 7:13].any()


# ---- what the feature is for -----------------------------------------------------------------------------------------------------------------
EH, EW, K = 48, 64, 3
PITCHED, THETA = 2, 0.5


def run_rig(records, displaced=None):
    """All six cameras as references with their K nearest neighbours, audited against ``records``.  Returns (rows by (ref, nbr), best, per)."""
    d = hb.HostDensifier(2)
    try:
        d.upload_cameras(records)
        refs = [asc.make(r, asc.neighbours(r, K), EH, EW, match=MATCH, displaced=displaced).inputs for r in range(asc.N_CAMS)]
        best = torch.zeros((asc.N_CAMS, EH * EW), dtype=torch.uint8)
        table = d.epipolar_audit(hb.PreparedBatch(refs, MATCH, MATCH, cameras=records), CERT, best=best)
    finally:
        d.close()
    want, want_best, per = audit_ref.audit(records, refs, K, MATCH, MATCH, CERT)
    assert np.array_equal(u64(table), want) and np.array_equal(best.numpy(), want_best)
    rows = {(r, n): table[r * K + j].tolist() for r in range(asc.N_CAMS) for j, n in enumerate(asc.neighbours(r, K))}
    return rows, best.numpy(), per


def test_effect():
    """Six references of 48 x 64 cells with three neighbours each, every knob at its default.

    Exact records: no camera is suspect and every usable pair's median is the first bin's edge.  The record of camera 2 pitched by 0.5 degrees
    (f tan(theta) = 2.09 px >= 2.5 x audit_warn_px): exactly that camera is suspect, its score lies within 25 % of f tan(theta) - a pitch moves
    every observation of a horizontal rig by f tan(theta) (1 + (v / f)^2) across the rows, 1 .. 1.25 x over this image's half height of f / 2,
    and the bin's upper edge adds at most 0.125 px - and every pair without it stays in the first bin."""
    rows, _best, _per = run_rig(asc.cameras())
    rep = audit_report.build_report(rows, None, MIN_SAMPLES, WARN_PX, CERT)
    assert rep["scene"]["suspects"] == [] and rep["scene"]["usable_pairs"] >= 16
    assert all(p["median_px"] == 0.125 for p in rep["pairs"] if p["usable"])
    shift = asc.FOCAL * math.tan(math.radians(THETA))
    assert shift >= 2.5 * WARN_PX
    rows, _best, _per = run_rig(asc.cameras((PITCHED, THETA)))
    rep = audit_report.build_report(rows, None, MIN_SAMPLES, WARN_PX, CERT)
    usable = [p for p in rep["pairs"] if p["usable"]]
    for cam in range(asc.N_CAMS):                                      # the premise of the per-camera rule on this rig
        if cam != PITCHED:
            mine = [p for p in usable if cam in (p["reference_uid"], p["neighbour_uid"])]
            assert 2 * sum(PITCHED in (p["reference_uid"], p["neighbour_uid"]) for p in mine) < len(mine)
    assert rep["scene"]["suspects"] == [PITCHED]
    score = [c for c in rep["cameras"] if c["uid"] == PITCHED][0]["score_px"]
    print("f tan(theta) =", shift, "score =", score)
    assert abs(score - shift) <= 0.25 * shift
    with_it = [p for p in usable if PITCHED in (p["reference_uid"], p["neighbour_uid"])]
    assert len(with_it) == 8 and all(abs(p["median_px"] - shift) <= 0.25 * shift for p in with_it)
    assert all(p["median_px"] == 0.125 for p in usable if PITCHED not in (p["reference_uid"], p["neighbour_uid"]))
    assert len(audit_report.warnings(rep)) == 1 and "uid 2" in audit_report.warnings(rep)[0]


def test_effect_maps():
    """A rectangle of cells displaced by 3 px across the epipolar line in every slot: every displaced cell with a confident slot reads >= 2.5
    px, every other cell with data reads 0 (bin 0), cells without a confident slot read NaN."""
    box = (10, 30, 20, 44)
    _rows, best, per = run_rig(asc.cameras(), displaced=box)
    inside = np.zeros((EH, EW), bool)
    inside[box[0]:box[1], box[2]:box[3]] = True
    inside = inside.reshape(-1)
    for r in range(asc.N_CAMS):
        px = np.where(best[r] == 255, np.nan, best[r].astype(np.float32) / 8.0)
        has = per[r]["conf"].any(axis=1)
        assert (inside & has).sum() > 200 and (~inside & has).sum() > 1000
        assert (px[inside & has] >= 2.5).all()
        assert (px[~inside & has] == 0).all()
        assert np.isnan(px[~has]).all()
