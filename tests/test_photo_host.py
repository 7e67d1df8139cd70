"""CPU tier of the photo-consistency gate (lfd_photo_gate_host): the twin against the brute-force reference of
tests/photo_ref.py - EXACTLY on status, kept points, offsets, per-slot counts and every copied array, within one f32 ulp on ncc - on the
rendered plane of tests/photo_scene.py: a 6 x 8 grid (at R = 3 the window crosses every border at once) and 20 x 24, k in {1, 3, 16}, 2- and
4-channel warps, masks on and off, R in {1, 2, 3}, an empty reference, the guards, a NaN observation and a certainty of exactly 0 inside a
window, the participation threshold from both sides, constant patches - and what the stage is for (test_effect)."""
import dataclasses

import numpy as np
import pytest
import torch

import colour_scene as cs
import photo_ref
import photo_scene as ps
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

MATCH = ps.MATCH


@pytest.fixture(scope="module")
def twin():
    d = hb.HostDensifier(2)
    d.upload_cameras(cs.cameras())
    yield d
    d.close()


def gate_and_compare(twin, inputs, res, R, min_ncc=0.8, min_texture=2.0, match=MATCH):
    """The twin over ``res`` against the reference, everything the call returns; (status, ncc, kept mask)."""
    batch = hb.PreparedBatch(inputs, match, match)
    counters = torch.tensor([1, 10, 100, 1000, 10000], dtype=torch.int64)
    out, status, ncc = twin.photo_gate(batch, res, R, min_ncc, min_texture, with_status=True, with_ncc=True, counters=counters)
    want_status, kept, want_ncc = photo_ref.batch_reference(inputs, match, match, res, R, min_ncc, min_texture)
    st = status.numpy()
    assert np.array_equal(st, want_status)
    assert ps.ulp_apart(ncc.numpy(), want_ncc) <= 1
    assert np.array_equal(np.isnan(want_ncc), (want_status < 3) | ((want_status == 4) & np.isnan(want_ncc)))
    cols, offs, seg = photo_ref.filtered(res, kept)
    assert out.count == int(kept.sum()) and np.array_equal(out.ref_offsets, offs) and np.array_equal(out.seg_counts, seg)
    for name, want in zip(("xyz", "rgb", "err", "cell", "slot"), cols):
        assert np.array_equal(ps.bits(getattr(out, name)), ps.bits(want)), name
    assert (counters - torch.tensor([1, 10, 100, 1000, 10000])).tolist() == np.bincount(st, minlength=5).tolist()      # added to
    plain = twin.photo_gate(batch, res, R, min_ncc, min_texture)                       # no optional output: the same points
    assert plain.count == out.count and np.array_equal(ps.bits(plain.xyz), ps.bits(out.xyz))
    return st, ncc.numpy(), kept


def dense_points(twin, scenes):
    return twin.triangulate_dense(hb.PreparedBatch([s.inputs for s in scenes], MATCH, MATCH), ps.params())


@pytest.mark.parametrize("H,W,k,channels,masks,R", ps.SHAPES)
def test_twin_equals_the_reference(twin, H, W, k, channels, masks, R):
    scenes = ps.case(H, W, k, channels, masks)
    res = dense_points(twin, scenes)
    assert res.count > 0.8 * 2 * H * W and (np.diff(res.ref_offsets) > 0).all()
    st, _ncc, _kept = gate_and_compare(twin, [s.inputs for s in scenes], res, R)
    seen = set(st.tolist())
    if (H, W) == (20, 24) and not masks:
        assert {2, 3, 4} <= seen, seen                                        # untextured, consistent and refuted points all occur
    if (H, W, R) == (6, 8, 3):
        assert 1 in seen                                                       # a corner's window holds 16 of 49 cells


@pytest.mark.parametrize("which", [0, 1])
def test_one_reference_empty(twin, which):
    scenes = ps.case(20, 24, 3, 2, False)
    res = ps.one_reference_empty(dense_points(twin, scenes), which)
    assert res.ref_offsets[which + 1] == res.ref_offsets[which] and res.count > 300
    gate_and_compare(twin, [s.inputs for s in scenes], res, 2)


def test_guarded_points_are_kept_untouched(twin):
    scenes = ps.case(20, 24, 3, 2, False)
    res = dense_points(twin, scenes)
    n0, HW = int(res.ref_offsets[1]), 20 * 24
    cell, slot = res.cell.clone(), res.slot.clone()
    cell[7] = -1
    cell[8] = HW
    cell[n0 + 1] = 2 ** 31 - 1
    cell[n0 + 3] = -2 ** 31
    slot[9] = 3                                                                # n_slots of every reference is 3
    slot[n0 + 2] = 255
    bad = [7, 8, 9, n0 + 1, n0 + 2, n0 + 3]
    hurt = dataclasses.replace(res, cell=cell, slot=slot, _packed=None)
    st, ncc, kept = gate_and_compare(twin, [s.inputs for s in scenes], hurt, 3)
    assert (st[bad] == 0).all() and kept[bad].all() and np.isnan(ncc[bad]).all()


def centre_point(res, H, W, y, x):
    hit = np.nonzero(res.cell.numpy() == y * W + x)[0]
    assert hit.size == 1
    return int(hit[0])


def test_nan_observation_and_zero_certainty_inside_a_window(twin):
    """A window cell with a NaN observation, one with an infinite one, one just outside [-1, 1] and one whose certainty is exactly 0 take no
    part: the point's sums are those of the others."""
    H, W = 20, 24
    sc = ps.make(5, 1, H, W, match=MATCH)
    hurt = ps.to_device(sc.inputs, "cpu")
    hurt.warp[0], hurt.cert[0] = sc.inputs.warp[0].clone(), sc.inputs.cert[0].clone()
    hurt.warp[0][9, 10, 0] = float("nan")
    hurt.warp[0][9, 11, 1] = float("inf")
    hurt.warp[0][10, 11, 0] = float(np.nextafter(np.float32(1.0), np.float32(2.0)))
    hurt.warp[0][11, 11, 1] = -1.0                                             # exactly on the border: takes part
    hurt.cert[0][11, 10] = 0.0
    hurt.cert[0][11, 12] = float("nan")
    res = twin.triangulate_dense(hb.PreparedBatch([sc.inputs], MATCH, MATCH), ps.params())
    gate_and_compare(twin, [hurt], res, 1)
    sums = []
    photo_ref.batch_reference([hurt], MATCH, MATCH, res, 1, 0.8, 2.0, sums)
    assert int(sums[0][centre_point(res, H, W, 10, 11), 0]) == 9 - 5


@pytest.mark.parametrize("R", [1, 3])
def test_exactly_half_the_window_and_one_fewer(twin, R):
    """2 n >= (2R + 1)^2 + 1 decides: with n = ((2R + 1)^2 + 1) / 2 cells the point is judged, with one fewer it is kept with status 1."""
    H, W = 20, 24
    sc = ps.make(5, 1, H, W, match=MATCH)
    res = twin.triangulate_dense(hb.PreparedBatch([sc.inputs], MATCH, MATCH), ps.params())
    side = 2 * R + 1
    need = (side * side + 1) // 2
    i = centre_point(res, H, W, 10, 11)
    for n, judged in ((need, True), (need - 1, False)):
        hurt = ps.to_device(sc.inputs, "cpu")
        hurt.cert[0] = sc.inputs.cert[0].clone()
        window = [(10 + dy, 11 + dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1)]
        for (y, x) in window[:side * side - n]:
            hurt.cert[0][y, x] = 0.0
        st, _ncc, _kept = gate_and_compare(twin, [hurt], res, R)
        sums = []
        photo_ref.batch_reference([hurt], MATCH, MATCH, res, R, 0.8, 2.0, sums)
        assert int(sums[0][i, 0]) == n and (st[i] != 1) == judged


@pytest.mark.parametrize("min_texture,status", [(2.0, 2), (0.0, 4)])
def test_constant_patches(twin, min_texture, status):
    """Constant images: va = vb = cov = 0.  With a texture floor the points are untextured (kept); with min_texture = 0 nothing is below the
    floor, cov > 0 fails and they are refuted - the rule as written - with ncc = 0 / 0 = NaN."""
    H, W = 6, 8
    sc = ps.make(5, 3, H, W, match=MATCH)
    flat = ps.to_device(sc.inputs, "cpu")
    flat.image = torch.full_like(sc.inputs.image, 131)
    flat.nbr_images = [torch.full_like(t, 90 + 7 * j) for j, t in enumerate(sc.inputs.nbr_images)]
    res = twin.triangulate_dense(hb.PreparedBatch([flat], MATCH, MATCH), ps.params())
    st, ncc, _kept = gate_and_compare(twin, [flat], res, 1, min_texture=min_texture)
    sums = []
    photo_ref.batch_reference([flat], MATCH, MATCH, res, 1, 0.8, min_texture, sums)
    n, Sa, Sb, Saa, Sbb, Sab = (sums[0][:, e] for e in range(6))
    judged = st != 1
    assert judged.sum() > 20
    assert (n * Saa == Sa * Sa)[judged].all() and (n * Sbb == Sb * Sb)[judged].all() and (n * Sab == Sa * Sb)[judged].all()
    assert (st[judged] == status).all() and np.isnan(ncc).all()


def whole_window(mask, cell, H, W, R):
    """Points whose whole window (clamped to the grid) lies inside ``mask``."""
    y, x = cell // W, cell % W
    ok = np.ones(cell.shape, bool)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            ok &= mask[np.clip(y + dy, 0, H - 1), np.clip(x + dx, 0, W - 1)]
    return ok


def test_effect():
    """What the stage buys: k = 1, so no third view exists and no support filter is possible.  A 256^2 rendering of the plane, 40 x 48 cells;
    rows 4 .. 15 have their observations slid by 3 match pixels along their epipolar lines; cells (24 .. 36, 6 .. 22) look at constant albedo.
    R = 3, min_photo_ncc = 0.8, photo_min_texture = 2.  The conditions are on the REFERENCE's verdicts, over the points whose whole window
    lies in the slid band, in the untextured rectangle, in neither:

        at least 0.90 of the slid points are dropped; at most 0.01 of the clean textured points are; every untextured point is kept, status 2

    and the same scene through every geometric gate the twin has (Sampson, reprojection, parallax at their defaults) keeps EVERY slid point.

    Measured: 288 slid points, 0.958 dropped (the others have under half a window inside the neighbour's image: status 1), the 95th
    percentile of their ZNCC 0.27; 619 clean points, none dropped, the 5th percentile of their ZNCC 0.991; 77 untextured points, all status 2."""
    match, H, W, R = 256, 40, 48, 3
    sc = ps.make(12, 1, H, W, match=match, slide_rows=(4, 15), slide_px=3.0, flat_cells=(24, 36, 6, 22))
    twin = hb.HostDensifier(2)
    twin.upload_cameras(cs.cameras())
    try:
        res = twin.triangulate_dense(hb.PreparedBatch([sc.inputs], match, match), ps.params())
    finally:
        twin.close()
    cell = res.cell.numpy().astype(np.int64)
    assert sc.slid.sum() == 12 * W and np.isin(np.nonzero(sc.slid.reshape(-1))[0], cell).all()      # the geometric gates keep every slid cell
    status, kept, ncc = photo_ref.batch_reference([sc.inputs], match, match, res, R, 0.8, 2.0)
    slid, flat = whole_window(sc.slid, cell, H, W, R), whole_window(sc.flat, cell, H, W, R)
    clean = whole_window(~sc.slid & ~sc.flat, cell, H, W, R)
    assert slid.sum() >= 200 and clean.sum() >= 400 and flat.sum() >= 50
    print(f"slid: {slid.sum()} points, {(~kept[slid]).mean():.3f} dropped, ZNCC p95 {np.nanpercentile(ncc[slid], 95):.3f}; "
          f"clean: {clean.sum()} points, {(~kept[clean]).mean():.3f} dropped, ZNCC p5 {np.nanpercentile(ncc[clean], 5):.3f}; "
          f"untextured: {flat.sum()} points, statuses {np.bincount(status[flat]).tolist()}")
    assert (~kept[slid]).mean() >= 0.90
    assert (~kept[clean]).mean() <= 0.01
    assert (status[flat] == 2).all() and kept[flat].all()
