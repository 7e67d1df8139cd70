"""CPU tier of the multi-view re-triangulation: the twin (lfd_refine_multiview_host) against the f64 reference of tests/refine_ref.py, the gain in
accuracy against the noise-free truth, the exact properties of the contract and its edge cases.

Measured on the probe scenes (ring of 40 cameras, reference 10, 512^2 match size, tie-free certainty, 0.5 px noise, 5 % outliers, two-view points from
the twin's dense call at reproj_thresh 0.8), for the twin: points with a candidate / refined / fallen back / in band, and the ratio of the median
distance to the truth after and before (the f64 reference gives the same ratios to four digits):
    64x48 k=3  tau 1.6   2816 / 2660 / 156 / 2 (0.07 %)   0.662        tau 3.0   2888 / 2601 / 287 / 3 (0.10 %)   0.634
    37x29 k=8  tau 1.6   1000 /  876 / 124 / 4 (0.40 %)   0.527 (two and four channels)
    96x96 k=3  tau 1.6   8522 / 8063 / 459 / 11 (0.13 %)  0.666
No status outside the band differs from the reference's; refined coordinates differ from the reference's by at most 1e-9.  The cap is 0.5 %."""
import dataclasses

import numpy as np
import pytest
import torch

import refine_ref as rr
import support_scene as sc
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from test_support_filter_host import _epipolar_shift

THR = 0.8            # reproj_thresh of the two-view filter and of the acceptance test
_cache = {}


@pytest.fixture(scope="module")
def twin():
    d = hb.HostDensifier(4)
    d.upload_cameras(sc.cameras())
    yield d
    d.close()


def probe(twin, k, H, W, channels=2, masks=False):
    """One reference of the probe scene triangulated by the twin's dense call, the noise-free truth of its points: computed once per module."""
    key = (k, H, W, channels, masks)
    if key not in _cache:
        _s, ri = sc.reference_inputs(10, k, H, W, channels=channels, masks=masks)
        batch = hb.PreparedBatch([ri], sc.MATCH, sc.MATCH)
        src = twin.triangulate_dense(batch, sc.params(reproj_thresh=THR))
        _s0, clean = sc.reference_inputs(10, k, H, W, channels=channels, noise_px=0.0, outlier_frac=0.0)
        truth = rr.two_view_f64(sc.cameras(), 10, ri.nbr_cams, [w.numpy() for w in clean.warp], sc.MATCH, sc.MATCH, src.cell.numpy(), src.slot.numpy())
        _cache[key] = (ri, batch, src, truth)
    return _cache[key]


def reference_of(ri, src, tau):
    return rr.over_references(sc.cameras(), [ri], src, tau, THR, sc.MATCH, sc.MATCH)


CASES = [(3, 48, 64, 2, False, 1.6), (3, 48, 64, 2, False, 3.0), (8, 29, 37, 4, False, 1.6), (8, 29, 37, 2, False, 1.6), (3, 48, 64, 2, True, 1.6)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"k{c[0]}_{c[2]}x{c[1]}_c{c[3]}{'_masks' if c[4] else ''}_tau{c[5]}")
def test_twin_takes_the_reference_decision_outside_the_band(twin, case):
    k, H, W, channels, masks, tau = case
    ri, batch, src, _truth = probe(twin, k, H, W, channels, masks)
    counters = torch.zeros(2, dtype=torch.int64)
    res, status = twin.refine_multiview(batch, src, tau, THR, with_status=True, counters=counters)
    ref = reference_of(ri, src, tau)
    n_has, n_band, n_acc, n_fall = rr.check_against_reference(ref, src, res.xyz, res.err, status, THR, sc.BAND_CAP)
    print(f"{case}: {src.count} points, {n_has} with a candidate, {n_acc} refined, {n_fall} fallen back, {n_band} in band "
          f"({100.0 * n_band / max(n_has, 1):.3f} %)")
    assert src.count > 900 and n_has > (0.6 if masks else 0.9) * src.count and n_acc > 0.8 * n_has and n_fall > 20
    assert counters.tolist() == [n_acc, n_fall]
    # what never changes: the other arrays, the offsets, the order
    for name in ("rgb", "cell", "slot"):
        assert np.array_equal(rr.bits(getattr(res, name)), rr.bits(getattr(src, name)))
    assert np.array_equal(res.ref_offsets, src.ref_offsets) and np.array_equal(res.seg_counts, src.seg_counts)
    # the candidates are the support filter's own count, bit for bit
    _f, sup = twin.support_filter(batch, src, 1, tau, with_support=True)
    assert np.array_equal(status.numpy() & 0x7f, sup.numpy())
    # a second call adds to the counters and gives the same bits
    again, status2 = twin.refine_multiview(batch, src, tau, THR, with_status=True, counters=counters)
    assert counters.tolist() == [2 * n_acc, 2 * n_fall] and torch.equal(status, status2)
    assert np.array_equal(rr.bits(again.xyz), rr.bits(res.xyz)) and np.array_equal(rr.bits(again.err), rr.bits(res.err))


@pytest.mark.parametrize("k,H,W,bound", [(3, 48, 64, 0.8), (8, 29, 37, 0.7)])
def test_refined_points_are_closer_to_the_truth(twin, k, H, W, bound):
    """Median distance to the noise-free truth over the points with a candidate: the f64 study gives 0.66 x the two-view median at k = 3 and
    0.52 x at k = 8.  First the reference's own output, then the twin's."""
    ri, batch, src, truth = probe(twin, k, H, W)
    ref = reference_of(ri, src, 1.6)
    res, status = twin.refine_multiview(batch, src, 1.6, THR, with_status=True)
    has = ref["n_extra"] > 0
    assert np.array_equal(has, (status.numpy() & 0x7f) > 0)
    dist = lambda xyz: np.linalg.norm(np.asarray(xyz, np.float64) - truth, axis=1)[has]
    before, by_ref, by_twin = np.median(dist(src.xyz.numpy())), np.median(dist(ref["xyz"])), np.median(dist(res.xyz.numpy()))
    print(f"k={k} {W}x{H}: median distance to the truth {before:.5f} -> reference {by_ref:.5f} ({by_ref / before:.3f}), twin {by_twin:.5f} "
          f"({by_twin / before:.3f})")
    assert by_ref <= bound * before
    assert by_twin <= bound * before


def test_in_place_and_out_of_place_give_the_same_bits(twin):
    """OutputBuffers are refined in place (the asynchronous form the hot path uses), a collected result is copied."""
    refs = [sc.reference_inputs(ref, k, 24, 32)[1] for ref, k in ((10, 3), (20, 2))]
    batch = hb.PreparedBatch(refs, sc.MATCH, sc.MATCH)
    buf = hb.OutputBuffers(2 * 24 * 32, 2, 3, torch.device("cpu"))
    import ctypes as C
    assert twin._lib.lfd_triangulate_dense_host(twin._ctx, C.byref(batch.c), C.byref(sc.params(reproj_thresh=THR)), C.byref(buf.c),
                                                buf.ref_offsets.data_ptr(), buf.seg_counts.data_ptr()) == 0
    src = buf.collect()
    src = dataclasses.replace(src, xyz=src.xyz.clone(), err=src.err.clone(), rgb=src.rgb.clone(), _packed=None)
    copy, st_copy = twin.refine_multiview(batch, src, 1.6, THR, with_status=True)
    assert copy.xyz.data_ptr() != src.xyz.data_ptr()
    same, st_same = twin.refine_multiview(batch, buf, 1.6, THR, with_status=True)
    assert same is buf and st_same.numel() == buf.capacity
    got = buf.collect()
    assert np.array_equal(rr.bits(got.xyz), rr.bits(copy.xyz)) and np.array_equal(rr.bits(got.err), rr.bits(copy.err))
    assert np.array_equal(rr.bits(got.rgb), rr.bits(src.rgb)) and torch.equal(got.cell, src.cell) and torch.equal(got.slot, src.slot)
    assert torch.equal(st_same[:src.count], st_copy) and int((st_copy & 0x80 != 0).sum()) > 100
    moved = (rr.bits(copy.xyz) != rr.bits(src.xyz)).any(axis=1)
    assert np.array_equal(moved, (st_copy.numpy() & 0x80) != 0)
    with pytest.raises(ValueError, match="with_cell"):
        twin.refine_multiview(batch, hb.OutputBuffers(16, 2, 3, torch.device("cpu"), with_cell=False), 1.6, THR)
    with pytest.raises(ValueError, match="references"):
        twin.refine_multiview(hb.PreparedBatch(refs[:1], sc.MATCH, sc.MATCH), buf, 1.6, THR)
    with pytest.raises(ValueError, match="counters"):
        twin.refine_multiview(batch, buf, 1.6, THR, counters=torch.zeros(2, dtype=torch.int32))


# ---- edge cases ---------------------------------------------------------------------------------------------------------------------------------
def small(twin, spec, H=24, W=32, **kw):
    refs = [sc.reference_inputs(ref, k, H, W, **kw)[1] for ref, k in spec]
    batch = hb.PreparedBatch(refs, sc.MATCH, sc.MATCH)
    return refs, batch, twin.triangulate_dense(batch, sc.params(reproj_thresh=THR))


def unchanged(res, src, rows=slice(None)):
    return np.array_equal(rr.bits(res.xyz)[rows], rr.bits(src.xyz)[rows]) and np.array_equal(rr.bits(res.err)[rows], rr.bits(src.err)[rows])


def test_one_neighbour_has_nobody_to_ask(twin):
    refs, batch, src = small(twin, [(10, 1)])
    counters = torch.zeros(2, dtype=torch.int64)
    res, status = twin.refine_multiview(batch, src, 1e9, THR, with_status=True, counters=counters)
    assert src.count > 300 and int(status.max()) == 0 and unchanged(res, src) and counters.tolist() == [0, 0]


def test_ragged_slots_an_empty_reference_and_an_empty_cloud(twin):
    refs = [sc.reference_inputs(ref, k, 24, 32)[1] for ref, k in ((10, 3), (20, 1), (30, 3), (35, 2))]
    refs[2].mask_a = torch.zeros((sc.MATCH, sc.MATCH), dtype=torch.uint8)         # masked out: a reference with 0 points
    batch = hb.PreparedBatch(refs, sc.MATCH, sc.MATCH)
    src = twin.triangulate_dense(batch, sc.params(reproj_thresh=THR))
    off = src.ref_offsets
    assert off[1] > 0 and off[2] > off[1] and off[3] == off[2] and off[4] > off[3]
    res, status = twin.refine_multiview(batch, src, 1.6, THR, with_status=True)
    ref = rr.over_references(sc.cameras(), refs, src, 1.6, THR, sc.MATCH, sc.MATCH)
    rr.check_against_reference(ref, src, res.xyz, res.err, status, THR, 1.0)      # (a few hundred points: the cap is the probe scenes' business)
    st = status.numpy()
    assert int(st[off[1]:off[2]].max()) == 0 and unchanged(res, src, slice(off[1], off[2]))      # the one-neighbour reference is copied
    assert (st[:off[1]] & 0x80).any() and (st[off[3]:] & 0x80).any() and int((st[off[3]:] & 0x7f).max()) == 1
    for r in refs:
        r.mask_a = torch.zeros((sc.MATCH, sc.MATCH), dtype=torch.uint8)
    dead = hb.PreparedBatch(refs, sc.MATCH, sc.MATCH)
    none = twin.triangulate_dense(dead, sc.params())
    assert none.count == 0
    res, status = twin.refine_multiview(dead, none, 1.6, THR, with_status=True)
    assert res.count == 0 and res.xyz.shape[0] == 0 and status.numel() == 0


def test_a_dead_or_nan_certainty_plane_is_no_candidate(twin):
    refs, batch, src = small(twin, [(10, 3)], noise_px=0.0, outlier_frac=0.0)
    _res, st0 = twin.refine_multiview(batch, src, 1e9, THR, with_status=True)
    assert (st0.numpy() & 0x7f == 2).all()
    slot = src.slot.numpy()
    for value in (0.0, float("nan"), -0.5):
        ri = dataclasses.replace(refs[0], cert=list(refs[0].cert))
        ri.cert[1] = torch.full_like(ri.cert[1], value)
        b2 = hb.PreparedBatch([ri], sc.MATCH, sc.MATCH)
        _res, st = twin.refine_multiview(b2, src, 1e9, THR, with_status=True)    # (the same points: what is asked is who may join them)
        n = st.numpy() & 0x7f
        assert (n[slot == 1] == 2).all() and (n[slot != 1] == 1).all(), value


def test_non_finite_coordinates_in_a_neighbour_s_warp_are_no_candidate(twin):
    refs, batch, src = small(twin, [(10, 3)], noise_px=0.0, outlier_frac=0.0)
    cell, slot = src.cell.numpy(), src.slot.numpy()
    pick = np.flatnonzero(slot == 0)[:6]
    ri = dataclasses.replace(refs[0], warp=[w.clone() for w in refs[0].warp])
    for i, v in zip(pick, [float("nan"), float("inf"), float("-inf"), 3.0e38, -3.0e38, float("nan")]):
        ri.warp[1].view(-1, 2)[cell[i], i % 2] = v
    b2 = hb.PreparedBatch([ri], sc.MATCH, sc.MATCH)
    res, st = twin.refine_multiview(b2, src, 1e9, THR, with_status=True)
    n = st.numpy() & 0x7f
    assert (n[pick] == 1).all() and (np.delete(n, pick) == 2).all()
    assert np.isfinite(res.xyz.numpy()).all() and np.isfinite(res.err.numpy()).all()
    # ... and in the WINNER's own warp: whatever the solve makes of it, the point falls back
    ri2 = dataclasses.replace(refs[0], warp=[w.clone() for w in refs[0].warp])
    ri2.warp[0].view(-1, 2)[cell[pick[0]], 0] = float("nan")
    ri2.warp[0].view(-1, 2)[cell[pick[1]], 1] = float("inf")
    res2, st2 = twin.refine_multiview(hb.PreparedBatch([ri2], sc.MATCH, sc.MATCH), src, 1e9, THR, with_status=True)
    assert (st2.numpy()[pick[:2]] == 2).all() and unchanged(res2, src, pick[:2])


def test_a_point_behind_a_neighbour_or_outside_the_grid_is_copied(twin):
    refs, batch, src = small(twin, [(10, 3)], noise_px=0.0, outlier_frac=0.0)
    moved = dataclasses.replace(src, xyz=src.xyz.clone(), cell=src.cell.clone(), slot=src.slot.clone())
    cams = sc.cameras()
    moved.xyz[0] = torch.from_numpy(np.asarray(cams[refs[0].nbr_cams[1]].C, np.float32) * 3.0)       # behind neighbour 1 (and far from the others' rays)
    moved.cell[1] = 24 * 32                                                      # one past the grid
    moved.cell[2] = -1
    moved.slot[3] = 7                                                            # a slot the reference does not have
    res, st = twin.refine_multiview(batch, moved, 1e9, THR, with_status=True)
    s = st.numpy()
    assert s[1] == 0 and s[2] == 0 and s[3] == 0 and unchanged(res, moved, slice(1, 4))
    assert (s[0] & 0x7f) <= 1 or not (s[0] & 0x80)
    assert (s[4:] & 0x7f == 2).all()


def test_planted_errors_are_not_moved_and_clean_points_are(twin):
    """The planted-error scene of DESIGN 4.8: matches slid 20 px along their epipolar line pass every two-view test and no other view agrees with
    them - none has a candidate, none is moved; the clean points all are candidates of both other views."""
    k, H, W, tau = 3, 48, 48, 1.6
    cams = sc.cameras()
    _s, ri = sc.reference_inputs(10, k, H, W, noise_px=0.0, outlier_frac=0.0)
    clean = twin.triangulate_dense(hb.PreparedBatch([ri], sc.MATCH, sc.MATCH), sc.params())
    cell0, slot0, xyz0 = clean.cell.numpy(), clean.slot.numpy(), clean.xyz.numpy()
    planted = np.random.RandomState(1).choice(clean.count, size=200, replace=False)
    for j in range(k):
        mine = planted[slot0[planted] == j]
        xn, yn = _epipolar_shift(cams, 10, ri.nbr_cams[j], xyz0[mine], 20.0)
        inside = (np.abs(xn) < 0.98) & (np.abs(yn) < 0.98)
        w = ri.warp[j].view(-1, 2)
        w[cell0[mine[inside]], 0] = torch.from_numpy(xn[inside].astype(np.float32))
        w[cell0[mine[inside]], 1] = torch.from_numpy(yn[inside].astype(np.float32))
    batch = hb.PreparedBatch([ri], sc.MATCH, sc.MATCH)
    src = twin.triangulate_dense(batch, sc.params())
    cell = src.cell.numpy()
    shifted = np.isin(cell, cell0[planted]) & (np.linalg.norm(src.xyz.numpy() - xyz0[np.searchsorted(cell0, cell)], axis=1) > 1e-3)
    untouched = ~np.isin(cell, cell0[planted])
    assert shifted.sum() > 100
    res, status = twin.refine_multiview(batch, src, tau, float(sc.params().reproj_thresh), with_status=True)
    st = status.numpy()
    assert (st[shifted] == 0).all() and unchanged(res, src, shifted)
    assert (st[untouched] & 0x7f == k - 1).all() and (st[untouched] & 0x80).mean() > 0.99
    assert (rr.bits(res.xyz)[untouched] != rr.bits(src.xyz)[untouched]).any(axis=1).mean() > 0.5
