"""CPU tier of the precision-weighted re-triangulation: the twin (lfd_refine_multiview_weighted_host) against the f64 reference of
tests/wrefine_ref.py, the gain over the unweighted call against the noise-free truth, the exact properties of the contract and
its edge cases.  The probe scenes are 4.8's (ring of 40 cameras, reference 10, tie-free certainty, 5 % outliers) with noise_model="hetero";
two-view points from the twin's dense call at reproj_thresh 0.8.  The measured figures are in DESIGN.md 4.10."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import refine_ref as rr
import support_scene as sc
import wrefine_ref as wr
import wrefine_scene as ws
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from test_support_filter_host import _epipolar_shift

THR = ws.THR
REF_BAND_CAP = 0.004     # the f64 reference alone must stay at or below this share before the twin is held to sc.BAND_CAP (0.5 %)
# weighted / unweighted median distance to the truth as the f64 reference measures it on the seeded scenes, + 0.05 absolute
RATIO_BOUND = {(3, 48, 64): 0.936 + 0.05, (8, 29, 37): 0.777 + 0.05}
_cache = {}


@pytest.fixture(scope="module")
def twin():
    d = hb.HostDensifier(4)
    d.upload_cameras(sc.cameras())
    yield d
    d.close()


def probe(twin, k, H, W, channels=2, masks=False, noise_model="hetero"):
    """One reference of the probe scene triangulated by the twin's dense call, the noise-free truth of its points: computed once per module."""
    key = (k, H, W, channels, masks, noise_model)
    if key not in _cache:
        ri = ws.reference_inputs(10, k, H, W, channels=channels, masks=masks, noise_model=noise_model)
        batch = hb.PreparedBatch([ri], sc.MATCH, sc.MATCH)
        src = twin.triangulate_dense(batch, sc.params(reproj_thresh=THR))
        _cache[key] = (ri, batch, src, ws.truth_of(ri, src, H, W, channels))
    return _cache[key]


_refs = {}


def reference_of(key, ri, src, tau):
    if (key, tau) not in _refs:
        _refs[(key, tau)] = wr.over_references(sc.cameras(), [ri], src, tau, THR, sc.MATCH, sc.MATCH)
    return _refs[(key, tau)]


CASES = [(3, 48, 64, 2, False, 1.6), (8, 29, 37, 4, False, 3.0), (3, 48, 64, 2, True, 1.6)]
case_id = lambda c: f"k{c[0]}_{c[2]}x{c[1]}_c{c[3]}{'_masks' if c[4] else ''}_tau{c[5]}"


@pytest.mark.parametrize("case", CASES[:2], ids=case_id)
def test_the_reference_alone_stays_under_its_band_cap(twin, case):
    k, H, W, channels, masks, tau = case
    ri, _batch, src, _truth = probe(twin, k, H, W, channels, masks)
    ref = reference_of(case, ri, src, tau)
    has = ref["n_extra"] > 0
    n_has, n_band = int(has.sum()), int((has & ref["band"]).sum())
    print(f"{case}: {src.count} points, {n_has} with a candidate, {n_band} in band ({100.0 * n_band / max(n_has, 1):.3f} %)")
    assert n_has > 500 and n_band <= REF_BAND_CAP * n_has


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_twin_takes_the_reference_decision_outside_the_band(twin, case):
    k, H, W, channels, masks, tau = case
    ri, batch, src, _truth = probe(twin, k, H, W, channels, masks)
    counters = torch.zeros(3, dtype=torch.int64)
    res, status = twin.refine_multiview(batch, src, tau, THR, with_status=True, counters=counters, precision=True)
    ref = reference_of(case, ri, src, tau)
    n_has, n_band, n_acc, n_fall, n_w = wr.check_against_reference(ref, src, res.xyz, res.err, status, THR, sc.BAND_CAP)
    print(f"{case}: {src.count} points, {n_has} with a candidate, {n_acc} refined, {n_fall} fallen back, {n_w} weighted, {n_band} in band "
          f"({100.0 * n_band / max(n_has, 1):.3f} %)")
    st = status.numpy()
    assert np.array_equal((st & 0x40) != 0, ref["weighted"])                 # validity is decided exactly: no band
    assert src.count > 900 and n_has > 0.4 * src.count and n_acc > 0.5 * n_has and n_fall > 20 and n_w == n_has      # (the scene exercises both ends)
    assert counters.tolist() == [n_acc, n_fall, n_w]
    assert (res.err.numpy()[(st & 0x80) != 0] <= np.float32(THR)).all()
    for name in ("rgb", "cell", "slot"):
        assert np.array_equal(rr.bits(getattr(res, name)), rr.bits(getattr(src, name)))
    assert np.array_equal(res.ref_offsets, src.ref_offsets) and np.array_equal(res.seg_counts, src.seg_counts)
    # the candidates are the support filter's own count, and the unweighted call's, bit for bit
    _f, sup = twin.support_filter(batch, src, 1, tau, with_support=True)
    assert np.array_equal(st & 0x3f, sup.numpy())
    _u, st_u = twin.refine_multiview(batch, src, tau, THR, with_status=True)
    assert np.array_equal(st & 0x3f, st_u.numpy() & 0x7f)
    again, status2 = twin.refine_multiview(batch, src, tau, THR, with_status=True, counters=counters, precision=True)
    assert counters.tolist() == [2 * n_acc, 2 * n_fall, 2 * n_w] and torch.equal(status, status2)
    assert np.array_equal(rr.bits(again.xyz), rr.bits(res.xyz)) and np.array_equal(rr.bits(again.err), rr.bits(res.err))


def medians(truth, has, *clouds):
    return [float(np.median(np.linalg.norm(np.asarray(x, np.float64) - truth, axis=1)[has])) for x in clouds]


@pytest.mark.parametrize("case", CASES[:2], ids=case_id)
def test_weighted_points_are_closer_to_the_truth_than_unweighted_ones(twin, case):
    """Median distance to the noise-free truth over the points with a candidate: first the reference's own output, then the twin's, against the
    unweighted call on the same input points and against the two-view points."""
    k, H, W, channels, masks, tau = case
    ri, batch, src, truth = probe(twin, k, H, W, channels, masks)
    ref = reference_of(case, ri, src, tau)
    unw, st_u = twin.refine_multiview(batch, src, tau, THR, with_status=True)
    res, st_w = twin.refine_multiview(batch, src, tau, THR, with_status=True, precision=True)
    has = ref["n_extra"] > 0
    assert np.array_equal(has, (st_w.numpy() & 0x3f) > 0)
    before, by_unw, by_ref, by_twin = medians(truth, has, src.xyz.numpy(), unw.xyz.numpy(), ref["xyz"], res.xyz.numpy())
    bound = RATIO_BOUND[(k, H, W)]
    print(f"k={k} {W}x{H} tau {tau}: median distance to the truth {before:.5f}; unweighted {by_unw:.5f} ({by_unw / before:.3f}); weighted "
          f"reference {by_ref:.5f} ({by_ref / before:.3f}, {by_ref / by_unw:.4f} of unweighted); twin {by_twin:.5f} ({by_twin / by_unw:.4f})")
    assert bound < 1.0
    assert by_ref < by_unw and by_ref < before and by_ref <= bound * by_unw
    assert by_twin < by_unw and by_twin < before and by_twin <= bound * by_unw


def test_homoscedastic_planes_do_not_lose_to_the_unweighted_solve(twin):
    k, H, W = 3, 48, 64
    ri, batch, src, truth = probe(twin, k, H, W, noise_model="iid")
    unw, _s = twin.refine_multiview(batch, src, 1.6, THR, with_status=True)
    res, st = twin.refine_multiview(batch, src, 1.6, THR, with_status=True, precision=True)
    has = (st.numpy() & 0x3f) > 0
    by_unw, by_w = medians(truth, has, unw.xyz.numpy(), res.xyz.numpy())
    print(f"iid planes: unweighted {by_unw:.5f}, weighted {by_w:.5f} ({by_w / by_unw:.4f})")
    assert has.sum() > 2000 and (st.numpy()[has] & 0x40).all() and by_w <= by_unw


# ---- exact properties ----------------------------------------------------------------------------------------------------------------------------
def same_bits(a, b, rows=slice(None)):
    return np.array_equal(rr.bits(a.xyz)[rows], rr.bits(b.xyz)[rows]) and np.array_equal(rr.bits(a.err)[rows], rr.bits(b.err)[rows])


@pytest.mark.parametrize("values", [(float("nan"),) * 3, (0.0, 0.0, 0.0), (1.0, 2.0, 1.0), (1.0, 0.0, float("inf")), (-1.0, 0.0, -1.0)],
                         ids=["nan", "zero", "indefinite", "inf", "negative"])
def test_invalid_planes_everywhere_give_the_unweighted_call_bit_for_bit(twin, values):
    ri, batch, src, _t = probe(twin, 3, 48, 64)
    bad = hb.PreparedBatch([ws.filled(ri, values)], sc.MATCH, sc.MATCH)
    cu, cw = torch.zeros(2, dtype=torch.int64), torch.zeros(3, dtype=torch.int64)
    unw, st_u = twin.refine_multiview(batch, src, 1.6, THR, with_status=True, counters=cu)
    res, st_w = twin.refine_multiview(bad, src, 1.6, THR, with_status=True, counters=cw, precision=True)
    assert torch.equal(st_u, st_w) and not (st_w & 0x40).any() and same_bits(res, unw) and cw.tolist() == cu.tolist() + [0]
    assert int((st_w & 0x80 != 0).sum()) > 1000


def test_an_invalid_patch_in_one_slot_falls_back_exactly_where_that_slot_takes_part(twin):
    k, H, W, tau = 3, 48, 64, 1.6
    ri, batch, src, _t = probe(twin, k, H, W)
    planes = [q.clone() for q in ri.precision]
    planes[1][10:30, 20:50] = torch.tensor([1.0, 5.0, 1.0])                   # indefinite
    planes[1][12, 22] = float("nan")
    patched = hb.PreparedBatch([ws.with_planes(ri, planes)], sc.MATCH, sc.MATCH)
    unw, st_u = twin.refine_multiview(batch, src, tau, THR, with_status=True)
    full, st_f = twin.refine_multiview(batch, src, tau, THR, with_status=True, precision=True)
    res, st = twin.refine_multiview(patched, src, tau, THR, with_status=True, precision=True)
    cell, slot = src.cell.numpy(), src.slot.numpy()
    y, x = cell // W, cell % W
    in_patch = (y >= 10) & (y < 30) & (x >= 20) & (x < 50)
    cand1 = wr.reference(sc.cameras(), ri.ref_cam, ri.nbr_cams, [c.numpy() for c in ri.cert], [w.numpy() for w in ri.warp], None,
                         [q.numpy() for q in planes], sc.MATCH, sc.MATCH, cell, slot, src.xyz.numpy(), src.err.numpy(), tau, THR)["cand"][:, 1]
    part = in_patch & ((slot == 1) | cand1)
    s = st.numpy()
    assert part.sum() > 300 and (~part & (s & 0x3f > 0)).sum() > 1000
    assert not (s[part] & 0x40).any() and np.array_equal(s[part], st_u.numpy()[part]) and same_bits(res, unw, part)
    assert np.array_equal(s[~part], st_f.numpy()[~part]) and same_bits(res, full, ~part)
    assert ((s[~part] & 0x3f) > 0).sum() == ((s[~part] & 0x40) != 0).sum()


def test_a_common_scale_of_the_planes_changes_nothing(twin):
    ri, batch, src, _t = probe(twin, 8, 29, 37, 4)
    scaled = hb.PreparedBatch([ws.with_planes(ri, [q * 4.0 for q in ri.precision])], sc.MATCH, sc.MATCH)
    a, st_a = twin.refine_multiview(batch, src, 3.0, THR, with_status=True, precision=True)
    b, st_b = twin.refine_multiview(scaled, src, 3.0, THR, with_status=True, precision=True)
    assert torch.equal(st_a, st_b) and int((st_a & 0x80 != 0).sum()) > 500
    np.testing.assert_allclose(b.xyz.numpy(), a.xyz.numpy(), rtol=1e-6, atol=0)


def test_in_place_and_out_of_place_give_the_same_bits(twin):
    refs = [ws.reference_inputs(ref, k, 24, 32) for ref, k in ((10, 3), (20, 2))]
    batch = hb.PreparedBatch(refs, sc.MATCH, sc.MATCH)
    buf = hb.OutputBuffers(2 * 24 * 32, 2, 3, torch.device("cpu"))
    assert twin._lib.lfd_triangulate_dense_host(twin._ctx, C.byref(batch.c), C.byref(sc.params(reproj_thresh=THR)), C.byref(buf.c),
                                                buf.ref_offsets.data_ptr(), buf.seg_counts.data_ptr()) == 0
    src = buf.collect()
    src = dataclasses.replace(src, xyz=src.xyz.clone(), err=src.err.clone(), rgb=src.rgb.clone(), _packed=None)
    copy, st_copy = twin.refine_multiview(batch, src, 1.6, THR, with_status=True, precision=True)
    assert copy.xyz.data_ptr() != src.xyz.data_ptr()
    same, st_same = twin.refine_multiview(batch, buf, 1.6, THR, with_status=True, precision=True)
    assert same is buf and st_same.numel() == buf.capacity
    got = buf.collect()
    assert same_bits(got, copy)
    assert np.array_equal(rr.bits(got.rgb), rr.bits(src.rgb)) and torch.equal(got.cell, src.cell) and torch.equal(got.slot, src.slot)
    assert np.array_equal(got.ref_offsets, src.ref_offsets)
    assert torch.equal(st_same[:src.count], st_copy) and int((st_copy & 0x80 != 0).sum()) > 100
    moved = (rr.bits(copy.xyz) != rr.bits(src.xyz)).any(axis=1)
    assert not moved[(st_copy.numpy() & 0x80) == 0].any()                      # every fallback is its input bit for bit
    assert (copy.err.numpy()[(st_copy.numpy() & 0x80) != 0] <= np.float32(THR)).all()
    with pytest.raises(ValueError, match="counters"):
        twin.refine_multiview(batch, buf, 1.6, THR, counters=torch.zeros(2, dtype=torch.int64), precision=True)
    plain = hb.PreparedBatch([dataclasses.replace(r, precision=None) for r in refs], sc.MATCH, sc.MATCH)
    with pytest.raises(ValueError, match="precision"):
        twin.refine_multiview(plain, buf, 1.6, THR, precision=True)
    with pytest.raises(ValueError, match="every reference"):
        hb.PreparedBatch([refs[0], dataclasses.replace(refs[1], precision=None)], sc.MATCH, sc.MATCH)


# ---- edge cases (the list of DESIGN 4.9) ------------------------------------------------------------------------------------------------------------
def small(twin, spec, H=24, W=32, **kw):
    refs = [ws.reference_inputs(ref, k, H, W, **kw) for ref, k in spec]
    batch = hb.PreparedBatch(refs, sc.MATCH, sc.MATCH)
    return refs, batch, twin.triangulate_dense(batch, sc.params(reproj_thresh=THR))


def wcall(twin, batch, src, tau=1e9, **kw):
    return twin.refine_multiview(batch, src, tau, THR, with_status=True, precision=True, **kw)


def test_one_neighbour_has_nobody_to_ask(twin):
    refs, batch, src = small(twin, [(10, 1)])
    counters = torch.zeros(3, dtype=torch.int64)
    res, status = wcall(twin, batch, src, counters=counters)
    assert src.count > 300 and int(status.max()) == 0 and same_bits(res, src) and counters.tolist() == [0, 0, 0]


def test_ragged_slots_an_empty_reference_and_an_empty_cloud(twin):
    refs = [ws.reference_inputs(ref, k, 24, 32) for ref, k in ((10, 3), (20, 1), (30, 3), (35, 2))]
    refs[2].mask_a = torch.zeros((sc.MATCH, sc.MATCH), dtype=torch.uint8)         # masked out: a reference with 0 points
    batch = hb.PreparedBatch(refs, sc.MATCH, sc.MATCH)
    src = twin.triangulate_dense(batch, sc.params(reproj_thresh=THR))
    off = src.ref_offsets
    assert off[1] > 0 and off[2] > off[1] and off[3] == off[2] and off[4] > off[3]
    res, status = wcall(twin, batch, src, 1.6)
    ref = wr.over_references(sc.cameras(), refs, src, 1.6, THR, sc.MATCH, sc.MATCH)
    wr.check_against_reference(ref, src, res.xyz, res.err, status, THR, 1.0)      # (a few hundred points: the cap is the probe scenes' business)
    st = status.numpy()
    assert int(st[off[1]:off[2]].max()) == 0 and same_bits(res, src, slice(off[1], off[2]))      # the one-neighbour reference is copied
    assert (st[:off[1]] & 0xc0 == 0xc0).any() and (st[off[3]:] & 0xc0 == 0xc0).any() and int((st[off[3]:] & 0x3f).max()) == 1
    for r in refs:
        r.mask_a = torch.zeros((sc.MATCH, sc.MATCH), dtype=torch.uint8)
    dead = hb.PreparedBatch(refs, sc.MATCH, sc.MATCH)
    none = twin.triangulate_dense(dead, sc.params())
    assert none.count == 0
    res, status = wcall(twin, dead, none, 1.6)
    assert res.count == 0 and res.xyz.shape[0] == 0 and status.numel() == 0


def test_a_dead_or_nan_certainty_plane_is_no_candidate(twin):
    refs, batch, src = small(twin, [(10, 3)], noise_px=0.0, outlier_frac=0.0, noise_model="iid")
    _res, st0 = wcall(twin, batch, src)
    assert (st0.numpy() & 0x3f == 2).all() and (st0.numpy() & 0x40).all()
    slot = src.slot.numpy()
    for value in (0.0, float("nan"), -0.5):
        ri = dataclasses.replace(refs[0], cert=list(refs[0].cert))
        ri.cert[1] = torch.full_like(ri.cert[1], value)
        _res, st = wcall(twin, hb.PreparedBatch([ri], sc.MATCH, sc.MATCH), src)
        n = st.numpy() & 0x3f
        assert (n[slot == 1] == 2).all() and (n[slot != 1] == 1).all(), value


def test_non_finite_coordinates_in_a_warp_are_no_candidate_and_never_leak(twin):
    refs, batch, src = small(twin, [(10, 3)], noise_px=0.0, outlier_frac=0.0, noise_model="iid")
    cell, slot = src.cell.numpy(), src.slot.numpy()
    pick = np.flatnonzero(slot == 0)[:6]
    ri = dataclasses.replace(refs[0], warp=[w.clone() for w in refs[0].warp])
    for i, v in zip(pick, [float("nan"), float("inf"), float("-inf"), 3.0e38, -3.0e38, float("nan")]):
        ri.warp[1].view(-1, 2)[cell[i], i % 2] = v
    res, st = wcall(twin, hb.PreparedBatch([ri], sc.MATCH, sc.MATCH), src)
    n = st.numpy() & 0x3f
    assert (n[pick] == 1).all() and (np.delete(n, pick) == 2).all()
    assert np.isfinite(res.xyz.numpy()).all() and np.isfinite(res.err.numpy()).all()
    ri2 = dataclasses.replace(refs[0], warp=[w.clone() for w in refs[0].warp])          # ... in the WINNER's own warp: the point falls back
    ri2.warp[0].view(-1, 2)[cell[pick[0]], 0] = float("nan")
    ri2.warp[0].view(-1, 2)[cell[pick[1]], 1] = float("inf")
    res2, st2 = wcall(twin, hb.PreparedBatch([ri2], sc.MATCH, sc.MATCH), src)
    assert (st2.numpy()[pick[:2]] & 0xbf == 2).all() and same_bits(res2, src, pick[:2])


def test_a_point_behind_a_neighbour_or_outside_the_grid_is_copied(twin):
    refs, batch, src = small(twin, [(10, 3)], noise_px=0.0, outlier_frac=0.0, noise_model="iid")
    moved = dataclasses.replace(src, xyz=src.xyz.clone(), cell=src.cell.clone(), slot=src.slot.clone())
    cams = sc.cameras()
    moved.xyz[0] = torch.from_numpy(np.asarray(cams[refs[0].nbr_cams[1]].C, np.float32) * 3.0)       # behind neighbour 1
    moved.cell[1] = 24 * 32                                                      # one past the grid
    moved.cell[2] = -1
    moved.slot[3] = 7                                                            # a slot the reference does not have
    res, st = wcall(twin, batch, moved)
    s = st.numpy()
    assert s[1] == 0 and s[2] == 0 and s[3] == 0 and same_bits(res, moved, slice(1, 4))
    assert (s[0] & 0x3f) <= 1 or not (s[0] & 0x80)
    assert (s[4:] & 0x3f == 2).all()
    assert np.isfinite(res.xyz.numpy()).all()


def test_planted_errors_are_not_moved(twin):
    """The planted-error scene of DESIGN 4.8: matches slid 20 px along their epipolar line have no candidate - none is moved, weights or not."""
    k, H, W, tau = 3, 48, 48, 1.6
    cams = sc.cameras()
    ri = ws.reference_inputs(10, k, H, W, noise_px=0.0, outlier_frac=0.0, noise_model="iid")
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
    res, status = twin.refine_multiview(batch, src, tau, float(sc.params().reproj_thresh), with_status=True, precision=True)
    st = status.numpy()
    assert (st[shifted] == 0).all() and same_bits(res, src, shifted)
    assert (st[untouched] & 0x3f == k - 1).all() and (st[untouched] & 0x40).all() and (st[untouched] & 0x80).mean() > 0.99
