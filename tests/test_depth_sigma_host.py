"""CPU tier of the depth-uncertainty gate: the twin (lfd_depth_sigma_filter_host) against the f64 reference of tests/depth_sigma_ref.py, the
calibration of sigma_rel against the noise-free truth, its usefulness on a low-parallax patch, the exact properties of the contract (DESIGN.md
4.11) and its edge cases.  The probe scenes are 4.8's and 4.10's (ring of 40 cameras, reference 10, tie-free certainty); two-view points from
the twin's dense call at reproj_thresh 0.8.  The measured figures are in DESIGN.md 4.11."""
import dataclasses

import numpy as np
import pytest
import torch

import depth_sigma_ref as dr
import refine_ref as rr
import support_scene as sc
import wrefine_scene as ws
from lichtfeld_densification_plugin_amd import synthetic as syn
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

THR = ws.THR
NOISE = 0.5              # iid matching noise of the probe scene: camera px of the neighbour (synthetic.synth_reference), sigma_rel's own unit
GAUSS_MEDIAN = 0.6745    # median |z| of a standard normal
_cache = {}


@pytest.fixture(scope="module")
def twin():
    d = hb.HostDensifier(4)
    d.upload_cameras(sc.cameras())
    yield d
    d.close()


def probe(twin, k, H, W, channels=2, masks=False, noise_model="hetero", outlier_frac=0.05):
    """One reference of the probe scene triangulated by the twin's dense call, the noise-free truth of its points: computed once per module."""
    key = (k, H, W, channels, masks, noise_model, outlier_frac)
    if key not in _cache:
        ri = ws.reference_inputs(10, k, H, W, channels=channels, masks=masks, noise_model=noise_model, noise_px=NOISE, outlier_frac=outlier_frac)
        batch = hb.PreparedBatch([ri], sc.MATCH, sc.MATCH)
        src = twin.triangulate_dense(batch, sc.params(reproj_thresh=THR))
        _cache[key] = (ri, batch, src, ws.truth_of(ri, src, H, W, channels))
    return _cache[key]


def refined(twin, key, tau, weighted=True):
    """The probe's points through the (weighted) re-triangulation with status: once per module."""
    ck = ("refined", key, tau, weighted)
    if ck not in _cache:
        _ri, batch, src, _t = probe(twin, *key)
        _cache[ck] = twin.refine_multiview(batch, src, tau, THR, with_status=True, precision=weighted)
    return _cache[ck]


def sigma_of(twin, batch, src, max_rel=0.0, iso=0.0, status=None, tau=0.0):
    return twin.depth_sigma_filter(batch, src, max_rel, iso_sigma_px=iso, refine_status=status, support_thresh_px=tau, with_sigma=True)


def C_A():
    return np.asarray(sc.cameras()[10].C, np.float32)


def median_abs_z(xyz, truth, sigma, rows):
    z = dr.depth_z(xyz, truth, C_A(), sigma)
    rows = rows & np.isfinite(z)
    return float(np.median(np.abs(z[rows]))), int(rows.sum())


# ---- twin against reference -------------------------------------------------------------------------------------------------------------------
CASES = [((3, 48, 64, 2, False, "iid"), "iso", None), ((3, 48, 64, 2, False, "hetero"), "planes", None),
         ((3, 48, 64, 2, False, "hetero"), "planes", 1.6), ((8, 29, 37, 4, False, "hetero"), "planes", 3.0),
         ((3, 48, 64, 2, True, "hetero"), "planes", 1.6), ((8, 29, 37, 4, False, "hetero"), "iso", 3.0)]
case_id = lambda c: f"k{c[0][0]}_{c[0][2]}x{c[0][1]}_c{c[0][3]}{'_masks' if c[0][4] else ''}_{c[0][5]}_{c[1]}_{'winner' if c[2] is None else 'status'}"


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_twin_agrees_with_the_reference(twin, case):
    key, form, tau = case
    ri, batch, src, _truth = probe(twin, *key)
    status = None
    if tau is not None:
        src, status = refined(twin, key, tau)
    iso = NOISE if form == "iso" else 0.0
    res, sigma, sigma_out = sigma_of(twin, batch, src, 0.0, iso, status, tau or 0.0)
    ref = dr.over_references(sc.cameras(), [ri], src, sc.MATCH, sc.MATCH, status, tau or 0.0, iso)
    got = sigma.numpy().astype(np.float64)
    clean = ~ref["band"]
    n_band = int(ref["band"].sum())
    fin = np.isfinite(ref["sigma"])
    rel = np.abs(got[clean & fin] - ref["sigma"][clean & fin]) / ref["sigma"][clean & fin]
    print(f"{case_id(case)}: {src.count} points, {int(fin.sum())} finite, {n_band} in the candidates' band, largest relative difference "
          f"{rel.max():.3e}, views per point {ref['n_views'].mean():.2f}")
    assert src.count > 900 and fin.sum() > 0.9 * src.count and n_band <= sc.BAND_CAP * src.count
    assert np.array_equal(np.isinf(got[clean]), ~fin[clean]) and not np.isnan(got).any()
    assert rel.max() <= 1e-6
    if tau is not None:
        assert (ref["n_views"] > 1).sum() > 0.3 * src.count          # (the status form has candidates to count)
    # annotate only: everything is copied
    assert sc.same_points(res, src) and np.array_equal(rr.bits(sigma_out), rr.bits(sigma))


# ---- calibration ------------------------------------------------------------------------------------------------------------------------------
def test_two_view_sigma_is_calibrated(twin):
    """median |z| of the depth error along the ray over the predicted sigma: the f64 reference first, then the twin, in 0.6745 +- 0.07."""
    key = (3, 48, 64, 2, False, "iid", 0.05)
    ri, batch, src, truth = probe(twin, *key)
    ref = dr.over_references(sc.cameras(), [ri], src, sc.MATCH, sc.MATCH, None, 0.0, NOISE)
    all_rows = np.ones(src.count, bool)
    m_ref, n = median_abs_z(src.xyz.numpy(), truth, ref["sigma"], all_rows)
    _res, sigma, _so = sigma_of(twin, batch, src, 0.0, NOISE)
    m_twin, _n = median_abs_z(src.xyz.numpy(), truth, sigma.numpy(), all_rows)
    print(f"two-view, iid {NOISE} px, 5 % outliers: {n} points, median |z| reference {m_ref:.4f}, twin {m_twin:.4f} (Gaussian {GAUSS_MEDIAN})")
    assert n > 2500
    assert abs(m_ref - GAUSS_MEDIAN) <= 0.07
    assert abs(m_twin - GAUSS_MEDIAN) <= 0.07


def test_weighted_n_view_sigma_is_calibrated_and_the_unweighted_solve_is_not_efficient(twin):
    key, tau = (8, 29, 37, 2, False, "hetero", 0.05), 3.0
    ri, batch, src, truth = probe(twin, *key)
    res_w, st_w = refined(twin, key, tau, True)
    res_u, st_u = refined(twin, key, tau, False)
    acc = (st_w.numpy() & 0x80) != 0
    acc_both = acc & ((st_u.numpy() & 0x80) != 0)
    ref = dr.over_references(sc.cameras(), [ri], res_w, sc.MATCH, sc.MATCH, st_w, tau, 0.0)
    m_ref, n = median_abs_z(res_w.xyz.numpy(), truth, ref["sigma"], acc)
    _r, sigma, _so = sigma_of(twin, batch, res_w, 0.0, 0.0, st_w, tau)
    m_twin, _n = median_abs_z(res_w.xyz.numpy(), truth, sigma.numpy(), acc)
    # the same points through the unweighted refinement, against the sigma of the views that placed them
    _r, sigma_u, _so = sigma_of(twin, batch, res_u, 0.0, 0.0, st_u, tau)
    m_w_both, _n = median_abs_z(res_w.xyz.numpy(), truth, sigma.numpy(), acc_both)
    m_unw, n_u = median_abs_z(res_u.xyz.numpy(), truth, sigma_u.numpy(), acc_both)
    print(f"weighted N-view, hetero, k 8: {n} accepted points, median |z| reference {m_ref:.4f}, twin {m_twin:.4f}; over the {n_u} points both "
          f"refinements accepted: weighted {m_w_both:.4f}, unweighted {m_unw:.4f}")
    assert n > 400
    assert 0.6 <= m_twin <= m_ref + 0.05
    assert abs(m_ref - REF_WEIGHTED_MEDIAN) <= 0.002                   # (the value DESIGN.md 4.11 quotes)
    assert m_unw > m_w_both


REF_WEIGHTED_MEDIAN = 0.768      # median |z| of the f64 reference on the seeded 37 x 29, k = 8 hetero scene


# ---- usefulness -------------------------------------------------------------------------------------------------------------------------------
def test_gating_at_the_median_sigma_drops_the_worse_depths(twin):
    """A scene with a low-parallax patch (depths 6 .. 60 along x) and the parallax test set low enough to let it through: the points the gate
    drops at the median sigma have the larger relative depth error."""
    H, W, k = 48, 64, 3
    nbrs = syn.ring_neighbours(sc.N_CAMS, 10, k)
    kw = dict(channels=2, seed=0, cert_mode="tiefree", low_parallax_patch=(0.2, 0.7, 0.1, 0.9), patch_depths=(6.0, 60.0))
    s = syn.synth_reference(sc.cameras(), 10, nbrs, H, W, sc.MATCH, sc.MATCH, noise_px=NOISE, **kw)
    clean = syn.synth_reference(sc.cameras(), 10, nbrs, H, W, sc.MATCH, sc.MATCH, noise_px=0.0, **kw)
    ri = hb.ReferenceInputs(ref_cam=10, nbr_cams=nbrs, cert=[s.cert[j] for j in range(k)], warp=[s.warp[j] for j in range(k)], image=s.image)
    batch = hb.PreparedBatch([ri], sc.MATCH, sc.MATCH)
    src = twin.triangulate_dense(batch, sc.params(reproj_thresh=THR, min_parallax_deg=0.02))
    truth = rr.two_view_f64(sc.cameras(), 10, nbrs, [clean.warp[j].numpy() for j in range(k)], sc.MATCH, sc.MATCH, src.cell.numpy(), src.slot.numpy())
    cell = src.cell.numpy()
    in_patch = ((cell // W >= int(0.2 * H)) & (cell // W < int(0.7 * H)) & (cell % W >= int(0.1 * W)) & (cell % W < int(0.9 * W)))
    _r, sigma, _so = sigma_of(twin, batch, src, 0.0, NOISE)
    sg = sigma.numpy()
    med = float(np.median(sg))
    res, sigma2, sigma_out = sigma_of(twin, batch, src, med, NOISE)
    keep = sg <= np.float32(med)
    err = np.abs(dr.depth_z(src.xyz.numpy(), truth, C_A(), np.ones(src.count)))         # relative depth error itself
    e_keep, e_drop = float(np.median(err[keep])), float(np.median(err[~keep]))
    print(f"low-parallax patch: {src.count} points, {int(in_patch.sum())} in the patch, median sigma {med:.5f}; median relative depth error kept "
          f"{e_keep:.6f}, dropped {e_drop:.6f}; {int((in_patch & ~keep).sum())} patch points dropped")
    assert in_patch.sum() >= 300 and 0 < keep.sum() < src.count
    assert e_drop > e_keep
    assert res.count == int(keep.sum()) and np.array_equal(rr.bits(sigma_out), rr.bits(sigma)[keep])


# ---- exact properties -------------------------------------------------------------------------------------------------------------------------
KEY3 = (3, 48, 64, 2, False, "hetero", 0.05)
TAU3 = 1.6


def scaled(ri, f):
    return ws.with_planes(ri, [q * f for q in ri.precision])


@pytest.mark.parametrize("with_status", [False, True], ids=["winner", "status"])
def test_planes_times_four_halve_sigma_bit_for_bit(twin, with_status):
    ri, batch, src, _t = probe(twin, *KEY3)
    status = None
    if with_status:
        src, status = refined(twin, KEY3, TAU3)
    _r, a, _o = sigma_of(twin, batch, src, 0.0, 0.0, status, TAU3 if with_status else 0.0)
    b4 = hb.PreparedBatch([scaled(ri, 4.0)], sc.MATCH, sc.MATCH)
    _r, b, _o = sigma_of(twin, b4, src, 0.0, 0.0, status, TAU3 if with_status else 0.0)
    a, b = a.numpy(), b.numpy()
    fin = np.isfinite(a)
    assert fin.sum() > 2000 and np.array_equal(np.isfinite(b), fin)
    assert np.array_equal(rr.bits(b[fin]), rr.bits((a[fin] * np.float32(0.5)).astype(np.float32)))


def test_isotropic_form_equals_isotropic_planes(twin):
    ri, batch, src, _t = probe(twin, 3, 48, 64, 2, False, "iid", 0.05)      # (its planes are I / NOISE^2 in camera px, written in match px^-2)
    src, status = refined(twin, (3, 48, 64, 2, False, "iid", 0.05), TAU3)
    for st, tau in ((None, 0.0), (status, TAU3)):
        _r, a, _o = sigma_of(twin, batch, src, 0.0, NOISE, st, tau)
        _r, b, _o = sigma_of(twin, batch, src, 0.0, 0.0, st, tau)
        a, b = a.numpy().astype(np.float64), b.numpy().astype(np.float64)
        fin = np.isfinite(a)
        assert fin.sum() > 2000 and np.array_equal(np.isfinite(b), fin)
        assert (np.abs(a[fin] - b[fin]) <= 1e-6 * a[fin]).all()


@pytest.mark.parametrize("with_status", [False, True], ids=["winner", "status"])
def test_gate_keeps_exactly_the_points_at_or_below_the_threshold(twin, with_status):
    ri, batch, src, _t = probe(twin, *KEY3)
    status, tau = None, 0.0
    if with_status:
        (src, status), tau = refined(twin, KEY3, TAU3), TAU3
    res0, sigma, sigma_out0 = sigma_of(twin, batch, src, 0.0, 0.0, status, tau)
    assert sc.same_points(res0, src) and np.array_equal(rr.bits(sigma_out0), rr.bits(sigma)) and res0.sigma_in == src.count
    sg = sigma.numpy()
    for q in (0.2, 0.5, 0.9):
        mx = float(np.quantile(sg[np.isfinite(sg)], q))
        res, sigma2, sigma_out = sigma_of(twin, batch, src, mx, 0.0, status, tau)
        assert np.array_equal(rr.bits(sigma2), rr.bits(sigma))
        keep = sg <= np.float32(mx)
        assert 0 < keep.sum() < src.count
        sc.check_is_stable_subset(src, res, torch.from_numpy(keep.astype(np.uint8)), 1, 3)
        assert np.array_equal(rr.bits(sigma_out), rr.bits(sigma)[keep])
    # exactly at a point's own sigma the point is kept
    res, _s, _o = sigma_of(twin, batch, src, float(np.sort(sg)[100]), 0.0, status, tau)
    assert res.count == int((sg <= np.sort(sg)[100]).sum()) >= 101


def test_status_all_zero_equals_no_status_and_unaccepted_points_have_the_winner_value(twin):
    ri, batch, src, _t = probe(twin, *KEY3)
    _r, win, _o = sigma_of(twin, batch, src)
    zero = torch.zeros(src.count, dtype=torch.uint8)
    res_z, sig_z, _o = sigma_of(twin, batch, src, 0.0, 0.0, zero, TAU3)
    assert np.array_equal(rr.bits(sig_z), rr.bits(win))
    mx = float(np.median(win.numpy()))
    a, _s, ao = sigma_of(twin, batch, src, mx)
    b, _s, bo = sigma_of(twin, batch, src, mx, 0.0, zero, TAU3)
    assert sc.same_points(a, b) and np.array_equal(rr.bits(ao), rr.bits(bo))
    # with the refinement's own status: a point without LFD_REFINE_ACCEPTED has the winner-only value of ITS position, bit for bit, and an
    # accepted one never a larger sigma than the winner alone gives it
    rsrc, status = refined(twin, KEY3, TAU3)
    _r, win_r, _o = sigma_of(twin, batch, rsrc)
    _r, full, _o = sigma_of(twin, batch, rsrc, 0.0, 0.0, status, TAU3)
    acc = (status.numpy() & 0x80) != 0
    assert acc.sum() > 1000 and (~acc).sum() > 100
    assert np.array_equal(rr.bits(full)[~acc], rr.bits(win_r)[~acc])
    assert (full.numpy()[acc] <= win_r.numpy()[acc]).all() and (full.numpy()[acc] < win_r.numpy()[acc]).sum() > 0.9 * acc.sum()


def test_one_neighbour_status_form_equals_winner_only(twin):
    ri, batch, src, _t = probe(twin, 1, 48, 64, 2, False, "hetero", 0.05)
    status = torch.full((src.count,), 0x80, dtype=torch.uint8)
    _r, a, _o = sigma_of(twin, batch, src)
    _r, b, _o = sigma_of(twin, batch, src, 0.0, 0.0, status, TAU3)
    assert src.count > 1000 and np.isfinite(a.numpy()).all() and np.array_equal(rr.bits(a), rr.bits(b))


@pytest.mark.parametrize("values", [(float("nan"),) * 3, (0.0, 0.0, 0.0), (1.0, 2.0, 1.0), (1.0, 0.0, float("inf")), (-1.0, 0.0, -1.0)],
                         ids=["nan", "zero", "indefinite", "inf", "negative"])
def test_invalid_planes_everywhere_give_inf_and_nothing_passes_the_gate(twin, values):
    ri, _b, _src, _t = probe(twin, *KEY3)
    src, status = refined(twin, KEY3, TAU3)
    bad = hb.PreparedBatch([ws.filled(ri, values)], sc.MATCH, sc.MATCH)
    res, sigma, _o = sigma_of(twin, bad, src, 0.0, 0.0, status, TAU3)
    assert np.isposinf(sigma.numpy()).all() and res.count == src.count
    res, sigma, sigma_out = sigma_of(twin, bad, src, 1e30, 0.0, status, TAU3)
    assert res.count == 0 and np.asarray(res.ref_offsets).tolist() == [0, 0] and not res.seg_counts.any() and sigma_out.numel() == 0


def test_an_invalid_patch_in_one_slot_changes_exactly_the_points_that_slot_takes_part_in(twin):
    ri, batch, _src, _t = probe(twin, *KEY3)
    src, status = refined(twin, KEY3, TAU3)
    H, W, j_bad = 48, 64, 1
    planes = [q.clone() for q in ri.precision]
    planes[j_bad][10:30, 15:50] = float("nan")
    bad = hb.PreparedBatch([ws.with_planes(ri, planes)], sc.MATCH, sc.MATCH)
    _r, a, _o = sigma_of(twin, batch, src, 0.0, 0.0, status, TAU3)
    _r, b, _o = sigma_of(twin, bad, src, 0.0, 0.0, status, TAU3)
    # where slot j_bad participates (winner, or candidate of an accepted point) inside the patch - from the twin's own candidate count
    only = [torch.zeros_like(c) if j != j_bad else c for j, c in enumerate(ri.cert)]
    _f, sup_bad = twin.support_filter(hb.PreparedBatch([dataclasses.replace(ri, cert=only)], sc.MATCH, sc.MATCH), src, 1, TAU3, with_support=True)
    cell, slot = src.cell.numpy(), src.slot.numpy()
    inside = (cell // W >= 10) & (cell // W < 30) & (cell % W >= 15) & (cell % W < 50)
    acc = (status.numpy() & 0x80) != 0
    takes_part = inside & ((slot == j_bad) | (acc & (slot != j_bad) & (sup_bad.numpy() > 0)))
    changed = rr.bits(a) != rr.bits(b)
    assert takes_part.sum() > 200 and (inside & ~takes_part).sum() > 50
    assert np.array_equal(changed, takes_part)
    assert (b.numpy()[takes_part] > a.numpy()[takes_part]).all()           # a view less: never more certain
    assert np.isposinf(b.numpy()[inside & (slot == j_bad) & ~acc]).all()


# ---- edge cases -------------------------------------------------------------------------------------------------------------------------------
def ragged_batch(twin):
    """Three references with 3, 1 and 2 loaded neighbours (k = 3): reference 1 is masked out, so it has no points."""
    if "ragged" not in _cache:
        refs = []
        for ref, kk in ((10, 3), (20, 1), (30, 2)):
            ri = ws.reference_inputs(ref, kk, 29, 37, noise_model="hetero", noise_px=NOISE)
            if ref == 20:                 # masked out: no candidate cell, a reference with 0 points
                ri = dataclasses.replace(ri, mask_a=torch.zeros((sc.MATCH, sc.MATCH), dtype=torch.uint8))
            refs.append(ri)
        batch = hb.PreparedBatch(refs, sc.MATCH, sc.MATCH)
        src = twin.triangulate_dense(batch, sc.params(reproj_thresh=THR, certainty_thresh=0.2))
        _cache["ragged"] = (refs, batch, src)
    return _cache["ragged"]


def test_ragged_slots_and_an_empty_reference_in_the_middle(twin):
    refs, batch, src = ragged_batch(twin)
    off = np.asarray(src.ref_offsets)
    assert off[1] > 300 and off[2] == off[1] and off[3] > off[2] + 300
    rsrc, status = twin.refine_multiview(batch, src, TAU3, THR, with_status=True, precision=True)
    res0, sigma, _o = sigma_of(twin, batch, rsrc, 0.0, 0.0, status, TAU3)
    ref = dr.over_references(sc.cameras(), refs, rsrc, sc.MATCH, sc.MATCH, status, TAU3, 0.0)
    got = sigma.numpy().astype(np.float64)
    clean = ~ref["band"] & np.isfinite(ref["sigma"])
    assert clean.sum() > 0.95 * src.count and (np.abs(got[clean] - ref["sigma"][clean]) <= 1e-6 * ref["sigma"][clean]).all()
    mx = float(np.median(sigma.numpy()))
    res, _s, sigma_out = sigma_of(twin, batch, rsrc, mx, 0.0, status, TAU3)
    keep = sigma.numpy() <= np.float32(mx)
    sc.check_is_stable_subset(rsrc, res, torch.from_numpy(keep.astype(np.uint8)), 1, 3)
    assert res.ref_offsets[1] == res.ref_offsets[2] and 0 < res.count < src.count


def test_zero_points(twin):
    ri, batch, src, _t = probe(twin, *KEY3)
    empty = dataclasses.replace(src, xyz=src.xyz[:0], rgb=src.rgb[:0], err=src.err[:0], cell=src.cell[:0], slot=src.slot[:0],
                                ref_offsets=np.zeros(2, np.int64), seg_counts=np.zeros((1, 3), np.int32), _packed=None)
    res, sigma, sigma_out = sigma_of(twin, batch, empty, 0.05, NOISE)
    assert res.count == 0 and sigma.numel() == 0 and sigma_out.numel() == 0 and np.asarray(res.ref_offsets).tolist() == [0, 0]
    assert not res.seg_counts.any() and res.sigma_in == 0


def test_bad_points_get_inf_and_form_no_address(twin):
    """NaN / inf coordinates, a cell outside the grid, a slot the reference does not have, a point behind a candidate."""
    ri, batch, _s, _t = probe(twin, *KEY3)
    src, status = refined(twin, KEY3, TAU3)
    xyz, cell, slot = src.xyz.clone(), src.cell.clone(), src.slot.clone()
    st = status.clone()
    xyz[0, 1] = float("nan"); xyz[1, 0] = float("inf"); xyz[2, 2] = -float("inf")
    cell[3] = -1; cell[4] = 48 * 64; cell[5] = 2 ** 31 - 1; cell[6] = -2 ** 31
    slot[7] = 3; slot[8] = 255
    bad = dataclasses.replace(src, xyz=xyz, cell=cell, slot=slot, _packed=None)
    res, sigma, _o = sigma_of(twin, batch, bad, 0.0, 0.0, st, TAU3)
    sg = sigma.numpy()
    assert np.isposinf(sg[:9]).all() and res.count == src.count
    _r, good, _o = sigma_of(twin, batch, src, 0.0, 0.0, st, TAU3)
    assert np.array_equal(rr.bits(sg[9:]), rr.bits(good.numpy()[9:]))
    res, _s, _o = sigma_of(twin, batch, bad, 1e30, 0.0, st, TAU3)
    assert res.count == int(np.isfinite(sg).sum()) and not np.isin(np.arange(9), np.flatnonzero(np.isfinite(sg))).any()
    # a point behind the winner's camera but in front of nothing else: mirrored through the reference's centre
    C = torch.from_numpy(C_A())
    behind = dataclasses.replace(src, xyz=(2.0 * C - src.xyz).contiguous(), _packed=None)
    allacc = torch.full_like(st, 0x80)
    _r, sb, _o = sigma_of(twin, batch, behind, 0.0, 0.0, allacc, 1e6)
    _r, sw, _o = sigma_of(twin, batch, behind)
    assert np.array_equal(rr.bits(sb), rr.bits(sw))                       # no candidate agrees behind its camera (pz <= 0): the winner's value
    assert np.isposinf(sw.numpy()).sum() > 0.5 * src.count               # ... and the winner itself is skipped where the point is behind it


def test_a_candidate_never_raises_sigma(twin):
    ri, batch, _s, _t = probe(twin, 8, 29, 37, 2, False, "hetero", 0.05)
    src, status = refined(twin, (8, 29, 37, 2, False, "hetero", 0.05), 3.0)
    _r, win, _o = sigma_of(twin, batch, src)
    _r, full, _o = sigma_of(twin, batch, src, 0.0, 0.0, status, 3.0)
    # fewer candidates at a tighter threshold: sigma in between
    _r, some, _o = sigma_of(twin, batch, src, 0.0, 0.0, status, 0.75)
    w, f, s = win.numpy(), full.numpy(), some.numpy()
    assert (f <= s).all() and (s <= w).all() and (f < s).sum() > 100 and (s < w).sum() > 100
