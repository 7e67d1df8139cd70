"""CPU tier of the free-space filter (lfd_freespace_filter_host): the twin - camera table, z-buffers, the per-point routine of
csrc/lfd_freespace.hpp - against the brute-force NumPy reference of tests/freespace_ref.py.  Every comparison is exact: the two counts, the kept
set, the offsets and the bits of every copied value."""
import numpy as np
import pytest
import torch

import consensus_ref as cr
import freespace_ref as fr
import freespace_scene as fs
from lichtfeld_densification_plugin_amd import synthetic
from lichtfeld_densification_plugin_amd.core import hip_backend as hb


@pytest.fixture(scope="module")
def twin():
    t = hb.HostDensifier(4)
    yield t
    t.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def call(dens, xyz, counts, P, wh, plane, tol, min_v, with_counts=True, rgb=None, err=None, device="cpu"):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device) if a is not None else None      # noqa: E731
    x, c, e, kept, v, s = dens.freespace_filter(t(xyz), t(rgb), t(err), counts, P, wh, plane, tol, min_v, with_counts)
    h = lambda a: a.cpu().numpy() if a is not None else None                                            # noqa: E731
    return h(x), h(c), h(e), np.asarray(kept), h(v), h(s)


def check_against_reference(dens, xyz, counts, P, wh, plane, tol, min_vs=(1, 2, 8), device="cpu"):
    """every output of the entry point against the reference; returns (violations, supports) of the reference"""
    xyz = np.ascontiguousarray(xyz, np.float32)
    n = xyz.shape[0]
    rng = np.random.default_rng(n + 17)
    rgb = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
    err = rng.uniform(0.0, 2.0, (n,)).astype(np.float32)
    if n > 2:
        rgb[1, 1], err[2] = np.nan, np.inf                                 # whatever travels along is copied, not looked at
    viol, supp = fr.counts_of(xyz, counts, P, wh, plane[0], plane[1], tol)
    ids = fr.ref_ids(counts)
    before = xyz.copy()
    for m in min_vs:
        keep = fr.keep_mask(viol, supp, m)
        x, c, e, kept, v, s = call(dens, xyz, counts, P, wh, plane, tol, m, True, rgb, err, device)
        assert np.array_equal(v, np.minimum(viol, 255).astype(np.uint8)), (m, np.flatnonzero(v != np.minimum(viol, 255))[:10])
        assert np.array_equal(s, np.minimum(supp, 255).astype(np.uint8)), (m, np.flatnonzero(s != np.minimum(supp, 255))[:10])
        assert np.array_equal(kept, np.bincount(ids[keep], minlength=len(counts)))
        assert np.array_equal(bits(x), bits(xyz[keep])) and np.array_equal(bits(c), bits(rgb[keep])) and np.array_equal(bits(e), bits(err[keep]))
        x2, c2, e2, kept2, v2, s2 = call(dens, xyz, counts, P, wh, plane, tol, m, False, device=device)    # without the count outputs
        assert v2 is None and s2 is None and c2 is None and e2 is None
        assert np.array_equal(bits(x2), bits(xyz[keep])) and np.array_equal(kept2, kept)
    assert np.array_equal(bits(xyz), bits(before))
    return viol, supp


CLOUDS = [(2, 900, 1), (3, 4000, 2), (7, 3000, 3), (17, 2500, 4), (40, 4000, 5)]
PLANES = [(1, 1), (8, 6), (96, 62)]


@pytest.mark.parametrize("n_refs,n,seed", CLOUDS)
@pytest.mark.parametrize("plane", PLANES)
def test_ring_clouds_equal_the_reference(twin, n_refs, n, seed, plane):
    xyz, counts, P, wh = fs.ring_cloud(n_refs, n, seed)
    seen = [check_against_reference(twin, xyz, counts, P, wh, plane, tol) for tol in (0.02, 0.2)]
    if plane != (1, 1) and n_refs > 2:
        assert seen[0][0].max() >= 2 and seen[0][1].max() >= 2             # the cloud exercises both verdicts


def test_the_minimum_of_a_cell_wins(twin):
    """several points of one reference in one cell: the nearest one is the z-buffer; the farther ones neither support nor stop a refutation"""
    cams = synthetic.ring_cameras(4)
    P, wh = fr.cameras(cams)
    c1 = np.asarray(cams[1].C, np.float64).reshape(3)
    ray = -c1 / np.linalg.norm(c1)                                         # reference 1 looks at the origin
    own = np.stack([c1 + ray * t for t in (3.0, 3.5, 4.2, 5.0)])           # four depths on one ray of reference 1
    probe = np.stack([c1 + ray * t for t in (2.0, 2.99, 3.0, 3.05, 3.5, 4.2, 6.0)])
    xyz = np.concatenate([probe, own]).astype(np.float32)
    counts = np.array([len(probe), len(own), 0, 0], np.int64)
    Z = fr.zbuffers(xyz, counts, P, wh, 96, 62)
    assert np.isfinite(Z[1]).sum() == 1 and abs(float(Z[1][np.isfinite(Z[1])][0]) - 3.0) < 1e-3
    viol, supp = check_against_reference(twin, xyz, counts, P, wh, (96, 62), 0.02, (1,))
    assert viol[:7].tolist() == [1, 0, 0, 0, 0, 0, 0] and supp[:7].tolist() == [0, 1, 1, 1, 0, 0, 0]


def test_frustum_borders_and_points_behind_a_camera(twin):
    cams = synthetic.ring_cameras(5)
    P, wh = fr.cameras(cams)
    cam = cams[2]
    Kinv, R, C = np.linalg.inv(cam.K), np.asarray(cam.R, np.float64), np.asarray(cam.C, np.float64).reshape(3)
    w, h = cam.width, cam.height

    def at(u, v, depth):
        return C + R.T @ (Kinv @ np.array([u, v, 1.0])) * depth
    us = [0.0, 1e-4, -1e-4, w - 1e-3, w - 1e-7, float(w), w + 1e-3, w / 2.0]
    vs = [0.0, 1e-4, -1e-4, h - 1e-3, h - 1e-7, float(h), h + 1e-3, h / 2.0]
    pts = [at(u, v, dep) for u in us for v in vs for dep in (2.0, 4.0)]
    pts += [at(w / 2.0, h / 2.0, -3.0), at(10.0, 10.0, -0.5), C.copy(), at(w / 2.0, h / 2.0, 1e-30)]       # behind the camera, at its centre
    rng = np.random.default_rng(3)
    ground = np.column_stack([rng.uniform(-2.0, 2.0, (600, 2)), np.zeros(600)])
    xyz = np.concatenate([np.asarray(pts), ground]).astype(np.float32)
    counts = np.array([len(pts), 0, 600, 0, 0], np.int64)
    ok, cx, cy, d = fr.project(P[2], w, h, 96, 62, xyz[:len(pts)])
    assert ok.any() and (~ok).any() and cx[ok].min() == 0 and cx[ok].max() == 95 and cy[ok].min() == 0 and cy[ok].max() == 61
    for plane in ((8, 6), (96, 62)):
        check_against_reference(twin, xyz, counts, P, wh, plane, 0.02)
    # a cloud entirely outside every frustum: nothing is written into a z-buffer, everything is kept
    out = np.array([[0.0, 0.0, 50.0], [0.0, 0.0, -50.0], [300.0, 0.0, 0.0], [0.0, 0.0, 2.5]], np.float32)
    assert not any(fr.project(P[j], wh[j, 0], wh[j, 1], 8, 6, out)[0].any() for j in range(5))
    viol, supp = check_against_reference(twin, out, np.array([1, 1, 1, 1, 0], np.int64), P, wh, (8, 6), 0.02)
    assert not viol.any() and not supp.any()


def test_non_finite_points_are_kept_and_decide_nothing(twin):
    xyz, counts, P, wh = fs.ring_cloud(6, 1500, 9)
    plain = fr.counts_of(xyz, counts, P, wh, 96, 62, 0.02)
    bad = np.array([[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, -np.inf], [np.nan, np.nan, np.nan], [0.0, 0.0, 1e30], [0.0, 0.0, -1e30],
                    [np.inf, -np.inf, 0.1], [0.1, 0.1, np.nan]], np.float32)
    offs = np.concatenate([[0], np.cumsum(counts)])
    parts, is_bad = [], []
    for r in range(6):                                                     # the bad points at the front of one reference, the end of the next ...
        own = xyz[offs[r]:offs[r + 1]]
        parts += [bad, own] if r % 2 == 0 else [own, bad]
        is_bad += [np.ones(8, bool), np.zeros(len(own), bool)] if r % 2 == 0 else [np.zeros(len(own), bool), np.ones(8, bool)]
    both, is_bad = np.concatenate(parts), np.concatenate(is_bad)
    viol, supp = check_against_reference(twin, both, counts + 8, P, wh, (96, 62), 0.02)
    assert not viol[is_bad].any() and not supp[is_bad].any()               # kept: v = 0
    assert np.array_equal(viol[~is_bad], plain[0]) and np.array_equal(supp[~is_bad], plain[1])     # and the rest does not notice them
    # non-finite points only
    viol, supp = check_against_reference(twin, bad, np.array([3, 0, 5], np.int64), P[:3], wh[:3], (8, 6), 0.2)
    assert not viol.any() and not supp.any()


def test_a_point_copied_into_a_second_reference_is_supported_by_it(twin):
    xyz, counts, P, wh = fs.ring_cloud(5, 1200, 12, floaters=0.0)
    offs = np.concatenate([[0], np.cumsum(counts)])
    inside3 = fr.project(P[3], wh[3, 0], wh[3, 1], 96, 62, xyz[:counts[0]])[0]
    i = int(np.flatnonzero(inside3)[0])
    lifted = xyz[i].copy()
    lifted[2] = 0.7                                                         # a floater of reference 0 ...
    a = np.concatenate([lifted[None], xyz])
    ca = counts.copy()
    ca[0] += 1
    v0, s0 = check_against_reference(twin, a, ca, P, wh, (96, 62), 0.02, (1,))
    b = np.concatenate([a[:offs[4] + 1], lifted[None], a[offs[4] + 1:]])      # ... and the same point again, in front of reference 4's own
    cb = ca.copy()
    cb[4] += 1
    v1, s1 = check_against_reference(twin, b, cb, P, wh, (96, 62), 0.02, (1,))
    assert s1[0] == s0[0] + 1 and v1[0] <= v0[0] and v0[0] >= 1


@pytest.mark.parametrize("empty", [(0,), (2, 3), (5,), (0, 1, 4, 5)])
def test_empty_references(twin, empty):
    xyz, counts, P, wh = fs.ring_cloud(6, 1000, 21, empty=empty)
    assert all(counts[g] == 0 for g in empty)
    check_against_reference(twin, xyz, counts, P, wh, (8, 6), 0.02)
    check_against_reference(twin, xyz, counts, P, wh, (96, 62), 0.2)


def test_one_reference_keeps_everything_and_tiny_clouds(twin):
    xyz, _counts, P, wh = fs.ring_cloud(3, 500, 30)
    viol, supp = check_against_reference(twin, xyz, np.array([500], np.int64), P[:1], wh[:1], (96, 62), 0.02)
    assert not viol.any() and not supp.any()
    check_against_reference(twin, xyz[:1], np.array([0, 1, 0], np.int64), P, wh, (8, 6), 0.02)
    x, c, e, kept, v, s = call(twin, np.zeros((0, 3), np.float32), np.array([0, 0, 0], np.int64), P, wh, (8, 6), 0.02, 1, True,
                               np.zeros((0, 3), np.float32), np.zeros((0,), np.float32))
    assert x.shape == (0, 3) and c.shape == (0, 3) and e.shape == (0,) and kept.tolist() == [0, 0, 0] and v.shape == (0,) and s.shape == (0,)


def saturating_cloud(n_refs=300):
    """10 points per reference: reference 0 owns one floater above the origin; every reference saw a patch of ground behind it"""
    cams = synthetic.ring_cameras(n_refs)
    P, wh = fr.cameras(cams)
    g = np.array([[x, y, 0.0] for x in (-0.05, 0.0, 0.05) for y in (-0.05, 0.0, 0.05)])
    more = np.array([[0.02, 0.03, 0.0]])
    parts = [np.concatenate([[[0.0, 0.0, 0.5]], g])] + [np.concatenate([g, more]) + 1e-4 * r for r in range(1, n_refs)]
    counts = np.full(n_refs, 10, np.int64)
    return np.concatenate(parts).astype(np.float32), counts, P, wh


def test_more_than_255_refuting_references_saturate_the_counts_and_still_drop(twin):
    xyz, counts, P, wh = saturating_cloud()
    viol, supp = check_against_reference(twin, xyz, counts, P, wh, (8, 6), 0.02, (1, 255))
    assert viol[0] == 299 and supp[0] == 0 and supp[1:].max() > 255
    x, _c, _e, kept, v, s = call(twin, xyz, counts, P, wh, (8, 6), 0.02, 255)
    assert v[0] == 255 and kept[0] == 9 and x.shape[0] == xyz.shape[0] - 1


def test_the_kept_set_shrinks_as_min_violations_falls(twin):
    xyz, counts, P, wh = fs.ring_cloud(12, 3000, 41)
    prev = None
    for m in (12, 8, 5, 3, 2, 1):
        x, _c, _e, _k, v, s = call(twin, xyz, counts, P, wh, (96, 62), 0.02, m)
        keep = fr.keep_mask(v.astype(np.int64), s.astype(np.int64), m)
        assert np.array_equal(bits(x), bits(xyz[keep]))
        if prev is not None:
            assert not (keep & ~prev).any()
        prev = keep
    assert 0 < prev.sum() < len(prev)


def test_permuting_references_with_their_cameras_permutes_the_result(twin):
    xyz, counts, P, wh = fs.ring_cloud(9, 2500, 43, empty=(4,))
    offs = np.concatenate([[0], np.cumsum(counts)])
    perm = np.random.default_rng(5).permutation(9)
    index = np.concatenate([np.arange(offs[g], offs[g + 1]) for g in perm])
    _x, _c, _e, kept, v, s = call(twin, xyz, counts, P, wh, (96, 62), 0.02, 2)
    _x, _c, _e, kept_p, v_p, s_p = call(twin, xyz[index], counts[perm], P[perm], wh[perm], (96, 62), 0.02, 2)
    assert np.array_equal(v_p, v[index]) and np.array_equal(s_p, s[index]) and np.array_equal(kept_p, kept[perm])


def _ground_windows(xyz, counts, P, wh, floater, pw, ph):
    """per reference j: (other, d, wmin) - the points of OTHER references inside j, their f64 depth there and the smallest depth of the 3 x 3
    window of j's z-buffer of the ground alone (+inf where the window is empty)"""
    ids = fr.ref_ids(counts)
    Z = fr.zbuffers(xyz[~floater], counts - np.bincount(ids[floater], minlength=8), P, wh, pw, ph).astype(np.float64)
    out = []
    for j in range(8):
        ok, cx, cy, d = fr.project(P[j], wh[j, 0], wh[j, 1], pw, ph, xyz)
        Zp = np.full((ph + 2, pw + 2), np.inf)
        Zp[1:-1, 1:-1] = Z[j]
        wmin = np.stack([Zp[cy + dy, cx + dx] for dy in (0, 1, 2) for dx in (0, 1, 2)]).min(axis=0)
        out.append((ok & (ids != j), d.astype(np.float64), wmin))
    return out


@pytest.mark.parametrize("plane", [(96, 62), (192, 124)])
def test_prototype_scene_floaters_stand_clear_of_the_ground(plane):
    """The scene's first precondition, in f64: every floater is inside at least 3 other references whose window there holds only ground depths
    above 1.1 x its depth.  On the 96 x 62 plane the margin is thin by geometry - the ground behind the lone patch is 1.14 x as deep as the
    patch, and the window reaches up to two cells (2.6 % of the depth each) towards the camera - which is why tests/freespace_scene.py keeps
    the patches small and says where they sit; exactly 3 references pass for some floaters there, all 7 on 192 x 124."""
    xyz, counts, P, wh, floater, _paired = fs.prototype_scene()
    clear = np.zeros(len(xyz), np.int64)
    for other, d, wmin in _ground_windows(xyz, counts, P, wh, floater, *plane):
        clear += other & floater & np.isfinite(wmin) & (wmin > 1.1 * d)
    print("references with every window depth above 1.1 x the floater's, minimum over the floaters:", int(clear[floater].min()))
    assert (clear[floater] >= 3).all()


@pytest.mark.parametrize("plane", [(96, 62), (192, 124)])
def test_prototype_scene_drops_every_floater_and_keeps_the_surface(twin, plane):
    tol = 0.02
    xyz, counts, P, wh, floater, paired = fs.prototype_scene()
    assert floater.sum() == 150 and (~floater).sum() == 12800 and paired.sum() == 100
    pw, ph = plane
    # precondition, f64: no surface point is in front of any other reference's window minimum by more than tol
    for other, d, wmin in _ground_windows(xyz, counts, P, wh, floater, pw, ph):
        surf = other & ~floater & np.isfinite(wmin)
        assert (d[surf] >= wmin[surf] * (1.0 - tol)).all()
    viol, supp = fr.counts_of(xyz, counts, P, wh, pw, ph, tol)
    assert viol[floater].min() >= 6 and supp[floater].max() <= 1
    assert viol[~floater].max() == 0 and supp[~floater].min() >= 6
    for m in (1, 2, 3):
        x, _c, _e, kept, v, s = call(twin, xyz, counts, P, wh, plane, tol, m)
        assert np.array_equal(v, viol.astype(np.uint8)) and np.array_equal(s, supp.astype(np.uint8))
        assert np.array_equal(bits(x), bits(xyz[~floater])) and kept.tolist() == [1600] * 8
    # the consensus filter at min_refs = 1 keeps the paired patch by construction: the two references vouch for each other (their patches are
    # the same points, so any radius makes them agree)
    sel = floater | (np.arange(len(xyz)) % 16 == 0)
    c = cr.consensus(xyz[sel], np.bincount(fr.ref_ids(counts)[sel], minlength=8), 0.01)
    assert (c[paired[sel]] >= 1).all()
