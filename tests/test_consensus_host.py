"""CPU tier of the cross-reference consensus filter (lfd_consensus_filter_host): the twin - keys, sort, the 27-cell scan through
csrc/lfd_consensus.hpp - against the brute-force NumPy reference of tests/consensus_ref.py, which knows no grid.  Every comparison is exact: the
counts, the kept set, the offsets and the bits of every copied value."""
import functools

import numpy as np
import pytest
import torch

import consensus_ref as cr
from lichtfeld_densification_plugin_amd.core import hip_backend as hb


@pytest.fixture(scope="module")
def twin():
    t = hb.HostDensifier(4)
    yield t
    t.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def split(n, n_refs, rng, empty=()):
    """points per reference: a random composition of n, the references in `empty` with none"""
    ids = rng.integers(0, n_refs, n)
    live = [g for g in range(n_refs) if g not in empty]
    ids = np.asarray(live)[ids % len(live)]
    return np.bincount(ids, minlength=n_refs).astype(np.int64)


def cloud(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    centres = rng.uniform(-3.0, 3.0, (9, 3))
    return (centres[rng.integers(0, 9, n)] + rng.normal(0.0, 0.03, (n, 3))).astype(np.float32)


def call(twin, xyz, counts, radius, min_refs, with_consensus=True, rgb=None, err=None):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)) if a is not None else None      # noqa: E731
    x, c, e, kept, cons = twin.consensus_filter(t(xyz), t(rgb), t(err), counts, radius, min_refs, with_consensus)
    return (x.numpy(), c.numpy() if c is not None else None, e.numpy() if e is not None else None, np.asarray(kept),
            cons.numpy() if cons is not None else None)


def check_against_reference(twin, xyz, counts, radius, min_refs_list=(1, 3, 8), want_c=None):
    xyz = np.ascontiguousarray(xyz, np.float32)
    n = xyz.shape[0]
    rng = np.random.default_rng(n + 17)
    rgb = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
    err = rng.uniform(0.0, 2.0, (n,)).astype(np.float32)
    if n > 2:
        rgb[1, 1], err[2] = np.nan, np.inf                                 # whatever travels along is copied, not looked at
    c_ref = cr.consensus(xyz, counts, radius) if want_c is None else np.asarray(want_c, np.uint8)
    ids = cr.ref_ids(counts)
    for m in min_refs_list:
        keep = c_ref >= m
        x, c, e, kept, cons = call(twin, xyz, counts, radius, m, True, rgb, err)
        assert np.array_equal(cons, c_ref), (m, np.flatnonzero(cons != c_ref)[:10])
        assert np.array_equal(kept, np.bincount(ids[keep], minlength=len(counts)))
        assert np.array_equal(bits(x), bits(xyz[keep])) and np.array_equal(bits(c), bits(rgb[keep])) and np.array_equal(bits(e), bits(err[keep]))
        # without the counts the scan stops at min_refs: the same kept set, nothing else copied
        x2, c2, e2, kept2, cons2 = call(twin, xyz, counts, radius, m, False)
        assert cons2 is None and c2 is None and e2 is None
        assert np.array_equal(bits(x2), bits(xyz[keep])) and np.array_equal(kept2, kept)
    return c_ref


CLOUDS = [("uniform", 4000, 2, 1), ("uniform", 3000, 7, 2), ("uniform", 1500, 40, 3), ("clustered", 4000, 5, 4), ("clustered", 2500, 23, 5)]


@pytest.mark.parametrize("kind,n,n_refs,seed", CLOUDS)
def test_seeded_clouds_equal_the_brute_force_reference(twin, kind, n, n_refs, seed):
    xyz = cloud(kind, n, seed)
    counts = split(n, n_refs, np.random.default_rng(seed))
    seen = []
    for radius in (1e-4, 0.02, 0.08, 0.5, 20.0):                          # from "nobody agrees" to "everyone agrees"
        c = check_against_reference(twin, xyz, counts, radius, min_refs_list=(1, 2, 3, 4, 5, 6, 7, 8))
        seen.append(c)
    assert seen[0].max() == 0
    assert np.array_equal(seen[-1], np.full(n, min(cr.CAP, int((counts > 0).sum()) - 1), np.uint8))
    for a, b in zip(seen, seen[1:]):                                       # a larger radius never lowers a count
        assert (b >= a).all()


def test_monotone_in_min_refs_and_symmetric(twin):
    xyz = cloud("clustered", 3000, 11)
    counts = split(3000, 12, np.random.default_rng(11))
    ids = cr.ref_ids(counts)
    radius = 0.05
    prev = None
    for m in range(1, 9):
        x, _c, _e, _k, cons = call(twin, xyz, counts, radius, m)
        kept = cons >= m
        assert np.array_equal(bits(x), bits(xyz[kept]))
        if prev is not None:
            assert not (kept & ~prev).any()                                # the kept set at m + 1 is a subset of the set at m
        prev = kept
    # symmetry: the test is symmetric bit for bit, so whenever i vouches for j (adds ref(i) to j's count), j vouches for i
    ok = cr.agree_matrix(xyz, radius)
    assert np.array_equal(ok, ok.T)
    onehot = np.zeros((3000, 12), bool)
    onehot[np.arange(3000), ids] = True
    vouch = (ok.astype(np.float32) @ onehot.astype(np.float32)) > 0        # vouch[i, g]: reference g owns a point agreeing with i
    i, j = np.nonzero(ok & (ids[:, None] != ids[None, :]))
    assert i.size > 1000 and vouch[i, ids[j]].all() and vouch[j, ids[i]].all()
    counted = vouch.copy()
    counted[np.arange(3000), ids] = False
    assert np.array_equal(np.minimum(counted.sum(1), cr.CAP), call(twin, xyz, counts, radius, 1)[4])


def test_the_lattice_threshold_is_kept_at_equality(twin):
    xyz = np.array([[0, 0, 0], [3, 4, 0]], np.float32)
    for radius, c in ((5.0, 1), (np.nextafter(np.float32(5.0), np.float32(0.0)), 0)):
        x, _c, _e, kept, cons = call(twin, xyz, [1, 1], float(radius), 1)
        assert cons.tolist() == [c, c] and kept.tolist() == [c, c] and x.shape[0] == 2 * c
    assert call(twin, xyz, [2], 5.0, 1)[4].tolist() == [0, 0]              # the same two points of ONE reference vouch for nobody


def test_points_on_cell_faces_at_the_minimum_and_negative_coordinates(twin):
    for radius in (0.25, 1.0, 0.1):
        h = 1.000001 * radius
        k = np.arange(-3, 4)
        g = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3)
        for origin in (np.zeros(3), np.array([-7.5, 2.25, -0.125])):      # the first point is the minimum: every point sits on a cell face
            xyz = (origin + g * h).astype(np.float32)
            xyz = np.concatenate([xyz, xyz + np.float32(radius) * np.array([0.5, -0.25, 0.75], np.float32)]).astype(np.float32)
            rng = np.random.default_rng(3)
            perm = rng.permutation(xyz.shape[0])
            check_against_reference(twin, xyz[perm], split(xyz.shape[0], 6, rng), radius, (1, 2))
            check_against_reference(twin, xyz[perm], split(xyz.shape[0], 6, rng), float(np.float32(h)), (1, 4))


def test_all_points_in_one_cell(twin):
    rng = np.random.default_rng(8)
    xyz = rng.uniform(0.0, 0.01, (1200, 3)).astype(np.float32)
    c = check_against_reference(twin, xyz, split(1200, 5, rng), 10.0)
    assert (c == 4).all()
    c = check_against_reference(twin, xyz, split(1200, 5, rng), 0.0015)   # ... and a radius at which only some agree
    assert 0 < int((c > 0).sum()) and c.min() < c.max()


def test_two_points_in_cells_one_apart_along_every_axis_and_diagonal(twin):
    radius = 1.0
    n = 0
    for d in np.stack(np.meshgrid([-1, 0, 1], [-1, 0, 1], [-1, 0, 1], indexing="ij"), -1).reshape(-1, 3):
        if not d.any():
            continue
        # a at the far corner of its cell from b's side, b just across the face(s): different cells, distance well inside the radius
        base = np.array([10.3, -4.2, 0.9])
        a = base
        b = base + d * 0.55 / np.linalg.norm(d) * radius
        anchor = base - 3.0                                                # fixes the grid's origin; far from both
        for off in np.linspace(0.0, 1.0, 7):                               # slide the pair through the cells: it straddles a face for some offsets
            xyz = np.array([anchor, a + off * d, b + off * d], np.float32)
            x, _c, _e, kept, cons = call(twin, xyz, [1, 1, 1], radius, 1)
            assert cons.tolist() == cr.consensus(xyz, [1, 1, 1], radius).tolist() == [0, 1, 1], (d, off)
            n += 1
    assert n == 26 * 7


def test_one_reference_only_drops_everything(twin):
    xyz = cloud("clustered", 500, 2)
    x, _c, _e, kept, cons = call(twin, xyz, [500], 10.0, 1)
    assert x.shape[0] == 0 and kept.tolist() == [0] and not cons.any()


def test_empty_references_at_the_start_in_the_middle_and_at_the_end(twin):
    rng = np.random.default_rng(5)
    xyz = cloud("clustered", 900, 6)
    counts = split(900, 9, rng, empty=(0, 1, 4, 8))
    assert counts[[0, 1, 4, 8]].tolist() == [0, 0, 0, 0]
    check_against_reference(twin, xyz, counts, 0.06)
    dense = counts[counts > 0]
    a, b = call(twin, xyz, counts, 0.06, 2), call(twin, xyz, dense, 0.06, 2)
    assert np.array_equal(a[4], b[4]) and np.array_equal(a[3][counts > 0], b[3]) and not a[3][counts == 0].any()


def test_no_points_and_one_point(twin):
    x, c, e, kept, cons = call(twin, np.zeros((0, 3), np.float32), [0, 0, 0], 1.0, 1, True, np.zeros((0, 3), np.float32), np.zeros((0,), np.float32))
    assert x.shape == (0, 3) and c.shape == (0, 3) and e.shape == (0,) and kept.tolist() == [0, 0, 0] and cons.shape == (0,)
    x, _c, _e, kept, cons = call(twin, np.ones((1, 3), np.float32), [0, 1], 1.0, 1)
    assert x.shape[0] == 0 and kept.tolist() == [0, 0] and cons.tolist() == [0]


def test_duplicates_in_nine_references_reach_the_cap(twin):
    xyz = np.tile(np.array([[1.5, -2.0, 0.25]], np.float32), (9, 1))
    x, _c, _e, kept, cons = call(twin, xyz, [1] * 9, 1e-3, 8)
    assert cons.tolist() == [8] * 9 and kept.tolist() == [1] * 9
    xyz = np.tile(np.array([[1.5, -2.0, 0.25]], np.float32), (24, 1))      # twelve references, two copies each: eleven others, counted as 8
    assert call(twin, xyz, [2] * 12, 1e-3, 8)[4].tolist() == [8] * 24


def test_non_finite_points_are_dropped_vouch_for_nobody_and_change_nothing(twin):
    rng = np.random.default_rng(9)
    xyz = cloud("clustered", 1200, 9)
    counts = split(1200, 6, rng)
    clean = call(twin, xyz, counts, 0.06, 1)[4]
    bad = rng.choice(1200, 60, replace=False)
    dirty = xyz.copy()
    dirty[bad[:20], 0] = np.nan
    dirty[bad[20:40], 2] = np.inf
    dirty[bad[40:], 1] = -np.inf
    with np.errstate(all="ignore"):
        c = check_against_reference(twin, dirty, counts, 0.06, (1, 2))
    assert not c[bad].any()
    # against the same cloud with those points REMOVED: the others count exactly what they count without them
    mask = np.ones(1200, bool)
    mask[bad] = False
    ids = cr.ref_ids(counts)
    removed = call(twin, xyz[mask], np.bincount(ids[mask], minlength=6), 0.06, 1)[4]
    assert np.array_equal(c[mask], removed) and (clean >= c).all()
    allbad = np.full((5, 3), np.nan, np.float32)
    x, _c, _e, kept, cons = call(twin, allbad, [2, 3], 1.0, 1)
    assert x.shape[0] == 0 and kept.tolist() == [0, 0] and cons.tolist() == [0] * 5


def test_permuting_whole_references_permutes_the_result(twin):
    rng = np.random.default_rng(12)
    xyz = cloud("clustered", 1500, 12)
    counts = split(1500, 7, rng)
    offs = np.concatenate([[0], np.cumsum(counts)])
    order = rng.permutation(7)
    idx = np.concatenate([np.arange(offs[g], offs[g + 1]) for g in order])
    a = call(twin, xyz, counts, 0.05, 2)
    b = call(twin, xyz[idx], counts[order], 0.05, 2)
    assert np.array_equal(b[4], a[4][idx]) and np.array_equal(b[3], a[3][order])
    assert np.array_equal(bits(b[0]), bits(xyz[idx][a[4][idx] >= 2]))


@functools.lru_cache(maxsize=None)
def floater_scene():
    """A wavy surface sampled by 6 references with noise, plus 5 floater clusters of 50 points, each cluster from ONE reference."""
    rng = np.random.default_rng(21)
    radius = 0.08
    parts, counts = [], []
    floaters = []
    axis = np.arange(25) * 0.025 - 0.3
    for g in range(6):
        # every reference samples the surface on its own jittered grid of spacing 0.025: another reference's sample is never farther than 0.03
        uv = np.stack(np.meshgrid(axis, axis, indexing="ij"), -1).reshape(-1, 2) + rng.uniform(-0.005, 0.005, (625, 2)) + 0.004 * g
        z = 0.05 * np.sin(2.0 * uv[:, 0]) * np.cos(1.5 * uv[:, 1])
        surf = np.column_stack([uv, z]) + rng.normal(0.0, 0.002, (625, 3))
        pts = [surf]
        flags = [np.zeros(625, bool)]
        if g < 5:
            centre = np.array([-0.8 + 0.4 * g, 0.6 - 0.3 * g, 0.9 + 0.1 * g])
            pts.append(centre + rng.normal(0.0, 0.008, (50, 3)))
            flags.append(np.ones(50, bool))
        parts.append(np.concatenate(pts))
        floaters.append(np.concatenate(flags))
        counts.append(parts[-1].shape[0])
    return np.concatenate(parts).astype(np.float32), np.asarray(counts, np.int64), np.concatenate(floaters), radius


def test_it_drops_what_a_radius_filter_keeps_floaters_of_one_reference(twin):
    xyz, counts, floater, radius = floater_scene()
    ids = cr.ref_ids(counts)
    p = xyz.astype(np.float64)
    d = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(-1))
    other = ids[:, None] != ids[None, :]
    # f64 premises: a floater is far from every point of another reference and has company of its own - a plain radius filter keeps it
    assert (np.where(other, d, np.inf)[floater].min(axis=1) > 2.0 * radius).all()
    assert (((d <= radius) & ~other).sum(axis=1)[floater] - 1 >= 10).all()
    # ... and every surface point has at least 3 other references well inside the radius
    near = (d <= radius / 2.0) & other
    onehot = np.zeros((ids.size, 6))
    onehot[np.arange(ids.size), ids] = 1.0
    assert (((near.astype(np.float64) @ onehot) > 0).sum(axis=1)[~floater] >= 3).all()
    for m in (1, 3):
        x, _c, _e, kept, cons = call(twin, xyz, counts, radius, m)
        assert not (cons[floater] >= m).any() and (cons[~floater] >= m).all()
        assert np.array_equal(bits(x), bits(xyz[~floater])) and kept.tolist() == [625] * 6
