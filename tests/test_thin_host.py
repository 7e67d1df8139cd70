"""CPU tier of the footprint-adaptive thinning (lfd_thin_footprint_host): the twin against the brute-force reference of
tests/thin_ref.py - index list, kept counts per reference and per-level statistics, element for element - on the edge cases of the rule, the level
boundary pinned to the bit, the two properties that bound the distance inside a cell, and what the stage is for: on a scene with a near and a far
field every reference keeps a similar share of its own image covered, where a world-uniform voxel of the same output size does not."""
import numpy as np
import pytest
import torch

import thin_ref as tr
import thin_scene as ts
from lichtfeld_densification_plugin_amd.core import hip_backend as hb


@pytest.fixture(scope="module")
def twin():
    dens = hb.HostDensifier(3)
    yield dens
    dens.close()


def run(dens, xyz, err, counts, rows, thin_cells):
    keep, kept = dens.thin_footprint(torch.from_numpy(np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)),
                                     None if err is None else torch.from_numpy(np.ascontiguousarray(err, np.float32)), counts, rows, thin_cells)
    return keep.numpy(), kept, dens.thin_stats


def same(twin, xyz, err, counts, rows, thin_cells):
    """twin == reference: the index list, the kept counts and the statistics"""
    keep, kept, stats = run(twin, xyz, err, counts, rows, thin_cells)
    want, want_kept, want_stats = tr.thin_ref(xyz, err, counts, rows, thin_cells)
    assert keep.dtype == np.int64 and keep.tolist() == want.tolist()
    assert kept.dtype == np.int64 and kept.tolist() == want_kept.tolist() and int(kept.sum()) == keep.size
    assert stats[0].tolist() == want_stats[0].tolist() and stats[1].tolist() == want_stats[1].tolist()
    assert isinstance(stats[2], float) and stats[2] == want_stats[2]
    assert int(stats[0].sum()) == np.asarray(xyz).reshape(-1, 3).shape[0] and int(stats[1].sum()) == keep.size
    assert (np.diff(keep) > 0).all()
    return keep, kept, stats


FRONT = np.array([[0.0, 0.0, 1.0, 10.0, 0.01]])                           # depth = z + 10


def test_no_point_and_one_point(twin):
    keep, kept, stats = same(twin, np.zeros((0, 3), np.float32), None, [0], FRONT, 2.0)
    assert keep.size == 0 and kept.tolist() == [0] and stats[2] == 0.0
    keep, kept, stats = same(twin, np.array([[1.0, 2.0, 3.0]], np.float32), np.array([0.5], np.float32), [1], FRONT, 2.0)
    assert keep.tolist() == [0] and stats[0][20] == 1 and stats[2] == 0.0            # no extent: level 20


def test_identical_points_keep_the_one_of_smallest_error(twin):
    xyz = np.repeat(np.array([[0.3, -0.7, 1.1]], np.float32), 50, axis=0)
    err = np.random.default_rng(2).uniform(0, 1, 50).astype(np.float32)
    keep, _, stats = same(twin, xyz, err, [20, 30], np.repeat(FRONT, 2, axis=0), 2.0)
    assert keep.tolist() == [int(np.argmin(err))] and stats[0][20] == 50 and stats[1][20] == 1
    keep, _, _ = same(twin, xyz, None, [20, 30], np.repeat(FRONT, 2, axis=0), 2.0)
    assert keep.tolist() == [0]


@pytest.mark.parametrize("with_err", [True, False])
def test_random_points_over_three_references(twin, with_err):
    counts = [700, 900, 400]
    xyz, err, rows = tr.random_case(2000, counts, 1, dupes=30)
    keep, kept, stats = same(twin, xyz, err if with_err else None, counts, rows, 2.0)
    assert 0 < keep.size < 2000 and np.count_nonzero(stats[0]) >= 2      # the stage acts, over more than one level
    assert np.count_nonzero(keep < 30) == 1                               # the duplicates share a cell


def test_error_ties_negative_zero_and_nan(twin):
    xyz = np.repeat(np.array([[0.0, 0.0, 0.0], [4.0, 4.0, 4.0]], np.float32), 6, axis=0)      # two cells of six points at any level >= 1
    rows = FRONT.copy()
    nan_neg = np.array([0xffc00000], np.uint32).view(np.float32)[0]       # a NaN with the sign bit: below every number in the rank's order
    err = np.array([0.5, 0.25, 0.25, 1.0, np.nan, 0.75,    0.0, -0.0, 3.0, nan_neg, -1.0, np.nan], np.float32)
    keep, _, _ = same(twin, xyz, err, [12], rows, 2.0)
    assert keep.tolist() == [1, 9]                                        # the first of the tie; the negative NaN's bits rank lowest
    err[9] = 2.0
    keep, _, _ = same(twin, xyz, err, [12], rows, 2.0)
    assert keep.tolist() == [1, 10]                                       # -1 < -0 < +0
    err[10] = 2.0
    keep, _, _ = same(twin, xyz, err, [12], rows, 2.0)
    assert keep.tolist() == [1, 7]


def test_empty_references_in_the_middle_and_at_the_end(twin):
    counts = [300, 0, 500, 0, 0, 200, 0]
    xyz, err, rows = tr.random_case(1000, counts, 3)
    keep, kept, _ = same(twin, xyz, err, counts, rows, 3.0)
    assert kept[1] == kept[3] == kept[4] == kept[6] == 0 and keep.size < 1000
    # a point takes the camera of the reference that owns it: other rows for the empty references change nothing
    other = rows.copy()
    other[[1, 3, 4, 6]] = [[1.0, 0.0, 0.0, 100.0, 0.5]] * 4
    assert run(twin, xyz, err, counts, other, 3.0)[0].tolist() == keep.tolist()


def test_a_point_behind_its_camera_is_of_level_twenty(twin):
    xyz, err, _ = tr.random_case(400, [400], 4)
    rows = np.array([[0.0, 0.0, 1.0, 0.0, 0.01]])                         # depth = z: about half of the points lie behind the camera
    keep, _, stats = same(twin, xyz, err, [400], rows, 2.0)
    behind = xyz[:, 2] <= 0
    assert 100 < behind.sum() < 300 and stats[0][20] == behind.sum()
    assert np.isin(np.flatnonzero(behind), keep).all()                    # distinct points at the finest level: all of them stay


def test_thin_cells_so_large_that_one_point_stays_and_so_small_that_all_do(twin):
    xyz, err, _ = tr.random_case(500, [200, 300], 5)
    rows = np.array([[0.0, 0.0, 1.0, 10.0, 0.01], [0.0, 1.0, 0.0, 10.0, 0.02]])      # every depth is positive
    keep, _, stats = same(twin, xyz, err, [200, 300], rows, 1e12)
    assert stats[0][0] == 500 and stats[1][0] == 1
    best = np.flatnonzero(err == err.min())[0]
    assert keep.tolist() == [int(best)]
    keep, _, stats = same(twin, xyz, err, [200, 300], rows, 1e-12)
    assert stats[0][20] == 500 and keep.tolist() == list(range(500))


@pytest.mark.parametrize("k", [1, 3, 11, 20])
def test_the_level_boundary_to_the_bit(twin, k):
    """L = 3 and a footprint g = thin_cells (depth 1, tangent 1): q = 3 / g is exactly 2^k for g = 3 / 2^k, and the f64 just below 2^k for the f64
    just above that g.  The first is of level k, the second of level k - 1."""
    rng = np.random.default_rng(k)
    xyz = np.concatenate([[[0, 0, 0], [3, 0, 0], [1, 1, 1], [1, 1, 1]], rng.uniform(0, 3, (60, 3))]).astype(np.float32)
    rows = np.array([[0.0, 0.0, 0.0, 1.0, 1.0]])
    g = np.float64(3.0) / np.float64(2.0 ** k)
    above = np.nextafter(g, np.inf)
    assert np.float64(3.0) / g == 2.0 ** k and np.float64(3.0) / above == np.nextafter(np.float64(2.0 ** k), 0.0)
    _, _, stats = same(twin, xyz, None, [64], rows, float(g))
    assert stats[2] == 3.0 and stats[0][k] == 64
    _, _, stats = same(twin, xyz, None, [64], rows, float(above))
    assert stats[0][k - 1] == 64
    if k == 20:                                                            # beyond the clamp nothing changes
        _, _, stats = same(twin, xyz, None, [64], rows, float(g) / 4.0)
        assert stats[0][20] == 64


def test_no_two_kept_points_share_a_code_and_every_point_has_its_code_kept(twin):
    """So a point lies in the cell of a kept point, of side L / 2^level < 2 g_i (level < 20): within sqrt(3) * 2 g_i of it."""
    counts = [900, 600, 1500]
    xyz, err, rows = tr.random_case(3000, counts, 6, dupes=10)
    keep, _, _ = run(twin, xyz, err, counts, rows, 2.5)
    codes, lev, L = tr.codes_ref(xyz, counts, rows, 2.5)
    kept_codes = [codes[i] for i in keep.tolist()]
    assert len(set(kept_codes)) == len(kept_codes)
    assert set(codes) == set(kept_codes)
    by_code = {codes[i]: i for i in keep.tolist()}
    ref = np.repeat(np.arange(3), counts)
    x64 = xyz.astype(np.float64)
    depth = (x64 * rows[ref, :3]).sum(axis=1) + rows[ref, 3]
    g = depth * rows[ref, 4] * 2.5
    rep = np.array([by_code[c] for c in codes])
    dist = np.linalg.norm(x64 - x64[rep], axis=1)
    inner = (lev > 0) & (lev < 20)
    assert inner.sum() > 2000 and (dist[inner] <= np.sqrt(3.0) * 2.0 * g[inner] * (1 + 1e-6)).all()
    assert (L / 2.0 ** lev[inner] >= g[inner] * (1 - 1e-12)).all()        # and a cell is never smaller than the footprint


def test_every_reference_keeps_a_similar_share_of_its_image_where_a_uniform_voxel_does_not():
    """Twelve references at 96 x 96 cells over a ground plane at 2 - 4 units and a wall at 40 (tests/thin_scene.py), 110 592 points, thin_cells = 2
    against the uniform first-point voxel filter at the largest size (of a ladder of 120 from 0.01 to 20) that still keeps at least as many points.
    Per reference, the share of its own occupied grid cells that still hold a kept point.  Measured:
        footprint   10 324 kept   0.207 .. 0.407 over the references   best / worst  1.97
        voxel 0.406 10 455 kept   0.004 .. 0.745                       best / worst  171.6
    """
    xyz, err, counts, rows, cams = ts.build()
    dens = hb.HostDensifier(3)
    try:
        keep, kept, _ = run(dens, xyz, err, counts, rows, 2.0)
    finally:
        dens.close()
    mine = ts.retention(xyz, counts, cams, keep)
    voxel = None
    for size in np.geomspace(0.01, 20.0, 120):
        k = ts.voxel_first(xyz, size)
        if k.size >= keep.size:
            voxel = (size, k)
    size, vkeep = voxel
    theirs = ts.retention(xyz, counts, cams, vkeep)
    print(f"footprint kept {keep.size}: {mine.min():.3f} .. {mine.max():.3f} ratio {mine.max() / mine.min():.2f}")
    print(f"voxel {size:.3f} kept {vkeep.size}: {theirs.min():.3f} .. {theirs.max():.3f} ratio {theirs.max() / theirs.min():.1f}")
    assert xyz.shape[0] == 110592 and vkeep.size >= keep.size
    assert mine.min() > theirs.min()
    assert mine.max() / mine.min() < theirs.max() / theirs.min()
