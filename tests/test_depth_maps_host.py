"""CPU tier of the depth-map renderer (lfd_render_depth_host): the twin against the brute-force NumPy reference of
tests/depth_ref.py, and the effect of the visibility rule on a scene whose answer follows from its construction.  Every comparison is exact: bit
patterns for depths and normals, == for indices."""
import numpy as np
import pytest
import torch

import depth_ref as dr
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

TOL = 0.02


@pytest.fixture(scope="module", params=[1, 4], ids=["1thread", "4threads"])
def twin(request):
    t = hb.HostDensifier(request.param)
    yield t
    t.close()


@pytest.fixture(scope="module")
def twin4():
    t = hb.HostDensifier(4)
    yield t
    t.close()


def render(dens, xyz, normals, P, wh, plane, r, R, tol=TOL, with_index=True, cams_per_batch=0):
    return dens.render_depth(np.asarray(xyz, np.float32).reshape(-1, 3), normals, P, wh, plane, r, R, tol, with_index, cams_per_batch)


def check(dens, xyz, normals, P, wh, plane, r, R, tol=TOL, want=None):
    want = dr.render(xyz, normals, P, wh, plane[0], plane[1], r, R, tol) if want is None else want
    dr.assert_equal(render(dens, xyz, normals, P, wh, plane, r, R, tol), want, (plane, r, R))
    return want


SCENE = dr.random_scene(3000, 5)
_REFERENCE = {}


def reference(r, R):
    """the reference rendering of SCENE on the 37 x 23 plane, computed once per (r, R)"""
    if (r, R) not in _REFERENCE:
        xyz, normals, P, wh = SCENE
        _REFERENCE[(r, R)] = dr.render(xyz, normals, P, wh, 37, 23, r, R, TOL)
    return _REFERENCE[(r, R)]


@pytest.mark.parametrize("R", [0, 1, 8])
@pytest.mark.parametrize("r", [0, 1, 3])
def test_random_cloud_equals_the_reference(twin, r, R):
    xyz, normals, P, wh = SCENE
    want = check(twin, xyz, normals, P, wh, (37, 23), r, R, want=reference(r, R))
    assert (want[1] >= 0).any()
    if R == 8:
        assert (want[1] >= 0).sum() < (reference(r, 0)[1] >= 0).sum()   # the rule drops cells on this cloud
    assert len({tuple(x) for x in wh.tolist()}) > 1                     # a camera of another aspect ratio is among them


def test_tensors_in_tensors_out_and_optional_outputs(twin4):
    xyz, normals, P, wh = SCENE
    want = reference(1, 1)
    got = twin4.render_depth(torch.from_numpy(xyz), torch.from_numpy(normals), P, wh, (37, 23), 1, 1, TOL, True)
    assert all(torch.is_tensor(g) for g in got)
    dr.assert_equal([g.numpy() for g in got], want)
    depth, index, normal = twin4.render_depth(torch.from_numpy(xyz), None, P, wh, (37, 23), 1, 1, TOL)
    assert index is None and normal is None
    dr.assert_equal((depth.numpy(), None, None), (want[0], None, None))
    # the batch size changes nothing
    dr.assert_equal(render(twin4, xyz, normals, P, wh, (37, 23), 1, 1, cams_per_batch=2), want)


def test_points_outside_on_the_border_and_not_finite(twin4):
    w, h = 64, 40
    P = np.array([[50.0, 0, 32, 0], [0, 50.0, 20, 0], [0, 0, 1, 0]], np.float32).reshape(1, 12)
    wh = np.array([[w, h]], np.int32)

    def at(u, v, z):
        return [(u - 32.0) * z / 50.0, (v - 20.0) * z / 50.0, z]
    us = [0.0, 1e-4, -1e-4, w - 1e-3, float(w), w + 1e-3, w / 2.0]
    vs = [0.0, 1e-4, -1e-4, h - 1e-3, float(h), h + 1e-3, h / 2.0]
    pts = [at(u, v, z) for u in us for v in vs for z in (2.0, 4.0)]
    pts += [at(32.0, 20.0, -3.0), at(10.0, 10.0, -0.5), [0.0, 0.0, 0.0], at(32.0, 20.0, 1e-30)]          # behind the camera, at its centre
    pts += [[np.nan, 0, 2], [0, np.inf, 2], [0, 0, np.inf], [0, 0, -np.inf], [np.nan] * 3]
    xyz = np.asarray(pts, np.float32)
    ok, cx, cy, _ = dr.project(P[0], w, h, 16, 10, xyz)
    assert ok.any() and (~ok).any() and cx[ok].min() == 0 and cx[ok].max() == 15 and cy[ok].min() == 0 and cy[ok].max() == 9
    normals = np.arange(3 * len(xyz), dtype=np.float32).reshape(-1, 3)
    for plane in ((16, 10), (3, 2)):
        for r, R in ((0, 0), (1, 3), (3, 8)):
            check(twin4, xyz, normals, P, wh, plane, r, R)
    # a depth that overflows f32: p_2 is a finite f64 above FLT_MAX, the point is outside; one a little below the limit is inside
    Pbig = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 3.0e38, 0]], np.float32).reshape(1, 12)
    one = np.array([[4, 4]], np.int32)
    far = np.array([[0.0, 0.0, 2.0], [0.0, 0.0, 1.0]], np.float32)
    ok, _, _, d = dr.project(Pbig[0], 4, 4, 2, 2, far)
    assert ok.tolist() == [False, True] and d[1] == np.float32(3.0e38)
    depth, index, _ = check(twin4, far, None, Pbig, one, (2, 2), 0, 0)
    assert index[0, 0, 0] == 1 and depth[0, 0, 0] == np.float32(3.0e38) and (index.reshape(-1)[1:] == -1).all()


def test_equal_depth_bits_in_one_cell_the_lower_index_wins(twin4):
    P = np.array([[64.0, 0, 32, 0], [0, 64.0, 32, 0], [0, 0, 1, 0]], np.float32).reshape(1, 12)
    wh = np.array([[64, 64]], np.int32)
    xyz = np.array([[0.50, 0.50, 3.0], [0.01, 0.02, 2.0], [0.02, 0.01, 2.0], [0.015, 0.015, 2.5]], np.float32)    # the last three in cell (4, 4) of 8 x 8, the first in (5, 5)
    normals = np.arange(12, dtype=np.float32).reshape(4, 3)
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [2, 0, 3, 1]):
        depth, index, normal = check(twin4, xyz[order], normals[order], P, wh, (8, 8), 0, 0)
        first = min(order.index(1), order.index(2))                       # of the two points at depth 2, the one that comes first
        assert index[0, 4, 4] == first and depth[0, 4, 4] == np.float32(2.0)
        assert normal[0, 4, 4].tolist() == normals[order][first].tolist()
        assert (index >= 0).sum() == 2                                    # (and the point at depth 3 in its own cell)


def test_no_points_and_the_smallest_plane(twin4):
    _, _, P, wh = SCENE
    empty = np.zeros((0, 3), np.float32)
    for normals in (None, empty):
        depth, index, normal = render(twin4, empty, normals, P, wh, (5, 4), 1, 3)
        assert depth.shape == (3, 4, 5) and not depth.any() and (index == -1).all()
        assert (normal is None) == (normals is None) and (normal is None or (normal.shape == (3, 4, 5, 3) and not normal.any()))
    xyz, normals = SCENE[0], SCENE[1]
    for r, R in ((0, 0), (3, 8)):
        depth, index, _ = check(twin4, xyz, normals, P, wh, (1, 1), r, R)
        assert (index >= 0).all()                                         # one cell per camera, its nearest point: nothing can be nearer


# ---- the effect, from the construction ------------------------------------------------------------------------------------------------------------
def two_walls():
    """One pinhole camera (f = 64, c = 32, 64 x 64 pixels) on a 64 x 64 plane.  Back wall at z = 4: a point at every cell centre.  Front wall at
    z = 2: a point at every cell centre with even cx and even cy, outside the hole 24 <= cx, cy < 40.  Every coordinate is exact in f32.
    Returns (xyz, P, wh, front [64, 64] bool: the cells that hold a front point)."""
    P = np.array([[64.0, 0, 32, 0], [0, 64.0, 32, 0], [0, 0, 1, 0]], np.float32).reshape(1, 12)
    wh = np.array([[64, 64]], np.int32)
    cy, cx = np.mgrid[0:64, 0:64]
    hole = (cx >= 24) & (cx < 40) & (cy >= 24) & (cy < 40)
    front = (cx % 2 == 0) & (cy % 2 == 0) & ~hole

    def wall(mask, z):
        return np.column_stack([(cx[mask] + 0.5 - 32.0) * z / 64.0, (cy[mask] + 0.5 - 32.0) * z / 64.0, np.full(int(mask.sum()), z)])
    xyz = np.concatenate([wall(np.ones_like(front), 4.0), wall(front, 2.0)]).astype(np.float32)
    return xyz, P, wh, front, hole


def within(mask, dist):
    """cells within Chebyshev distance ``dist`` of a cell of ``mask`` (the plane's border cuts the window)"""
    out = np.zeros_like(mask)
    for y, x in np.argwhere(mask):
        out[max(0, y - dist):y + dist + 1, max(0, x - dist):x + dist + 1] = True
    return out


@pytest.mark.parametrize("r,R,n_front,n_back,n_empty", [(0, 0, 960, 3136, 0), (0, 2, 960, 169, 2967), (1, 2, 3871, 121, 104)])
def test_the_back_wall_does_not_leak_through_the_front_wall(twin4, r, R, n_front, n_back, n_empty):
    xyz, P, wh, front, hole = two_walls()
    assert xyz.shape[0] == 5056
    # by the rule: a cell shows the front wall when a front point lies within r; else it holds the back wall, which is kept iff no cell within R
    # shows the front wall (4 > 2 + 0.02 * 2) - that is, no front point within R + r.  R = 0 tests nothing.
    shows_front = within(front, r)
    keeps_back = ~shows_front & (~within(shows_front, R) if R > 0 else True)
    assert np.array_equal(within(shows_front, R), within(front, R + r))    # the second identity, on this scene
    depth, index, _ = render(twin4, xyz, None, P, wh, (64, 64), r, R)
    depth, index = depth[0], index[0]
    assert np.array_equal(depth == np.float32(2.0), shows_front) and np.array_equal(depth == np.float32(4.0), keeps_back)
    assert np.array_equal(depth == 0, ~shows_front & ~keeps_back) and np.array_equal(index == -1, depth == 0)
    assert ((depth == 2).sum(), (depth == 4).sum(), (depth == 0).sum()) == (n_front, n_back, n_empty)
    leaks = (depth == 4) & ~hole
    assert leaks.sum() == (2880 if R == 0 else 0)                          # without the test the back wall shows through 2 880 gaps
    assert (index[depth == 4] < 4096).all() and (index[depth == 2] >= 4096).all()
    dr.assert_equal((depth[None], index[None], None), dr.render(xyz, None, P, wh, 64, 64, r, R, TOL)[:2] + (None,))
