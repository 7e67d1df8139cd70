"""The depth-map renderer on the device (lfd_render_depth through HipDensifier.render_depth) against the CPU twin - both sides are given the SAME
cloud and cameras - at the smallest sizes that take every path: one lane, one workgroup and a ragged second one, many workgroups; a plane of one
cell, of one tile, of partial tiles and of several tiles with partial ones on both edges; no splat and no window, the widest of both (a halo of
11 cells, wider than the small planes), the defaults; one camera, five in one batch and in batches of two with a tail of one; every point of a
large cloud in one cell; with and without normals and indices; one context reused at other sizes and between calls of another stage.  Depths and
normals equal the twin's bit for bit, indices by value: the twin walks the definition, the device the two min-filter identities."""
import numpy as np
import pytest
import torch

import depth_ref as dr
import freespace_scene as fs
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from test_gpu_freespace import both as freespace_both

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TOL = 0.02
MODES = [(0, 0), (3, 8), (1, 3)]


@pytest.fixture(scope="module")
def dens():
    d = hb.HipDensifier(DEV)
    yield d
    d.close()


@pytest.fixture(scope="module")
def twin():
    d = hb.HostDensifier(16)
    yield d
    d.close()


def both(dens, twin, xyz, normals, P, wh, plane, r, R, with_index=True, cams_per_batch=0, tensors=False):
    """one call on each side over the same cloud; returns the device's outputs (arrays) after comparing every one of them with the twin's"""
    want = twin.render_depth(xyz, normals, P, wh, plane, r, R, TOL, with_index)
    if tensors:
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if a is not None else None      # noqa: E731
        got = dens.render_depth(t(xyz), t(normals), P, wh, plane, r, R, TOL, with_index, cams_per_batch)
        assert all(g is None or (torch.is_tensor(g) and g.device == DEV) for g in got)
        got = tuple(None if g is None else g.cpu().numpy() for g in got)
    else:
        got = dens.render_depth(xyz, normals, P, wh, plane, r, R, TOL, with_index, cams_per_batch)
    dr.assert_equal(got, want, (len(xyz), plane, r, R, cams_per_batch))
    return got


@pytest.mark.parametrize("plane", [(1, 1), (16, 16), (37, 23), (130, 67)])
@pytest.mark.parametrize("n", [1, 255, 257, 70001])
def test_one_camera_equals_the_twin(dens, twin, n, plane):
    xyz, normals, P, wh = dr.random_scene(n, seed=n, n_cams=1)
    if n == 1:
        xyz[0] = [0.1, -0.1, 2.0]                                          # the one point is inside
    for r, R in MODES:
        depth, index, _ = both(dens, twin, xyz, normals, P, wh, plane, r, R, tensors=(r == 1))
        assert (index >= 0).any()
        assert (depth[index >= 0] > 0).all() and not depth[index < 0].any()


@pytest.mark.parametrize("per", [0, 2])
@pytest.mark.parametrize("n,plane", [(257, (37, 23)), (70001, (130, 67))])
def test_five_cameras_in_one_batch_and_in_batches_of_two(dens, twin, n, plane, per):
    xyz, normals, P, wh = dr.random_scene(n, seed=n + 1, n_cams=5)
    assert len({tuple(x) for x in wh.tolist()}) >= 4                       # several aspect ratios on the one plane
    for r, R in MODES:
        _, index, _ = both(dens, twin, xyz, normals, P, wh, plane, r, R, cams_per_batch=per)
        assert all((index[c] >= 0).any() for c in range(5))


def test_every_point_in_one_cell_a_quarter_of_them_at_the_minimal_depth(dens, twin):
    n = 70001
    rng = np.random.default_rng(9)
    P = np.array([[64.0, 0, 32, 0], [0, 64.0, 32, 0], [0, 0, 1, 0]], np.float32).reshape(1, 12)
    wh = np.array([[64, 64]], np.int32)
    z = np.where(rng.random(n) < 0.25, 2.0, rng.uniform(2.0, 5.0, n))
    z[:100] = 3.0                                                          # the winner is not the first point
    u, v = rng.uniform(32.5, 35.5, n), rng.uniform(32.5, 35.5, n)          # cell (8, 8) of 16 x 16, well inside it
    xyz = np.column_stack([(u - 32.0) * z / 64.0, (v - 32.0) * z / 64.0, z]).astype(np.float32)
    normals = rng.normal(size=(n, 3)).astype(np.float32)
    ok, cx, cy, d = dr.project(P[0], 64, 64, 16, 16, xyz)
    assert ok.all() and (cx == 8).all() and (cy == 8).all() and 0.2 * n < (d == 2.0).sum() < 0.3 * n
    first = int(np.flatnonzero(d == d.min())[0])
    assert first >= 100 and d.min() == np.float32(2.0)
    for r, R in MODES:
        depth, index, normal = both(dens, twin, xyz, normals, P, wh, (16, 16), r, R)
        assert index[0, 8, 8] == first and depth[0, 8, 8] == np.float32(2.0)
        assert (index >= 0).sum() == (2 * r + 1) ** 2 and (index[index >= 0] == first).all()
        assert np.array_equal(dr.bits(normal[0, 8, 8]), dr.bits(normals[first]))


def test_optional_outputs_and_no_points(dens, twin):
    xyz, normals, P, wh = dr.random_scene(5000, seed=3, n_cams=3)
    full = both(dens, twin, xyz, normals, P, wh, (37, 23), 1, 3)
    for nrm, with_index in ((None, True), (normals, False), (None, False)):
        got = both(dens, twin, xyz, nrm, P, wh, (37, 23), 1, 3, with_index=with_index, tensors=True)
        assert (got[1] is None) == (not with_index) and (got[2] is None) == (nrm is None)
        assert np.array_equal(dr.bits(got[0]), dr.bits(full[0]))           # the depth does not depend on what else is asked for
    empty = np.zeros((0, 3), np.float32)
    for nrm in (None, empty):
        depth, index, normal = both(dens, twin, empty, nrm, P, wh, (37, 23), 1, 3)
        assert not depth.any() and (index == -1).all() and (normal is None or not normal.any())


def test_a_context_reused_at_other_sizes_and_between_calls_of_another_stage(dens, twin):
    big = dr.random_scene(70001, seed=11, n_cams=5)
    small = dr.random_scene(257, seed=12, n_cams=2)
    fxyz, fcounts, fP, fwh = fs.ring_cloud(5, 5000, seed=13)
    first = both(dens, twin, *small, (16, 16), 1, 3)
    both(dens, twin, *big, (130, 67), 3, 8)                                # grows the workspace and dirties it
    again = both(dens, twin, *small, (16, 16), 1, 3)                       # the small call inside the large call's words
    for a, b in zip(first, again):
        assert np.array_equal(dr.bits(a) if a.dtype == np.float32 else a, dr.bits(b) if b.dtype == np.float32 else b)
    freespace_both(dens, twin, fxyz, fcounts, fP, fwh, (64, 41), 0.02, 1, True)          # another stage carves the same workspace
    both(dens, twin, *big, (37, 23), 1, 3, cams_per_batch=2)
    freespace_both(dens, twin, fxyz, fcounts, fP, fwh, (64, 41), 0.02, 1, True)
    both(dens, twin, *small, (130, 67), 0, 0)


def test_a_host_context_and_a_device_context_refuse_each_other(dens, twin):
    lib = hb.load_library()
    null = (None, 0, None, None, None, 1, 1, 1, 1, 3, 0.02, 0, None, None, None)
    assert lib.lfd_render_depth_host(dens._ctx, *null) == 4 and lib.lfd_render_depth(twin._ctx, *null) == 4       # LFD_ERR_STATE
