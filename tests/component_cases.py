"""The clouds the connected-component filter's tests share (tests/test_component_host.py against the brute-force reference,
tests/test_gpu_component.py against the twin), each built once.  A case is ``(xyz float32 (n, 3), counts int64 per reference, radius)``; the
points are shuffled so that neither the input order nor the references follow the geometry."""
import functools

import numpy as np


def _finish(parts, n_refs, radius, seed):
    rng = np.random.default_rng(seed)
    xyz = np.concatenate(parts).astype(np.float32)
    xyz = xyz[rng.permutation(xyz.shape[0])]
    cuts = np.sort(rng.integers(0, xyz.shape[0] + 1, n_refs - 1))
    counts = np.diff(np.concatenate([[0], cuts, [xyz.shape[0]]])).astype(np.int64)
    return xyz, counts, float(radius)


@functools.lru_cache(maxsize=None)
def chain(n=2000, gap_at=None, radius=0.125):
    """n points on a line along x, 0.9 radius apart: a point is linked to its two neighbours and to nothing else (the next one is 1.8 radius
    away; the coordinates stay below 256, where an f32 resolves 1.6e-5, against a margin of 0.0125); with ``gap_at`` the step in front of
    that point is 1.01 radius instead.  Returns ``(xyz, radius)`` in LINE order: shuffling is the caller's business."""
    steps = np.full(n, 0.9 * radius)
    steps[0] = 0.0
    if gap_at is not None:
        steps[gap_at] = 1.01 * radius
    x = np.cumsum(steps)
    xyz = np.stack([x - 3.0, np.full(n, 0.5), np.full(n, -2.0)], 1).astype(np.float32)
    return xyz, float(radius)


@functools.lru_cache(maxsize=None)
def lattice_with_clumps(radius=0.1):
    """A 64 x 64 lattice at 0.7 radius (one component of 4 096 points: every point is united with up to four neighbours, all into one root),
    200 singletons on a coarse grid 3 radius apart, and 40 clumps of 1 .. 40 points, each inside a ball of diameter 0.5 radius (so complete
    graphs), 5 radius apart.  Returns the case and, per point, the size its component has by construction."""
    rng = np.random.default_rng(31)
    a = np.arange(64) * 0.7 * radius
    lat = np.stack(np.meshgrid(a, a, indexing="ij"), -1).reshape(-1, 2)
    lat = np.column_stack([lat, np.zeros(lat.shape[0])])
    g = np.stack(np.meshgrid(np.arange(20), np.arange(10), indexing="ij"), -1).reshape(-1, 2) * 3.0 * radius
    single = np.column_stack([g[:, 0], g[:, 1] - 40.0 * radius, np.full(200, 2.0 * radius)])
    clumps, sizes = [], [np.full(lat.shape[0], lat.shape[0]), np.ones(200, np.int64)]
    for k in range(1, 41):
        centre = np.array([(k % 8) * 5.0 * radius, 60.0 * radius + (k // 8) * 5.0 * radius, -3.0 * radius])
        d = rng.normal(size=(k, 3))
        d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.0, 0.24 * radius, (k, 1))
        clumps.append(centre + d)
        sizes.append(np.full(k, k))
    rng2 = np.random.default_rng(32)
    xyz = np.concatenate([lat, single] + clumps).astype(np.float32)
    want = np.concatenate(sizes)
    perm = rng2.permutation(xyz.shape[0])
    cuts = np.sort(rng2.integers(0, xyz.shape[0] + 1, 4))
    counts = np.diff(np.concatenate([[0], cuts, [xyz.shape[0]]])).astype(np.int64)
    return xyz[perm], counts, float(radius), want[perm]


@functools.lru_cache(maxsize=None)
def one_cell(n=5000, radius=1.0):
    """n points in ONE cell of the grid (side 1.000001 radius from the cloud's minimum): two blobs of diameter 0.3 radius in opposite corners,
    further apart than the radius - two components of n / 2 points that the grid cannot tell apart."""
    rng = np.random.default_rng(33)
    half = n // 2
    a = rng.uniform(0.0, 0.17 * radius, (half, 3))
    b = rng.uniform(0.8 * radius, 0.97 * radius, (n - half, 3))
    a[0] = 0.0                                                            # the minimum: the grid's origin
    xyz, counts, radius = _finish([a, b], 3, radius, 34)
    cell = np.floor((xyz.astype(np.float64) - xyz.astype(np.float64).min(0)) / (1.000001 * radius))
    assert not cell.any()
    return xyz, counts, radius


@functools.lru_cache(maxsize=None)
def clustered(n, n_refs, seed, sigma=0.03):
    """n points around 9 centres (the consensus tests' clustered cloud)"""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-3.0, 3.0, (9, 3))
    xyz = (centres[rng.integers(0, 9, n)] + rng.normal(0.0, sigma, (n, 3))).astype(np.float32)
    cuts = np.sort(rng.integers(0, n + 1, n_refs - 1))
    return xyz, np.diff(np.concatenate([[0], cuts, [n]])).astype(np.int64)
