"""NumPy / Python-int reference of the footprint-adaptive thinning (lfd_thin_footprint), written from the rule in
include/lfd_densify.h: brute force, a dict from location code to the minimum of (error rank, input index).  Nothing here calls the library."""
import numpy as np

from cap_ref import keys_ref, rank_ref

LEVELS = 21          # levels 0 .. 20
MAX_LEVEL = 20


def offsets(ref_counts):
    offs = np.zeros(len(ref_counts) + 1, np.int64)
    np.cumsum(np.asarray(ref_counts, np.int64), out=offs[1:])
    return offs


def levels_ref(xyz, ref_counts, rows, thin_cells, L):
    """The level of every point (int64): every f64 operation is one NumPy ufunc call, so one rounding."""
    xyz = np.ascontiguousarray(xyz, np.float32).astype(np.float64)
    rows = np.asarray(rows, np.float64).reshape(-1, 5)
    ref = np.repeat(np.arange(len(ref_counts)), np.asarray(ref_counts, np.int64))
    r = rows[ref]
    ax = r[:, 0] * xyz[:, 0]
    ay = r[:, 1] * xyz[:, 1]
    az = r[:, 2] * xyz[:, 2]
    z = ((ax + ay) + az) + r[:, 3]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        g = (z * r[:, 4]) * np.float64(thin_cells)
        lev = np.full(xyz.shape[0], MAX_LEVEL, np.int64)
        ok = (g > 0) & ~np.isinf(g) & (L > 0)
        q = np.where(ok, np.float64(L) / np.where(ok, g, 1.0), 0.0)
    e = ((q.view(np.uint64) >> np.uint64(52)) & np.uint64(0x7ff)).astype(np.int64) - 1023
    lev[ok] = np.where(q[ok] < 1.0, 0, np.minimum(e[ok], MAX_LEVEL))
    return lev


def codes_ref(xyz, ref_counts, rows, thin_cells):
    """``(codes, levels, L)``: the location code of every point as a Python int."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    keys, L = keys_ref(xyz)
    lev = levels_ref(xyz, ref_counts, rows, thin_cells, L)
    codes = [(1 << (3 * int(l))) | (int(k) >> (3 * (21 - int(l)))) for k, l in zip(keys.tolist(), lev.tolist())]
    return codes, lev, L


def thin_ref(xyz, err, ref_counts, rows, thin_cells):
    """``(keep, counts, (points per level, cells per level, L))``: the kept input indices, ascending (int64), the kept points per reference and the
    statistics as ``thin_stats`` holds them."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = int(xyz.shape[0])
    counts_in = np.asarray(ref_counts, np.int64)
    assert counts_in.sum() == n and thin_cells > 0
    points, cells = np.zeros(LEVELS, np.int64), np.zeros(LEVELS, np.int64)
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(len(counts_in), np.int64), (points, cells, 0.0)
    codes, lev, L = codes_ref(xyz, counts_in, rows, thin_cells)
    rank = rank_ref(err).tolist() if err is not None else [0] * n
    best = {}
    for i, code in enumerate(codes):
        v = (rank[i], i)
        if code not in best or v < best[code]:
            best[code] = v
    keep = np.array(sorted(v[1] for v in best.values()), np.int64)
    for l in lev.tolist():
        points[l] += 1
    for code in best:
        cells[(code.bit_length() - 1) // 3] += 1
    offs = offsets(counts_in)
    counts = np.diff(np.searchsorted(keep, offs, side="left"))
    return keep, counts.astype(np.int64), (points, cells, L)


def random_case(n, ref_counts, seed, dupes=0):
    """``(xyz, err, rows)``: n points in a box of about 8 units, with ``dupes`` copies of one point in front, an error of few values (ties in
    every cell) and per reference a camera some 6 - 12 units away looking at the box, with a cell tangent of 0.004 - 0.02."""
    rng = np.random.default_rng(seed)
    xyz = np.column_stack([rng.uniform(-3, 5, n), rng.uniform(0, 2, n), rng.normal(0, 0.5, n)]).astype(np.float32)
    if dupes:
        xyz[:dupes] = xyz[dupes]
    err = (rng.integers(0, 16, n) / 16.0).astype(np.float32)
    rows = []
    for _ in range(len(ref_counts)):
        axis = rng.normal(0, 1, 3)
        axis /= np.linalg.norm(axis)
        rows.append([axis[0], axis[1], axis[2], rng.uniform(6, 12), rng.uniform(0.004, 0.02)])
    return xyz, err, np.asarray(rows, np.float64)
