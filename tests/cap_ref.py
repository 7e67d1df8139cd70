"""NumPy reference of the spatial point cap (lfd_cap_spatial), written from the rule in include/lfd_densify.h, and the clouds the
cap's tests share.  Nothing here calls the library."""
import numpy as np

LEVELS = 21


def keys_ref(xyz):
    """``(keys, L)``: the 63-bit Morton key of every point (uint64) and the longest side of the bounding box (f64 from the f32 min and max)."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    L = float(np.max(hi.astype(np.float64) - lo.astype(np.float64)))
    if L > 0.0:
        t = (xyz.astype(np.float64) - lo.astype(np.float64)) / L
        u = t * 2097152.0
        q = np.where(u >= 2097151.0, 2097151.0, np.floor(u)).astype(np.uint64)
    else:
        q = np.zeros(xyz.shape, np.uint64)
    keys = np.zeros(xyz.shape[0], np.uint64)
    for bit in range(LEVELS):
        for axis in range(3):
            keys |= ((q[:, axis] >> np.uint64(bit)) & np.uint64(1)) << np.uint64(3 * bit + 2 - axis)
    return keys, L


def rank_ref(err):
    """The monotone integer image of the f32 bit patterns (uint32): -0 < +0, NaN patterns by their bits."""
    bits = np.ascontiguousarray(err, np.float32).view(np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def cap_ref(xyz, err, m):
    """``(keep, stats)``: the kept input indices, ascending (int64), and ``(lev, cells(lev), cells(lev - 1) or 0, L)``."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    n, m = int(xyz.shape[0]), int(m)
    assert m >= 1
    if n == 0:
        return np.zeros(0, np.int64), (0, 0, 0, 0.0)
    keys, L = keys_ref(xyz)
    cells = [int(np.unique(keys >> np.uint64(3 * (LEVELS - l))).size) for l in range(LEVELS + 1)]
    lev = next((l for l in range(LEVELS + 1) if cells[l] >= m), LEVELS)
    c = cells[lev]
    stats = (lev, c, cells[lev - 1] if lev > 0 else 0, L)
    if n <= m:
        return np.arange(n, dtype=np.int64), stats
    cell_keys = keys >> np.uint64(3 * (LEVELS - lev))
    _, cell_of = np.unique(cell_keys, return_inverse=True)               # cell number in Morton order
    cell_of = cell_of.reshape(-1)
    rank = rank_ref(err).astype(np.uint64) if err is not None else np.zeros(n, np.uint64)
    packed = (rank << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    best = np.full(c, np.iinfo(np.uint64).max, np.uint64)
    np.minimum.at(best, cell_of, packed)
    k = np.arange(c, dtype=object)                                       # Python integers: no overflow to think about
    picked = np.array([True] * c) if c <= m else np.array([((int(v) + 1) * m) // c > (int(v) * m) // c for v in k])
    keep = np.sort((best[picked] & np.uint64(0xffffffff)).astype(np.int64))
    return keep, stats


# ---- the clouds ----------------------------------------------------------------------------------------------------------------------------------
def two_density(seed):
    """(f): two unit squares side by side, 20 000 points and 2 000, z ~ N(0, 0.002), shuffled.  Returns ``(xyz, err, dense)`` - ``dense`` marks the
    points of the dense square."""
    rng = np.random.default_rng(seed)
    a = np.column_stack([rng.uniform(0, 1, 20000), rng.uniform(0, 1, 20000), rng.normal(0, 0.002, 20000)])
    b = np.column_stack([rng.uniform(1, 2, 2000), rng.uniform(0, 1, 2000), rng.normal(0, 0.002, 2000)])
    xyz = np.concatenate([a, b]).astype(np.float32)
    dense = np.concatenate([np.ones(20000, bool), np.zeros(2000, bool)])
    order = rng.permutation(xyz.shape[0])
    err = rng.uniform(0, 2, xyz.shape[0]).astype(np.float32)
    return xyz[order], err, dense[order]


def clouds():
    """``[(name, xyz, err, m), ...]``: the cases (a) - (g) of the cap's tests."""
    out = []
    rng = np.random.default_rng(11)
    five = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [0.5, 0.5, 3], [0.25, 1.5, 1.0]], np.float32)
    for m in (1, 2, 3, 4):
        out.append((f"a-m{m}", five, np.array([3, 1, 2, 0.5, 1], np.float32), m))
    for n in (64, 65, 257):
        xyz = rng.uniform(-2, 3, (n, 3)).astype(np.float32)
        err = rng.uniform(0, 1, n).astype(np.float32)
        for m in (1, n // 2, n - 1):
            out.append((f"b-n{n}-m{m}", xyz, err, m))
    pt = np.array([[0.3, -0.7, 1.1]], np.float32)
    mixed = np.concatenate([np.repeat(pt, 40, axis=0), rng.uniform(-1, 2, (60, 3)).astype(np.float32)])[rng.permutation(100)]
    for m in (30, 80):
        out.append((f"c-m{m}", mixed, rng.uniform(0, 1, 100).astype(np.float32), m))
    out.append(("c-identical", np.repeat(pt, 50, axis=0), rng.uniform(0, 1, 50).astype(np.float32), 10))
    g = np.arange(8, dtype=np.float32)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    for m in (7, 64, 100, 511):
        out.append((f"d-m{m}", lattice, rng.uniform(0, 1, 512).astype(np.float32), m))
    s = np.linspace(0, 1, 200, dtype=np.float32)[rng.permutation(200)]
    line = np.column_stack([-5.0 - 3.0 * s, -1.0 + 2.0 * s, -7.5 * np.ones(200, np.float32) - s]).astype(np.float32)
    for m in (17, 199):
        out.append((f"e-m{m}", line, rng.uniform(0, 1, 200).astype(np.float32), m))
    for seed in (0, 1, 2):
        xyz, err, _ = two_density(seed)
        for m in (1000, 257):
            out.append((f"f-s{seed}-m{m}", xyz, err, m))
    xyz, err, _ = two_density(0)
    far = np.concatenate([xyz, np.array([[1000, 0, 0]], np.float32)])
    for m in (1000, 257):
        out.append((f"g-m{m}", far, np.concatenate([err, np.array([0.5], np.float32)]), m))
    return out
