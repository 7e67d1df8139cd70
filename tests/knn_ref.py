"""What the tests of the Gaussian-ready output share: the brute-force NumPy reference of lfd_knn_dist2 - every f32 rounding in
the order the contract writes it out -, the NumPy formula of the 68-byte record, and the clouds (a) .. (g) of the issue."""
import functools
import math

import numpy as np

REC68 = np.dtype([("xyz", "<f4", 3), ("normal", "<f4", 3), ("f_dc", "<f4", 3), ("opacity", "<f4"), ("scale", "<f4", 3), ("rot", "<f4", 4)])
PROPERTIES = ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2", "opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2",
              "rot_3"]
SH_C0 = np.float32(0.28209479177387814)


def brute_dist2(xyz: np.ndarray) -> np.ndarray:
    """((a + b) + c) / 3 over the three smallest d2 = (dx dx + dy dy) + dz dz, all in f32, the point itself left out BY INDEX."""
    x = np.ascontiguousarray(xyz, np.float32)
    n = x.shape[0]
    out = np.empty(n, np.float32)
    with np.errstate(over="ignore"):
        for i in range(n):
            d = x[i][None, :] - x                                  # f32
            s = d * d
            d2 = (s[:, 0] + s[:, 1]) + s[:, 2]
            d2 = np.delete(d2, i)
            a, b, c = np.sort(d2)[:3]
            out[i] = ((a + b) + c) / np.float32(3.0)
    assert out.dtype == np.float32
    return out


def third_neighbour(xyz: np.ndarray) -> np.ndarray:
    """f64 distance of every point to its third nearest neighbour (for the statements the tests make about the clouds themselves)."""
    x = np.asarray(xyz, np.float64)
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d2, np.inf)
    return np.sqrt(np.sort(d2, axis=1)[:, 2])


def to_u8(rgb: np.ndarray) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return np.clip(np.nan_to_num(np.round(np.asarray(rgb, np.float32) * np.float32(255.0)), nan=0.0), 0, 255).astype(np.uint8)      # (NaN -> 0)


def dc_of_u8(q: np.ndarray) -> np.ndarray:
    return ((q.astype(np.float32) / np.float32(255.0)) - np.float32(0.5)) / SH_C0


def rot_of_normals(nrm: np.ndarray) -> np.ndarray:
    nrm = np.asarray(nrm, np.float32)
    n = nrm.shape[0]
    q = np.zeros((n, 4), np.float32)
    q[:, 0] = 1.0
    usable = np.isfinite(nrm).all(1) & (nrm != 0).any(1)
    w = np.float32(1.0) + nrm[:, 2]
    flip = usable & (w < np.float32(2.0 ** -23))
    q[flip] = (0.0, 1.0, 0.0, 0.0)
    go = usable & ~flip
    x, y = -nrm[:, 1], nrm[:, 0]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        l = np.sqrt((w * w + x * x) + y * y)
        go &= np.isfinite(l) & (l > 0)
        q[go, 0], q[go, 1], q[go, 2] = (w / l)[go], (x / l)[go], (y / l)[go]
    return q


def gaussian_records_ref(xyz, nrm, rgb, dist2, opacity=0.1, flatten=1.0, max_scale=0.0) -> np.ndarray:
    n = int(np.asarray(xyz).shape[0])
    rec = np.empty(n, REC68)
    rec["xyz"] = np.asarray(xyz, np.float32)
    rec["normal"] = np.asarray(nrm, np.float32)
    rec["f_dc"] = dc_of_u8(to_u8(rgb))
    rec["opacity"] = np.float32(math.log(opacity / (1.0 - opacity)))
    m = np.maximum(np.asarray(dist2, np.float32), np.float32(1e-7))
    if max_scale > 0:
        cap = np.float32(min(max_scale * max_scale, 3.4028234663852886e38))
        m = np.minimum(m, cap if cap > 0 else np.float32(1.4012985e-45))      # (a square that rounds to 0 caps at the smallest positive f32)
    ls = 0.5 * np.log(m.astype(np.float64))
    rec["scale"][:, 0] = rec["scale"][:, 1] = ls.astype(np.float32)
    rec["scale"][:, 2] = (ls + math.log(flatten)).astype(np.float32)
    rec["rot"] = rot_of_normals(nrm)
    return rec


def ulp_distance(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """f32 values as ordered integers: the number of representable values between a and b (finite values)."""
    def key(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def rotate_z(q: np.ndarray) -> np.ndarray:
    """(0, 0, 1) rotated by the unit quaternions (w, x, y, z), in f64."""
    w, x, y, z = (np.asarray(q, np.float64)[:, k] for k in range(4))
    return np.stack([2 * (x * z + w * y), 2 * (y * z - w * x), 1 - 2 * (x * x + y * y)], 1)


# ---- the clouds ------------------------------------------------------------------------------------------------------------------------------
def surface_cloud(seed: int, n: int = 3000) -> np.ndarray:
    rs = np.random.RandomState(seed)
    return np.concatenate([rs.uniform(-1.0, 1.0, (n, 2)), rs.normal(0.0, 0.01, (n, 1))], 1).astype(np.float32)


FAR = np.array([[1000.0, 0.0, 0.0], [-500.0, 3.0, 2.0], [-500.0, 3.0, 2.001]], np.float32)


@functools.lru_cache(maxsize=None)
def cloud(name: str) -> np.ndarray:
    rs = np.random.RandomState(11)
    if name in ("a4", "a5", "b64", "b65", "b257"):
        out = rs.uniform(-1.0, 1.0, (int(name[1:]), 3)).astype(np.float32)
    elif name == "c":
        out = np.concatenate([np.tile(np.array([[0.25, -0.5, 0.125]], np.float32), (4, 1)), rs.uniform(-1.0, 1.0, (60, 3)).astype(np.float32)])
    elif name == "d":
        g = np.arange(6, dtype=np.float32)
        out = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    elif name == "e":
        out = np.zeros((200, 3), np.float32)
        out[:, 0] = -np.sort(rs.uniform(0.5, 40.0, 200)).astype(np.float32)
    elif name.startswith("f"):
        out = surface_cloud(int(name[1:]))
    elif name.startswith("g"):
        out = np.concatenate([surface_cloud(int(name[1:])), FAR])
    else:
        raise KeyError(name)
    out.setflags(write=False)
    return out


ALL = ["a4", "a5", "b64", "b65", "b257", "c", "d", "e", "f0", "f1", "f2", "g0", "g1", "g2"]
FORCED = ["d", "f0", "f1", "f2", "g0", "g1", "g2"]        # also run with the cell size forced to 0.01 L, L and 10 L (L: the longest box side)


@functools.lru_cache(maxsize=None)
def reference(name: str) -> np.ndarray:
    out = brute_dist2(cloud(name))
    out.setflags(write=False)
    return out


def longest_side(xyz: np.ndarray) -> float:
    x = np.asarray(xyz, np.float64)
    return float((x.max(0) - x.min(0)).max())


def cell_sizes(name: str):
    """0 = automatic for every cloud; the forced sizes for (d), (f), (g) - and the three lattice sizes that put points on cell faces for (d)."""
    if name not in FORCED:
        return [0.0]
    L = longest_side(cloud(name))
    return [0.0, 0.01 * L, L, 10.0 * L] + ([1.0, 2.0, 0.5] if name == "d" else [])
