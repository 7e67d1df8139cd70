"""NumPy reference of oriented voxel fusion (lfd_fuse_oriented): the rule and nothing else, with explicit per-voxel loops -
the keys of densify._voxel_downsample (np.unique(axis=0) on the f64 floor), sequential f64 sums in ascending input index, IEEE sqrt and divide.
Also the clouds the host and the GPU tests share."""
import numpy as np


def usable_normals(normals):
    n = np.asarray(normals, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.isfinite(n).all(axis=1) & (((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]) > 0.0)


def fuse_ref(xyz, normals, rgb, h):
    """-> (xyz_out, normals_out, rgb_out float32 [rows, 3], count int64 [rows], side int64 [rows], n_voxels)"""
    xyz, normals, rgb = (np.asarray(a, np.float32).reshape(-1, 3) for a in (xyz, normals, rgb))
    n = xyz.shape[0]
    if n == 0:
        e = np.zeros((0, 3), np.float32)
        return e, e.copy(), e.copy(), np.zeros(0, np.int64), np.zeros(0, np.int64), 0
    pts = xyz.astype(np.float64)
    with np.errstate(invalid="ignore"):
        scale = 255.0 if rgb.max() > 1.0 else 1.0           # a NaN maximum compares False: 1
    col = rgb.astype(np.float64) / scale
    N = normals.astype(np.float64)
    origin = pts.min(axis=0) - 0.5 * h
    key = np.floor((pts - origin) / float(h)).astype(np.int64)
    uq, inv = np.unique(key, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    order = np.argsort(inv, kind="stable")                  # voxels in key order, input order inside each
    starts = np.searchsorted(inv[order], np.arange(len(uq)))
    ends = np.append(starts[1:], n)
    ok = usable_normals(normals)
    out_x, out_n, out_c, out_cnt, out_side = [], [], [], [], []
    for a, b in zip(starts, ends):
        idx = order[a:b]
        pivot = None
        for i in idx:
            if ok[i]:
                pivot = N[i]
                break
        side = np.zeros(len(idx), np.int64)
        if pivot is not None:
            for t, i in enumerate(idx):
                if ok[i]:
                    d = (N[i, 0] * pivot[0] + N[i, 1] * pivot[1]) + N[i, 2] * pivot[2]
                    side[t] = 1 if d < 0.0 else 0
        for s in (0, 1):
            members = idx[side == s]
            if len(members) == 0:
                continue
            p, c, q = np.zeros(3), np.zeros(3), np.zeros(3)
            with np.errstate(invalid="ignore", over="ignore"):
                for i in members:
                    p = p + pts[i]
                    c = c + col[i]
                    if ok[i]:
                        q = q + N[i]
                qq = (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]
                nn = q / np.sqrt(qq) if (np.isfinite(qq) and qq > 0.0) else np.zeros(3)
                out_x.append((p / float(len(members))).astype(np.float32))
                out_c.append((c / float(len(members))).astype(np.float32))
            out_n.append(nn.astype(np.float32))
            out_cnt.append(len(members))
            out_side.append(s)
    return (np.stack(out_x), np.stack(out_n), np.stack(out_c), np.array(out_cnt, np.int64), np.array(out_side, np.int64), len(uq))


def voxel_mean_ref(xyz, rgb, h):
    """The NumPy branch of densify._voxel_downsample, restated (np.add.at sums)."""
    xyz, rgb = np.asarray(xyz, np.float32), np.asarray(rgb, np.float32)
    with np.errstate(invalid="ignore"):
        col = rgb.astype(np.float64) / (255.0 if rgb.size and rgb.max() > 1.0 else 1.0)
    pts = xyz.astype(np.float64)
    origin = pts.min(axis=0) - 0.5 * h
    key = np.floor((pts - origin) / float(h)).astype(np.int64)
    _, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    p, c = np.zeros((cnt.size, 3)), np.zeros((cnt.size, 3))
    np.add.at(p, inv, pts)
    np.add.at(c, inv, col)
    return (p / cnt[:, None]).astype(np.float32), (c / cnt[:, None]).astype(np.float32)


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def noisy_normals(rng, n0, sigma_deg, m):
    """m unit vectors around n0 with about sigma_deg of angular noise"""
    v = np.asarray(n0, np.float64) + rng.normal(0.0, np.tan(np.deg2rad(sigma_deg)) / np.sqrt(2.0), (m, 3))
    return unit(v)


def angle_deg(a, b):
    return np.rad2deg(np.arccos(np.clip((np.asarray(a, np.float64) * np.asarray(b, np.float64)).sum(-1), -1.0, 1.0)))


def uniform_cloud(seed, n):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32), unit(rng.normal(size=(n, 3))).astype(np.float32),
            rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32))


def clustered_cloud(seed, n, n_clusters=40, spread=0.02, flip=0.33):
    """Points around cluster centres; every cluster has an axis, its points' normals lie within about 25 degrees of it, and in a share `flip` of the
    clusters half of the points face the other way."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-1.0, 1.0, (n_clusters, 3))
    axes = unit(rng.normal(size=(n_clusters, 3)))
    two = rng.uniform(size=n_clusters) < flip
    which = rng.integers(0, n_clusters, n)
    xyz = (centres[which] + rng.normal(0.0, spread, (n, 3))).astype(np.float32)
    nrm = unit(axes[which] + rng.normal(0.0, 0.2, (n, 3)))
    sign = np.where(two[which] & (rng.uniform(size=n) < 0.5), -1.0, 1.0)
    return xyz, (nrm * sign[:, None]).astype(np.float32), rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)


def one_sided_cloud(seed, n):
    """Every normal within 30 degrees of +z: all pairwise dot products are positive"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    tilt = np.deg2rad(rng.uniform(0.0, 29.0, n))
    az = rng.uniform(0.0, 2.0 * np.pi, n)
    nrm = np.stack([np.sin(tilt) * np.cos(az), np.sin(tilt) * np.sin(az), np.cos(tilt)], axis=1).astype(np.float32)
    return xyz, nrm, rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)


def tilted_plane_scene(seed=7):
    """Usefulness scene (a): six references sample one tilted plane on jittered 0.01-spaced grids, normals with about 10 degrees of noise"""
    rng = np.random.default_rng(seed)
    n0 = unit(np.array([0.3, -0.2, 1.0]))
    u = unit(np.cross(n0, [1.0, 0.0, 0.0]))
    w = np.cross(n0, u)
    P, N = [], []
    for _ in range(6):
        g = np.stack(np.meshgrid(np.arange(40), np.arange(40)), -1).reshape(-1, 2) * 0.01 + rng.uniform(0.0, 0.01, 2)
        P.append(g[:, :1] * u + g[:, 1:] * w + rng.normal(0.0, 0.0005, (len(g), 1)) * n0)
        N.append(noisy_normals(rng, n0, 10.0, len(g)))
    P, N = np.concatenate(P).astype(np.float32), np.concatenate(N).astype(np.float32)
    return P, N, np.full_like(P, 0.5), n0


def thin_wall_scene(seed=7):
    """Usefulness scene (b): two faces at z = 0.010 and z = 0.030 with opposite normals, shuffled; h = 0.05"""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(60), np.arange(60)), -1).reshape(-1, 2) * 0.004
    front = np.c_[g, np.full(len(g), 0.010)] + rng.normal(0.0, 0.0005, (len(g), 3)) * [0.0, 0.0, 1.0]
    back = np.c_[g, np.full(len(g), 0.030)] + rng.normal(0.0, 0.0005, (len(g), 3)) * [0.0, 0.0, 1.0]
    X = np.r_[front, back].astype(np.float32)
    N = np.r_[noisy_normals(rng, [0.0, 0.0, -1.0], 10.0, len(g)), noisy_normals(rng, [0.0, 0.0, 1.0], 10.0, len(g))].astype(np.float32)
    perm = rng.permutation(len(X))
    return X[perm], N[perm], np.full_like(X, 0.5)
