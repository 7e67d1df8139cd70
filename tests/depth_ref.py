"""Brute-force NumPy reference of the depth-map renderer (lfd_render_depth): the definition and nothing else - an f64 projection
with every sum written out, ``np.minimum.at`` on u64 keys over the full footprint, a direct loop over the visibility window.  Neither of the two
min-filter identities the device uses, no tiles, no batches."""
import numpy as np

EMPTY_BITS = np.uint64(0x7F800000)
EMPTY = np.uint64((0x7F800000 << 32) | 0xFFFFFFFF)


def project(P, w, h, pw, ph, xyz):
    """inside (bool [n]), cx, cy (int64 [n], 0 outside), d (f32 [n], meaningless outside) of the points in one camera"""
    P = np.asarray(P, np.float32).reshape(12).astype(np.float64)
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    X, Y, Z = (xyz[:, k].astype(np.float64) for k in range(3))
    with np.errstate(all="ignore"):
        a0, a1, a2 = P[0] * X, P[1] * Y, P[2] * Z
        b0, b1, b2 = P[4] * X, P[5] * Y, P[6] * Z
        c0, c1, c2 = P[8] * X, P[9] * Y, P[10] * Z
        s0, s1, s2 = a0 + a1, b0 + b1, c0 + c1
        t0, t1, t2 = s0 + a2, s1 + b2, s2 + c2
        p0, p1, p2 = t0 + P[3], t1 + P[7], t2 + P[11]
        ok = np.isfinite(p0) & np.isfinite(p1) & np.isfinite(p2) & (p2 > 0.0)
        u, v = p0 / p2, p1 / p2
        ok &= (u >= 0.0) & (u < float(w)) & (v >= 0.0) & (v < float(h))
        d = p2.astype(np.float32)
        ok &= (d > 0) & np.isfinite(d)
        cx = np.minimum(float(pw - 1), np.floor((u * float(pw)) / float(w)))
        cy = np.minimum(float(ph - 1), np.floor((v * float(ph)) / float(h)))
    cx = np.where(ok, cx, 0.0).astype(np.int64)
    cy = np.where(ok, cy, 0.0).astype(np.int64)
    return ok, cx, cy, d


def keys_of(P, w, h, pw, ph, xyz, r):
    """K (u64 [ph, pw]): the smallest key of the points whose cell lies within Chebyshev distance r, EMPTY where there are none"""
    ok, cx, cy, d = project(P, w, h, pw, ph, xyz)
    idx = np.flatnonzero(ok)
    key = (np.ascontiguousarray(d[idx]).view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)
    K = np.full((ph, pw), EMPTY, np.uint64)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            x, y = cx[idx] + dx, cy[idx] + dy
            m = (x >= 0) & (x < pw) & (y >= 0) & (y < ph)              # only the in-plane part of the footprint counts
            np.minimum.at(K, (y[m], x[m]), key[m])
    return K


def render_camera(P, w, h, pw, ph, xyz, r, R, tol, normals=None):
    """(depth f32 [ph, pw], index i32 [ph, pw], normal f32 [ph, pw, 3] or None) of one camera"""
    K = keys_of(P, w, h, pw, ph, xyz, r)
    bits = (K >> np.uint64(32)).astype(np.uint32)
    index = (K & np.uint64(0xFFFFFFFF)).astype(np.int64)
    tol = np.float32(tol)
    depth = np.zeros((ph, pw), np.float32)
    out_idx = np.full((ph, pw), -1, np.int32)
    for y in range(ph):
        for x in range(pw):
            if bits[y, x] >= 0x7F800000:
                continue
            win = bits[max(0, y - R):min(ph, y + R + 1), max(0, x - R):min(pw, x + R + 1)]
            m = win.min().reshape(1).view(np.float32)[0]                # the cell itself is finite: so is the window's minimum
            D = bits[y, x].reshape(1).view(np.float32)[0]
            t = np.float32(tol * m)
            hi = np.float32(m + t)
            if D <= hi:
                depth[y, x] = D
                out_idx[y, x] = index[y, x]
    normal = None
    if normals is not None:
        normals = np.asarray(normals, np.float32).reshape(-1, 3)
        normal = np.zeros((ph, pw, 3), np.float32)
        keep = out_idx >= 0
        normal[keep] = normals[out_idx[keep]]
    return depth, out_idx, normal


def render(xyz, normals, P, wh, pw, ph, r, R, tol):
    """(depth [n_cams, ph, pw], index, normal or None) over all cameras"""
    P = np.asarray(P, np.float32).reshape(-1, 12)
    wh = np.asarray(wh, np.int32).reshape(-1, 2)
    outs = [render_camera(P[c], wh[c, 0], wh[c, 1], pw, ph, xyz, r, R, tol, normals) for c in range(P.shape[0])]
    depth, index = np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])
    return depth, index, (np.stack([o[2] for o in outs]) if normals is not None else None)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_equal(got, want, what=""):
    """depth and normals by bit pattern, indices by value"""
    for g, w, name in zip(got, want, ("depth", "index", "normal")):
        assert (g is None) == (w is None), (what, name)
        if g is None:
            continue
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        same = np.array_equal(bits(g), bits(w)) if g.dtype == np.float32 else np.array_equal(g, w)
        assert same, (what, name, np.argwhere(g != w)[:10])


def random_scene(n, seed, n_cams=3):
    """n random points in front of n_cams pinhole cameras near the origin that look down +z, the second of another aspect ratio; normals too"""
    rng = np.random.default_rng(seed)
    xyz = np.column_stack([rng.uniform(-2.0, 2.0, n), rng.uniform(-1.5, 1.5, n), rng.uniform(1.0, 6.0, n)]).astype(np.float32)
    normals = rng.normal(size=(n, 3)).astype(np.float32)
    sizes = [(64, 40), (30, 50), (64, 40), (48, 48), (80, 20)]
    P, wh = [], []
    for c in range(n_cams):
        w, h = sizes[c % len(sizes)]
        f = 0.9 * w + 3.0 * c
        a = 0.15 * (c - 1)                                             # a small turn about y
        Rm = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
        t = np.array([0.2 * c - 0.2, 0.1 * c, 0.3])
        Kc = np.array([[f, 0.0, w / 2.0], [0.0, f, h / 2.0], [0.0, 0.0, 1.0]])
        P.append((Kc @ np.column_stack([Rm, t])).astype(np.float32).reshape(12))
        wh.append([w, h])
    return xyz, normals, np.stack(P), np.array(wh, np.int32)
