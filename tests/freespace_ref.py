"""Brute-force NumPy reference of the free-space filter (lfd_freespace_filter): the definition and nothing else - an f64
projection with every sum written out, ``np.minimum.at`` for the z-buffers, the 3 x 3 window, the two counts.  No kernel structure, no camera
table, no chunks."""
import numpy as np

f32 = np.float32
INF = np.float32(np.inf)


def ref_ids(counts):
    return np.repeat(np.arange(len(counts)), np.asarray(counts, np.int64))


def cameras(cams, idx=None):
    """(P [n, 12] f32, wh [n, 2] i32) of CameraRecords"""
    idx = range(len(cams)) if idx is None else idx
    P = np.stack([np.asarray(cams[i].P, np.float64).astype(np.float32).reshape(12) for i in idx])
    wh = np.array([[cams[i].width, cams[i].height] for i in idx], np.int32)
    return P, wh


def project(P, w, h, pw, ph, xyz):
    """inside (bool [n]), cx, cy (int64 [n], 0 outside), d (f32 [n], meaningless outside) of the points in one camera"""
    P = np.asarray(P, np.float32).reshape(3, 4).astype(np.float64)
    X = np.asarray(xyz, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        p = [((P[r, 0] * X[:, 0] + P[r, 1] * X[:, 1]) + P[r, 2] * X[:, 2]) + P[r, 3] for r in range(3)]
        ok = np.isfinite(p[0]) & np.isfinite(p[1]) & np.isfinite(p[2]) & (p[2] > 0.0)
        u, v = p[0] / p[2], p[1] / p[2]
        d = p[2].astype(np.float32)
        ok &= (u >= 0.0) & (u < float(w)) & (v >= 0.0) & (v < float(h)) & np.isfinite(d) & (d > 0)
        cx = np.minimum(float(pw - 1), np.floor((u * float(pw)) / float(w)))
        cy = np.minimum(float(ph - 1), np.floor((v * float(ph)) / float(h)))
    cx = np.where(ok, cx, 0.0).astype(np.int64)
    cy = np.where(ok, cy, 0.0).astype(np.int64)
    return ok, cx, cy, d


def zbuffers(xyz, counts, P, wh, pw, ph):
    """Z [n_refs, ph, pw] f32: the smallest depth of every reference's OWN points per cell, +inf where there are none"""
    offs = np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))])
    Z = np.full((len(counts), ph, pw), INF, np.float32)
    for r in range(len(counts)):
        own = xyz[offs[r]:offs[r + 1]]
        ok, cx, cy, d = project(P[r], wh[r, 0], wh[r, 1], pw, ph, own)
        np.minimum.at(Z[r], (cy[ok], cx[ok]), d[ok])
    return Z


def counts_of(xyz, counts, P, wh, pw, ph, tol):
    """(violations, supports): int64 [n] each, unsaturated"""
    xyz = np.ascontiguousarray(xyz, np.float32)
    n = xyz.shape[0]
    ids = ref_ids(counts)
    Z = zbuffers(xyz, counts, P, wh, pw, ph)
    tol = np.float32(tol)
    viol, supp = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for j in range(len(counts)):
        ok, cx, cy, d = project(P[j], wh[j, 0], wh[j, 1], pw, ph, xyz)
        ok &= ids != j
        Zp = np.full((ph + 2, pw + 2), INF, np.float32)              # a border of +inf: cells outside the plane hold nothing
        Zp[1:-1, 1:-1] = Z[j]
        support = np.zeros(n, bool)
        dmin = np.full(n, INF, np.float32)
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                D = Zp[cy + dy, cx + dx]
                fin = np.isfinite(D)
                with np.errstate(all="ignore"):
                    t = (tol * D).astype(np.float32)
                    lo, hi = (D - t).astype(np.float32), (D + t).astype(np.float32)
                    support |= fin & (lo <= d) & (d <= hi)
                dmin = np.where(fin, np.minimum(dmin, D), dmin)
        fin = np.isfinite(dmin)
        with np.errstate(all="ignore"):
            lo_min = (dmin - (tol * dmin).astype(np.float32)).astype(np.float32)
            refute = fin & ~support & (d < lo_min)
        supp += ok & support
        viol += ok & refute
    return viol, supp


def keep_mask(viol, supp, min_violations):
    return ~((viol >= min_violations) & (viol > supp))


def plane_size(cells, w, h):
    """(pw, ph): ``cells`` along the longer image side, the shorter side max(1, floor(cells * short / long + 0.5))"""
    lng, sht = max(int(w), int(h)), min(int(w), int(h))
    other = max(1, int(np.floor(cells * sht / lng + 0.5)))
    return (int(cells), other) if w >= h else (other, int(cells))
