"""Record what the host build of csrc/lfd_geometry.hpp::lfd_null_vector returns: g13_null_vector.npz.

    python tests/golden/make_null_vector_fixture.py [out.npz]
    python tests/golden/make_null_vector_fixture.py --rerecord          (see below)

Run it on the commit whose solver is to be the reference (the fixture in the tree was recorded on the parent of the
change that restructured the solver's pass 0); tests/test_null_vector_fixture.py then asks the current build for
bit-identical c[4] and the identical solve count on the stored matrices.  The matrices themselves are stored (f32),
not re-drawn by the test, so the comparison does not depend on the BLAS behind NumPy.

``--rerecord`` keeps the matrices and every record the current build still reproduces bit for bit, replaces the records it does not and
stores which (``rerecorded``) with what they were (``c_prev``, ``it_prev``).  It is for a change of the solver that is meant to change some
results - the shifted passes' inertia test replaced 48 records this way - and tests/test_null_vector_fixture.py names the indices it accepts.

Cases (column `kind`):
  0  DLT rows of synthetic.ring_cameras correspondences, pixel noise 0.1 .. 2 px (the ordinary cell)
  1  the same, noise-free: rank-deficient, sigma4 ~ 0
  2  the same, 10 .. 60 px noise: sigma4/sigma3 up to ~1
  3  point at infinity: the triangulated X has X[3] -> 0
  4  U diag(s) V^T with sigma4/sigma3 in {0.5, 0.9, 0.99, 0.999, 0.99999, 1}: the shifted passes run
  5  NaN / Inf entries, one per position and a few combinations
  6  zero, identity, ones, huge, tiny, repeated rows
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

SEED = 20240713


def _rows(P1, P2, u1, u2):
    u1, u2, P1f, P2f = u1.astype(np.float32), u2.astype(np.float32), P1.astype(np.float32), P2.astype(np.float32)
    return np.stack([u1[0] * P1f[2] - P1f[0], u1[1] * P1f[2] - P1f[1], u2[0] * P2f[2] - P2f[0], u2[1] * P2f[2] - P2f[1]]).astype(np.float32)


def _dlt(rng, cams, noise_px, X=None):
    i = rng.randint(len(cams))
    j = (i + rng.randint(1, 4)) % len(cams)
    P1, P2 = np.asarray(cams[i].P, np.float64), np.asarray(cams[j].P, np.float64)
    if X is None:
        X = np.array([rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(-0.3, 0.5), 1.0])
    u1 = (P1 @ X)[:2] / (P1 @ X)[2] + rng.normal(0, noise_px, 2)
    u2 = (P2 @ X)[:2] / (P2 @ X)[2] + rng.normal(0, noise_px, 2)
    return _rows(P1, P2, u1, u2)


def inputs():
    from lichtfeld_densification_plugin_amd import synthetic
    cams = synthetic.ring_cameras(60, seed=0)
    rng = np.random.RandomState(SEED)
    A, kind = [], []

    def add(a, k):
        A.append(np.asarray(a, np.float32).reshape(4, 4)); kind.append(k)

    for _ in range(2000):
        add(_dlt(rng, cams, rng.choice([0.1, 0.5, 1.0, 2.0])), 0)
    for _ in range(300):
        add(_dlt(rng, cams, 0.0), 1)
    for _ in range(500):
        add(_dlt(rng, cams, rng.choice([10.0, 30.0, 60.0])), 2)
    for w in (1e-3, 1e-6, 1e-9, 1e-12, 1e-20, 0.0):
        for _ in range(20):
            d = rng.normal(size=3)
            d[2] = -abs(d[2]) * 0.2          # roughly along the ground, in front of most cameras
            add(_dlt(rng, cams, rng.choice([0.0, 0.3]), X=np.array([d[0], d[1], d[2], w])), 3)
    for ratio in (0.5, 0.9, 0.99, 0.999, 0.99999, 1.0):
        for _ in range(25):
            U, _ = np.linalg.qr(rng.normal(size=(4, 4)))
            V, _ = np.linalg.qr(rng.normal(size=(4, 4)))
            s3 = rng.uniform(0.1, 10.0)
            s = np.array([s3 * rng.uniform(50, 500), s3 * rng.uniform(2, 20), s3, s3 * ratio])
            add((U * s) @ V.T * rng.choice([1.0, 1e3]), 4)
    base = _dlt(rng, cams, 0.5)
    for pos in range(16):
        for val in (np.nan, np.inf, -np.inf):
            b = base.copy().reshape(16)
            b[pos] = val
            add(b, 5)
    for _ in range(20):
        b = _dlt(rng, cams, 0.5).reshape(16)
        b[rng.choice(16, 3, replace=False)] = rng.choice([np.nan, np.inf, -np.inf], 3)
        add(b, 5)
    add(np.full((4, 4), np.nan), 5)
    add(np.full((4, 4), np.inf), 5)
    add(np.zeros((4, 4)), 6)
    add(np.eye(4), 6)
    add(np.ones((4, 4)), 6)
    add(rng.randn(4, 4) * 1e18, 6)
    add(rng.randn(4, 4) * 1e-18, 6)
    add(rng.randn(4, 4) * 1e-30, 6)
    r2 = rng.randn(4, 4)
    r2[2], r2[3] = r2[0], r2[1]
    add(r2, 6)
    d = np.diag([3.0, 2.0, 1.0, 1.0])
    add(d, 6)
    add(np.diag([1.0, 1.0, 1.0, 0.0]), 6)
    add(np.diag([0.0, 1.0, 1.0, 1.0]), 6)
    return np.stack(A), np.asarray(kind, np.int8)


def rerecord(path):
    from lichtfeld_densification_plugin_amd.core import hip_backend as hb
    g = dict(np.load(path))
    A, c, it = g["A"], g["c"].copy(), g["it"].copy()
    changed = []
    for i in range(A.shape[0]):
        x, n = hb.host_null_vector(A[i])
        if n != int(it[i]) or x.tobytes() != c[i].tobytes():
            changed.append(i)
            c[i], it[i] = x, n
    idx = np.asarray(changed, np.int32)
    if "rerecorded" in g:          # records replaced before stay listed, with what they were at first
        keep = ~np.isin(g["rerecorded"], idx)
        first = {int(i): (cp, ip) for i, cp, ip in zip(g["rerecorded"], g["c_prev"], g["it_prev"])}
        idx = np.sort(np.concatenate([g["rerecorded"][keep], idx]).astype(np.int32))
        c_prev = np.stack([first[int(i)][0] if int(i) in first else g["c"][i] for i in idx])
        it_prev = np.asarray([first[int(i)][1] if int(i) in first else g["it"][i] for i in idx], np.int8)
    else:
        c_prev, it_prev = g["c"][idx], g["it"][idx]
    np.savez_compressed(path, A=A, kind=g["kind"], c=c, it=it, rerecorded=idx, c_prev=c_prev, it_prev=it_prev)
    print(path, "re-recorded", len(changed), "records:", changed)


def main():
    from lichtfeld_densification_plugin_amd.core import hip_backend as hb
    if "--rerecord" in sys.argv:
        return rerecord(os.path.join(HERE, "g13_null_vector.npz"))
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "g13_null_vector.npz")
    A, kind = inputs()
    c = np.empty((A.shape[0], 4), np.float64)
    it = np.empty(A.shape[0], np.int8)
    for i in range(A.shape[0]):
        c[i], it[i] = hb.host_null_vector(A[i])
    np.savez_compressed(out, A=A, kind=kind, c=c, it=it)
    print(out, A.shape[0], "matrices; solves:", dict(zip(*np.unique(it, return_counts=True))))
    for k in range(7):
        print("  kind", k, "solves", dict(zip(*np.unique(it[kind == k], return_counts=True))))


if __name__ == "__main__":
    main()
