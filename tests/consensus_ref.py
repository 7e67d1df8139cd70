"""Brute-force NumPy reference of the cross-reference consensus filter (lfd_consensus_filter): every pair of points through the
f32 test of the contract - dx, dy, dz, d2 = (dx dx + dy dy) + dz dz, r2 = radius radius, d2 <= r2, one rounding per operation - then the number of
DISTINCT other references that own an agreeing point, capped at LFD_CONSENSUS_CAP.  No grid: what the library finds through its sorted cells has
to equal this exactly."""
import numpy as np

CAP = 8


def ref_ids(ref_counts) -> np.ndarray:
    counts = np.asarray(ref_counts, np.int64)
    return np.repeat(np.arange(counts.size, dtype=np.int64), counts)


def agree_matrix(xyz, radius) -> np.ndarray:
    """(n, n) bool: the f32 agreement test for every pair (rows of a non-finite point and its column are False)"""
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    r2 = np.float32(radius) * np.float32(radius)
    with np.errstate(all="ignore"):
        dx = p[:, None, 0] - p[None, :, 0]
        dy = p[:, None, 1] - p[None, :, 1]
        dz = p[:, None, 2] - p[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == np.float32
        ok = d2 <= r2
    fin = np.isfinite(p).all(axis=1)
    return ok & fin[:, None] & fin[None, :]


def consensus(xyz, ref_counts, radius) -> np.ndarray:
    """c_i (uint8) of every point"""
    ids = ref_ids(ref_counts)
    n_refs = len(ref_counts)
    ok = agree_matrix(xyz, radius)
    onehot = np.zeros((ids.size, n_refs), np.float32)
    onehot[np.arange(ids.size), ids] = 1.0
    vouch = (ok.astype(np.float32) @ onehot) > 0          # (n, n_refs): reference g owns a point agreeing with i
    vouch[np.arange(ids.size), ids] = False
    return np.minimum(vouch.sum(axis=1), CAP).astype(np.uint8)


def filter_cloud(xyz, rgb, err, ref_counts, radius, min_refs):
    """(keep mask, c, kept counts per reference)"""
    c = consensus(xyz, ref_counts, radius)
    keep = c >= min_refs
    ids = ref_ids(ref_counts)
    return keep, c, np.bincount(ids[keep], minlength=len(ref_counts)).astype(np.int64)
