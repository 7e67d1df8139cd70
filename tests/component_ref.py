"""Brute-force reference of the connected-component filter (lfd_component_filter), plain NumPy and Python: every pair of points
through the f32 link test of the contract - dx, dy, dz, d2 = (dx dx + dy dy) + dz dz, r2 = radius radius, d2 <= r2, one rounding per operation,
written here as csrc/lfd_consensus.hpp writes it - then a Python union-find over the edge list, and from the partition the sizes, the labels
(smallest input index of a component), the keep mask and the 66 summary words.  No grid and no sort: what the library finds through its sorted
cells has to equal this exactly.  For clouds of at most a few thousand points (the pair test is done in row blocks of a bounded size)."""
import numpy as np

SUMMARY_WORDS = 66
BINS = 32


def ref_ids(ref_counts) -> np.ndarray:
    counts = np.asarray(ref_counts, np.int64)
    return np.repeat(np.arange(counts.size, dtype=np.int64), counts)


def link_rows(p, rows, r2) -> np.ndarray:
    """(len(rows), n) bool: the f32 link test of the points `rows` against every point"""
    with np.errstate(all="ignore"):
        dx = p[rows, None, 0] - p[None, :, 0]
        dy = p[rows, None, 1] - p[None, :, 1]
        dz = p[rows, None, 2] - p[None, :, 2]
        sx, sy, sz = dx * dx, dy * dy, dz * dz
        sxy = sx + sy
        d2 = sxy + sz
        assert d2.dtype == np.float32
        return d2 <= r2                        # a NaN anywhere rejects; inf - inf is a NaN


def edge_blocks(xyz, radius):
    """every linked pair i < j, as (m, 2) int64 arrays, one per block of rows"""
    p = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = p.shape[0]
    r2 = np.float32(radius) * np.float32(radius)
    fin = np.isfinite(p).all(axis=1)
    block = max(1, (1 << 18) // max(n, 1))     # small blocks: partition() contracts the edges between them
    for a in range(0, n, block):
        rows = np.arange(a, min(n, a + block))
        ok = link_rows(p, rows, r2) & fin[rows, None] & fin[None, :]
        i, j = np.nonzero(ok)
        i = i + a
        m = i < j
        yield np.stack([i[m], j[m]], 1)


def edges(xyz, radius) -> np.ndarray:
    """(m, 2) int64: every linked pair i < j"""
    out = list(edge_blocks(xyz, radius))
    return np.concatenate(out) if out else np.zeros((0, 2), np.int64)


def partition(n, blocks) -> np.ndarray:
    """A representative of every point's class after uniting the two ends of every edge of every block.  The union-find is plain Python: the
    smaller index becomes the parent, finds halve their path.  A cloud in one cell has millions of edges, nearly all inside a set that is
    already one, so between blocks the edges are first mapped to the roots found so far and the pairs that are already joined, or repeat,
    are dropped - uniting two roots is uniting their sets."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    root = np.arange(n, dtype=np.int64)
    for e in blocks:
        e = np.asarray(e, np.int64).reshape(-1, 2)
        a, b = root[e[:, 0]], root[e[:, 1]]
        pairs = np.unique(np.stack([a, b], 1)[a != b], axis=0)
        for i, j in pairs.tolist():
            ri, rj = find(i), find(j)
            if ri != rj:
                parent[max(ri, rj)] = min(ri, rj)
        root = np.array([find(x) for x in range(n)], np.int64)
    return root


def components(xyz, radius):
    """(size, label) of every point, uint32 each"""
    n = int(np.asarray(xyz).reshape(-1, 3).shape[0])
    root = partition(n, edge_blocks(xyz, radius))
    size = np.bincount(root, minlength=max(n, 1))[root] if n else np.zeros(0, np.int64)
    label = np.full(max(n, 1), n, np.int64)
    np.minimum.at(label, root, np.arange(n))
    return size.astype(np.uint32), (label[root] if n else np.zeros(0, np.int64)).astype(np.uint32)


def summary(size, label) -> np.ndarray:
    """the 66 words: n_components, largest size, per b the components with 2^b <= size < 2^(b + 1), per b their points"""
    out = np.zeros(SUMMARY_WORDS, np.int64)
    size = np.asarray(size, np.int64)
    heads = np.asarray(label, np.int64) == np.arange(size.size)          # one point per component: the one the label names
    s = size[heads]
    out[0] = s.size
    out[1] = s.max() if s.size else 0
    for v in s.tolist():
        b = int(v).bit_length() - 1
        out[2 + b] += 1
        out[2 + BINS + b] += v
    return out


def filter_cloud(xyz, ref_counts, radius, min_points):
    """(keep mask, size, label, kept counts per reference, summary)"""
    size, label = components(xyz, radius)
    keep = size >= min_points
    ids = ref_ids(ref_counts)
    return keep, size, label, np.bincount(ids[keep], minlength=len(ref_counts)).astype(np.int64), summary(size, label)
