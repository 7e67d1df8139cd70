"""Point-cloud writers (upstream core/writers.py:15-46), byte-identical output, vectorised.

Upstream packs every point with ``struct.pack`` in a Python loop (0.25-0.38 M points/s); here a
structured NumPy array with the same field layout is written in one call."""
from __future__ import annotations

import os
from typing import Optional

import numpy as np

_PLY_REC = np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)])                       # 15 bytes
_PLY_NORMAL_REC = np.dtype([("xyz", "<f4", 3), ("normal", "<f4", 3), ("rgb", "u1", 3)])    # 27 bytes: experimental['estimate_normals']
_GAUSS_REC = np.dtype([("xyz", "<f4", 3), ("normal", "<f4", 3), ("f_dc", "<f4", 3), ("opacity", "<f4"), ("scale", "<f4", 3), ("rot", "<f4", 4)])    # 68 bytes: experimental['gaussian_init']
GAUSSIAN_PROPERTIES = ("x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2", "opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3")
_BIN_REC = np.dtype([("id", "<u8"), ("xyz", "<f8", 3), ("rgb", "u1", 3), ("err", "<f8")])   # 43 bytes


def ensure_dir(path: str) -> None:
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)


def ply_header(n: int, normals: bool = False) -> bytes:
    """``normals``: the vertex also carries nx ny nz (27-byte records); without it upstream's header, byte for byte."""
    return ("ply\nformat binary_little_endian 1.0\n"
            f"element vertex {int(n)}\n"
            "property float x\nproperty float y\nproperty float z\n"
            + ("property float nx\nproperty float ny\nproperty float nz\n" if normals else "") +
            "property uchar red\nproperty uchar green\nproperty uchar blue\n"
            "end_header\n").encode("ascii")


def ply_records(xyz: np.ndarray, rgb_uint8: np.ndarray, normals: Optional[np.ndarray] = None) -> np.ndarray:
    n = int(xyz.shape[0])
    rec = np.empty(n, dtype=_PLY_REC if normals is None else _PLY_NORMAL_REC)
    rec["xyz"] = np.asarray(xyz, dtype=np.float32).reshape(n, 3)
    if normals is not None:
        rec["normal"] = np.asarray(normals, dtype=np.float32).reshape(n, 3)
    rec["rgb"] = np.asarray(rgb_uint8, dtype=np.uint8).reshape(n, 3)
    return rec


def write_ply(path_out: str, xyz: np.ndarray, rgb_uint8: np.ndarray, normals: Optional[np.ndarray] = None) -> None:
    """Binary little-endian PLY: x y z (f32) [+ nx ny nz (f32)] + red green blue (u8)."""
    with open(path_out, "wb") as f:
        f.write(ply_header(xyz.shape[0], normals is not None))
        ply_records(xyz, rgb_uint8, normals).tofile(f)


def write_points3D_bin(path_out: str, xyz: np.ndarray, rgb_uint8: np.ndarray,
                       errors: Optional[np.ndarray] = None) -> None:
    """Upstream's COLMAP-like ``points3D.bin``: u64 count, then per point u64 id (1-based), xyz f64,
    rgb u8, error f64 - and no track-length field, exactly as upstream writes it."""
    n = int(xyz.shape[0])
    rec = np.empty(n, dtype=_BIN_REC)
    rec["id"] = np.arange(1, n + 1, dtype=np.uint64)
    rec["xyz"] = np.asarray(xyz).reshape(n, 3).astype(np.float64)
    rec["rgb"] = np.asarray(rgb_uint8, dtype=np.uint8).reshape(n, 3)
    rec["err"] = 0.0 if errors is None else np.asarray(errors).reshape(n).astype(np.float64)
    with open(path_out, "wb") as f:
        f.write(np.uint64(n).tobytes())
        rec.tofile(f)


_STREAM_COUNT_WIDTH = 12


def streamed_ply_header(n: int) -> bytes:
    """Upstream's PLY header with the vertex count in a FIXED width (PLY allows comment lines: one pads the count), so that the data offset
    does not depend on the count and the count can be patched in at the end.  What StreamedPlyWriter / SharedFilePlyStream write."""
    head = ply_header(0).decode("ascii")
    prefix = "ply\nformat binary_little_endian 1.0\n"
    rest = head.split("element vertex 0\n", 1)[1]
    count = str(int(n))
    pad = "x" * (_STREAM_COUNT_WIDTH - len(count))
    return (prefix + f"comment {pad}\n" + f"element vertex {count}\n" + rest).encode("ascii")


class StreamedPlyWriter:
    """Append survivor segments as they complete; the vertex count in the header is patched on close
    (the header is padded so its length does not depend on the count)."""

    _COUNT_WIDTH = _STREAM_COUNT_WIDTH

    def __init__(self, path_out: str):
        ensure_dir(path_out)
        self._f = open(path_out, "wb")
        self._n = 0
        self._f.write(self._header_bytes(0))

    def _header_bytes(self, n: int) -> bytes:
        return streamed_ply_header(n)

    def append(self, xyz: np.ndarray, rgb_uint8: np.ndarray) -> None:
        ply_records(xyz, rgb_uint8).tofile(self._f)
        self._n += int(xyz.shape[0])

    def append_packed(self, body: bytes) -> None:
        """15-byte records as the device packs them (HipDensifier.pack_ply)."""
        if len(body) % 15:
            raise ValueError("PLY body must be 15 bytes per vertex")
        self._f.write(body)
        self._n += len(body) // 15

    @property
    def count(self) -> int:
        return self._n

    def close(self) -> None:
        if self._f is None:
            return
        self._f.seek(0)
        self._f.write(self._header_bytes(self._n))
        self._f.close()
        self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def write_ply_packed(path_out: str, n: int, body: bytes, normals: bool = False) -> None:
    """PLY from a body packed on the device: header + n 15-byte records (HipDensifier.pack_ply), or - ``normals`` - n 27-byte records
    (HipDensifier.pack_ply_normals)."""
    size = 27 if normals else 15
    if len(body) != size * int(n):
        raise ValueError(f"PLY body must be {size} bytes per vertex")
    with open(path_out, "wb") as f:
        f.write(ply_header(n, normals))
        f.write(body)


def gaussian_ply_header(n: int) -> bytes:
    """The header of a 3DGS ``point_cloud.ply`` at SH degree 0 (no ``f_rest_*``): 17 float properties, 68 bytes a vertex."""
    return ("ply\nformat binary_little_endian 1.0\n"
            f"element vertex {int(n)}\n"
            + "".join(f"property float {name}\n" for name in GAUSSIAN_PROPERTIES) +
            "end_header\n").encode("ascii")


def gaussian_records(xyz: np.ndarray, normals: np.ndarray, rgb01: np.ndarray, dist2: np.ndarray, opacity: float = 0.1, flatten: float = 1.0,
                     max_scale: float = 0.0) -> np.ndarray:
    """The 68-byte records of lfd_pack_gaussians in NumPy, rounding for rounding (csrc/lfd_knn.hpp): the colour through the u8 the point file
    stores, the scale from max(dist2, 1e-7) - capped at max_scale^2 if that is > 0 - as an f64 log rounded once, the rotation taking +z onto the
    normal.  ``dist2``: the mean squared distance to the three nearest neighbours (HostDensifier.knn_dist2)."""
    import math
    n = int(np.asarray(xyz).shape[0])
    f32 = np.float32
    rec = np.empty(n, dtype=_GAUSS_REC)
    rec["xyz"] = np.asarray(xyz, dtype=f32).reshape(n, 3)
    nrm = np.asarray(normals, dtype=f32).reshape(n, 3)
    rec["normal"] = nrm
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        q = np.clip(np.nan_to_num(np.round(np.asarray(rgb01, dtype=f32).reshape(n, 3) * f32(255.0)), nan=0.0), 0, 255).astype(f32)
        rec["f_dc"] = ((q / f32(255.0)) - f32(0.5)) / f32(0.28209479177387814)
        rec["opacity"] = f32(math.log(float(opacity) / (1.0 - float(opacity))))
        m = np.maximum(np.asarray(dist2, dtype=f32).reshape(n), f32(1e-7))
        if float(max_scale) > 0.0:
            cap = f32(min(float(max_scale) * float(max_scale), 3.4028234663852886e38))
            m = np.minimum(m, cap if cap > 0 else f32(1.4012985e-45))
        ls = 0.5 * np.log(m.astype(np.float64))
        rec["scale"][:, 0] = rec["scale"][:, 1] = ls.astype(f32)
        rec["scale"][:, 2] = (ls + math.log(float(flatten))).astype(f32)
        rot = np.zeros((n, 4), f32)
        rot[:, 0] = 1.0
        usable = np.isfinite(nrm).all(1) & (nrm != 0).any(1)
        w, x, y = f32(1.0) + nrm[:, 2], -nrm[:, 1], nrm[:, 0]
        flip = usable & (w < f32(2.0 ** -23))
        rot[flip] = (0.0, 1.0, 0.0, 0.0)
        length = np.sqrt((w * w + x * x) + y * y)
        go = usable & ~flip & np.isfinite(length) & (length > 0)
        rot[go, 0], rot[go, 1], rot[go, 2] = (w / length)[go], (x / length)[go], (y / length)[go]
    rec["rot"] = rot
    return rec


def write_gaussian_ply_packed(path_out: str, n: int, body: bytes) -> None:
    """A 3DGS ``point_cloud.ply`` at SH degree 0 from n packed 68-byte records (HipDensifier / HostDensifier.pack_gaussians)."""
    if len(body) != 68 * int(n):
        raise ValueError("Gaussian PLY body must be 68 bytes per vertex")
    with open(path_out, "wb") as f:
        f.write(gaussian_ply_header(n))
        f.write(body)


def write_points3D_bin_packed(path_out: str, n: int, body: bytes) -> None:
    if len(body) != 43 * int(n):
        raise ValueError("points3D.bin body must be 43 bytes per point")
    with open(path_out, "wb") as f:
        f.write(np.uint64(n).tobytes())
        f.write(body)


class CumulativePlyBody:
    """The PLY body of everything emitted so far, kept as bytes: upstream re-concatenates, re-quantises and re-packs the WHOLE cloud
    for every intermediate preview (core/pipeline.py:508-532 there); here each reference's 15-byte records are packed once (on the
    device when the points are there) and a preview is header + the bytes so far."""

    def __init__(self) -> None:
        self._chunks = []
        self._n = 0

    def append_packed(self, body: bytes) -> None:
        if len(body) % 15:
            raise ValueError("PLY body must be 15 bytes per vertex")
        self._chunks.append(bytes(body))
        self._n += len(body) // 15

    def append(self, xyz: np.ndarray, rgb_uint8: np.ndarray) -> None:
        self.append_packed(ply_records(xyz, rgb_uint8).tobytes())

    @property
    def count(self) -> int:
        return self._n

    def snapshot(self, path_out: str) -> None:
        """A complete PLY of the points so far (what upstream's intermediate previews contain)."""
        with open(path_out, "wb") as f:
            f.write(ply_header(self._n))
            for c in self._chunks:
                f.write(c)
