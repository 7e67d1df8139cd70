"""Point-cloud writers (upstream core/writers.py:15-46), byte-identical output, vectorised.

Upstream packs every point with ``struct.pack`` in a Python loop (0.25-0.38 M points/s); here a
structured NumPy array with the same field layout is written in one call."""
from __future__ import annotations

import os
from typing import Optional

import numpy as np

_PLY_REC = np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)])                       # 15 bytes
_PLY_NORMAL_REC = np.dtype([("xyz", "<f4", 3), ("normal", "<f4", 3), ("rgb", "u1", 3)])    # 27 bytes: experimental['estimate_normals']
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
