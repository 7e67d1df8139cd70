"""The writers with normals (core/writers.py): a 27-byte-vertex PLY against a struct.pack loop, the no-normals path byte-identical to what it
was, the packed writer, and the empty cloud."""
import os
import struct

import numpy as np
import pytest

from lichtfeld_densification_plugin_amd.core import writers

OLD_HEADER = ("ply\nformat binary_little_endian 1.0\nelement vertex {n}\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
NEW_HEADER = ("ply\nformat binary_little_endian 1.0\nelement vertex {n}\nproperty float x\nproperty float y\nproperty float z\n"
              "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")


def cloud(n, seed=0):
    rng = np.random.RandomState(seed)
    xyz = rng.uniform(-4, 4, (n, 3)).astype(np.float32)
    nrm = rng.standard_normal((n, 3))
    nrm = (nrm / np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-9)).astype(np.float32)
    rgb = rng.randint(0, 256, (n, 3)).astype(np.uint8)
    return xyz, nrm, rgb


@pytest.mark.parametrize("n", [0, 1, 257])
def test_a_file_with_normals_against_a_struct_pack_loop(tmp_path, n):
    xyz, nrm, rgb = cloud(n)
    path = os.path.join(str(tmp_path), "n.ply")
    writers.write_ply(path, xyz, rgb, nrm)
    want = NEW_HEADER.format(n=n).encode("ascii")
    for i in range(n):
        want += struct.pack("<ffffffBBB", *[float(v) for v in xyz[i]], *[float(v) for v in nrm[i]], *[int(v) for v in rgb[i]])
    assert open(path, "rb").read() == want
    assert writers.ply_header(n, True) == NEW_HEADER.format(n=n).encode("ascii")
    rec = writers.ply_records(xyz, rgb, normals=nrm)
    assert rec.dtype.itemsize == 27 and rec.tobytes() == want[len(NEW_HEADER.format(n=n)):]
    packed = os.path.join(str(tmp_path), "p.ply")
    writers.write_ply_packed(packed, n, rec.tobytes(), normals=True)
    assert open(packed, "rb").read() == want
    with pytest.raises(ValueError, match="27 bytes per vertex"):
        writers.write_ply_packed(packed, n + 1, rec.tobytes(), normals=True)


@pytest.mark.parametrize("n", [0, 1, 257])
def test_without_normals_every_byte_stays_as_it_was(tmp_path, n):
    xyz, _nrm, rgb = cloud(n, 1)
    path = os.path.join(str(tmp_path), "o.ply")
    writers.write_ply(path, xyz, rgb)
    want = OLD_HEADER.format(n=n).encode("ascii")
    for i in range(n):
        want += struct.pack("<fffBBB", *[float(v) for v in xyz[i]], *[int(v) for v in rgb[i]])
    assert open(path, "rb").read() == want
    assert writers.ply_header(n) == writers.ply_header(n, False) == OLD_HEADER.format(n=n).encode("ascii")
    rec = writers.ply_records(xyz, rgb)
    assert rec.dtype.itemsize == 15
    writers.write_ply(path, xyz, rgb, None)
    assert open(path, "rb").read() == want
    packed = os.path.join(str(tmp_path), "p.ply")
    writers.write_ply_packed(packed, n, rec.tobytes())
    assert open(packed, "rb").read() == want
    with pytest.raises(ValueError, match="15 bytes per vertex"):
        writers.write_ply_packed(packed, n + 1, rec.tobytes())
    # the intermediate previews and the streamed writer keep their 15-byte records
    body = writers.CumulativePlyBody()
    body.append(xyz, rgb)
    body.snapshot(packed)
    assert open(packed, "rb").read() == want
