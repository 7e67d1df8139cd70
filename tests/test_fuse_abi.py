"""CPU tier of the entry points of oriented voxel fusion (lfd_fuse_oriented / lfd_fuse_oriented_host): the library exports them, the header
declares them with the argument list of DESIGN.md 4.16, the binding types them, the ABI version and the pinned structures are unchanged, every
refusal of the contract answers LFD_ERR_INVALID with a message - the two data refusals in words the binding turns into FuseInputRefused -, a
context of the wrong kind is refused (a host context given to the device call: LFD_ERR_STATE; the reverse is tests/test_gpu_fuse.py's), and the
inputs are bitwise untouched."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from helpers import ROOT
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

LFD_ERR_INVALID, LFD_ERR_STATE = 1, 4
ARGS = ["lfd_context* ctx", "const float* xyz", "const float* normals", "const float* rgb", "int64_t n", "double voxel_size", "float* xyz_out",
        "float* normals_out", "float* rgb_out", "uint32_t* count_out", "int64_t* n_rows_host", "int64_t* n_voxels_host"]
NAMES = ["lfd_fuse_oriented", "lfd_fuse_oriented_host"]
NULL_CALL = (None, None, None, 0, 1.0, None, None, None, None, None, None)


@pytest.fixture(scope="module")
def lib():
    return hb.load_library()


@pytest.mark.parametrize("name", NAMES)
def test_library_exports_and_header_declares(lib, name):
    assert hasattr(lib, name)
    header = open(os.path.join(ROOT, "include", "lfd_densify.h")).read()
    decl = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert decl, f"{name} is not declared in include/lfd_densify.h"
    assert [" ".join(a.split()) for a in decl.group(1).split(",")] == ARGS


def test_abi_version_and_struct_layouts_are_unchanged(lib):
    assert lib.lfd_abi_version() == 9 == hb.LFD_ABI_VERSION
    hb.check_struct_layout(lib)
    assert C.sizeof(hb.lfd_params) == 32 and C.sizeof(hb.lfd_points) == 48 and C.sizeof(hb.lfd_batch) == 120


@pytest.mark.parametrize("name", NAMES)
def test_binding_sets_argtypes(lib, name):
    f = getattr(lib, name)
    assert f.restype is C.c_int
    assert f.argtypes is not None and len(f.argtypes) == len(ARGS)
    assert [i for i, t in enumerate(f.argtypes) if t is C.c_double] == [5] and [i for i, t in enumerate(f.argtypes) if t is C.c_int64] == [4]
    for cls in (hb.HipDensifier, hb.HostDensifier):
        sig = inspect.signature(cls.fuse_oriented).parameters
        assert list(sig)[1:] == ["xyz", "normals", "rgb", "voxel_size", "with_counts"] and sig["with_counts"].default is False
    assert issubclass(hb.FuseInputRefused, hb.HipBackendError)


@pytest.mark.parametrize("name", NAMES)
def test_null_context_is_invalid(lib, name):
    assert getattr(lib, name)(None, *NULL_CALL) == LFD_ERR_INVALID
    assert lib.lfd_last_error(None)


def test_host_context_is_refused_by_the_device_call(lib):
    ctx = C.c_void_p()
    assert lib.lfd_create_host(1, C.byref(ctx)) == 0 and ctx.value
    try:
        assert lib.lfd_fuse_oriented(ctx, *NULL_CALL) == LFD_ERR_STATE
        assert b"host" in lib.lfd_last_error(ctx)
        assert lib.lfd_fuse_oriented_host(ctx, *NULL_CALL) == LFD_ERR_INVALID               # its own entry point looks at the arguments
        assert b"lfd_fuse_oriented_host" in lib.lfd_last_error(ctx)
    finally:
        lib.lfd_destroy(ctx)


def test_every_refusal_of_the_contract(lib):
    twin = hb.HostDensifier(1)
    try:
        rng = np.random.default_rng(0)
        n = 300
        xyz = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
        nrm = rng.normal(size=(n, 3)).astype(np.float32)
        rgb = rng.uniform(0, 1, (n, 3)).astype(np.float32)
        xo, no, ro = np.zeros_like(xyz), np.zeros_like(xyz), np.zeros_like(xyz)
        cnt = np.zeros(n, np.uint32)
        n_rows, n_vox = C.c_int64(-1), C.c_int64(-1)
        p = lambda a: a.ctypes.data                                         # noqa: E731
        good = dict(xyz=p(xyz), nrm=p(nrm), rgb=p(rgb), n=n, h=0.3, xo=p(xo), no=p(no), ro=p(ro), cnt=p(cnt), n_rows=C.byref(n_rows),
                    n_vox=C.byref(n_vox))

        def call(**kw):
            a = {**good, **kw}
            return lib.lfd_fuse_oriented_host(twin._ctx, a["xyz"], a["nrm"], a["rgb"], a["n"], C.c_double(a["h"]), a["xo"], a["no"], a["ro"], a["cnt"],
                                              a["n_rows"], a["n_vox"])

        before = [a.copy() for a in (xyz, nrm, rgb)]
        assert call() == 0 and 0 < n_vox.value <= n_rows.value <= min(n, 2 * n_vox.value)
        assert int(cnt[:n_rows.value].sum()) == n
        for a, b in zip((xyz, nrm, rgb), before):
            assert a.tobytes() == b.tobytes()                                # the inputs are read only
        assert call(cnt=None) == 0                                           # the optional array
        assert call(n=0, xyz=None, nrm=None, rgb=None, xo=None, no=None, ro=None, cnt=None) == 0 and n_rows.value == 0 and n_vox.value == 0
        invalid = [dict(xyz=None), dict(nrm=None), dict(rgb=None), dict(xo=None), dict(no=None), dict(ro=None), dict(n_rows=None), dict(n_vox=None),
                   dict(n=-1), dict(n=1 << 31),
                   dict(h=0.0), dict(h=-0.5), dict(h=float("inf")), dict(h=float("nan")),
                   dict(xo=p(xyz)), dict(xo=p(xyz) + 12 * (n - 1)), dict(no=p(nrm)), dict(ro=p(rgb)), dict(xo=p(nrm)), dict(no=p(rgb)), dict(cnt=p(xyz)),
                   dict(cnt=p(rgb) + 4), dict(no=p(xo)), dict(ro=p(xo) + 12), dict(ro=p(no)), dict(cnt=p(xo)), dict(cnt=p(ro) + 12 * n - 4)]
        for kw in invalid:
            assert call(**kw) == LFD_ERR_INVALID, kw
            msg = lib.lfd_last_error(twin._ctx)
            assert msg.startswith(b"lfd_fuse_oriented_host: "), kw
            assert b"key range" not in msg and b"non-finite coordinate" not in msg
        # the two data refusals, decided before anything is sorted, in words of their own
        for value in (np.nan, np.inf, -np.inf):
            bad = xyz.copy()
            bad[17, 2] = value
            assert call(xyz=p(bad)) == LFD_ERR_INVALID and b"non-finite coordinate" in lib.lfd_last_error(twin._ctx)
        wide = (xyz * np.float32(1e30)).astype(np.float32)
        assert call(xyz=p(wide), h=1e-30) == LFD_ERR_INVALID and b"key range" in lib.lfd_last_error(twin._ctx)
        line = np.zeros((n, 3), np.float32)
        line[:, 0] = np.linspace(0.0, 3.0e38, n)                             # one axis alone: more than 2^63 voxels along it
        assert call(xyz=p(line), h=1e-3) == LFD_ERR_INVALID and b"key range" in lib.lfd_last_error(twin._ctx)
        assert call() == 0                                                   # and the context still works
    finally:
        twin.close()
