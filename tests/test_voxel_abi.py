"""CPU tier of the device distance filter (lfd_voxel_downsample): the library exports it, the header declares it, the binding types it, and the
argument checks that need no GPU answer as the other device entry points do (a null context: LFD_ERR_INVALID, a host context: LFD_ERR_STATE)."""
import ctypes as C
import os
import re

import pytest

from helpers import ROOT
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

LFD_ERR_INVALID, LFD_ERR_STATE = 1, 4


@pytest.fixture(scope="module")
def lib():
    return hb.load_library()


def test_library_exports_lfd_voxel_downsample(lib):
    assert hasattr(lib, "lfd_voxel_downsample")


def test_header_declares_lfd_voxel_downsample():
    header = open(os.path.join(ROOT, "include", "lfd_densify.h")).read()
    decl = re.search(r"int\s+lfd_voxel_downsample\s*\(([^)]*)\)\s*;", header)
    assert decl, "lfd_voxel_downsample is not declared in include/lfd_densify.h"
    args = [" ".join(a.split()) for a in decl.group(1).split(",")]
    assert args == ["lfd_context* ctx", "const float* xyz", "const float* rgb", "int64_t n", "double voxel_size", "float* xyz_out",
                    "float* rgb_out", "int64_t* n_out_host"]


def test_binding_sets_argtypes(lib):
    f = lib.lfd_voxel_downsample
    assert f.restype is C.c_int
    assert f.argtypes is not None and len(f.argtypes) == 8
    assert f.argtypes[3] is C.c_int64 and f.argtypes[4] is C.c_double
    assert f.argtypes[7] is C.POINTER(C.c_int64)
    assert issubclass(hb.VoxelInputRefused, hb.HipBackendError)
    assert callable(getattr(hb.HipDensifier, "voxel_downsample", None))


def test_null_context_is_invalid(lib):
    n_out = C.c_int64(-1)
    rc = lib.lfd_voxel_downsample(None, None, None, 0, 0.01, None, None, C.byref(n_out))
    assert rc == LFD_ERR_INVALID
    assert lib.lfd_last_error(None)


def test_host_context_is_refused_with_state(lib):
    ctx = C.c_void_p()
    assert lib.lfd_create_host(1, C.byref(ctx)) == 0 and ctx.value
    try:
        n_out = C.c_int64(-1)
        rc = lib.lfd_voxel_downsample(ctx, None, None, 0, 0.01, None, None, C.byref(n_out))
        assert rc == LFD_ERR_STATE
        assert b"host" in lib.lfd_last_error(ctx)
    finally:
        lib.lfd_destroy(ctx)
