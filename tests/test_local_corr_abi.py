"""CPU tier of the local-correlation entry points (lfd_local_corr / lfd_local_corr_host): the library exports them, the header declares them
with the documented argument list, the binding types them, and the argument checks that need no GPU answer as the other entry points do (a
null context: LFD_ERR_INVALID; a host context given to the device call, or the reverse: LFD_ERR_STATE)."""
import ctypes as C
import os
import re

import pytest

from helpers import ROOT
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

LFD_ERR_INVALID, LFD_ERR_STATE = 1, 4
ARGS = ["lfd_context* ctx", "const float* A", "const float* Bf", "const float* warp", "int32_t B", "int32_t N", "int32_t C", "int32_t K",
        "int32_t H1", "int32_t W1", "const int64_t* a_strides", "const int64_t* bf_strides", "float* out"]


@pytest.fixture(scope="module")
def lib():
    return hb.load_library()


@pytest.mark.parametrize("name", ["lfd_local_corr", "lfd_local_corr_host"])
def test_library_exports_and_header_declares(lib, name):
    assert hasattr(lib, name)
    header = open(os.path.join(ROOT, "include", "lfd_densify.h")).read()
    decl = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert decl, f"{name} is not declared in include/lfd_densify.h"
    assert [" ".join(a.split()) for a in decl.group(1).split(",")] == ARGS


def test_abi_version_is_unchanged(lib):
    assert lib.lfd_abi_version() == 9 == hb.LFD_ABI_VERSION


@pytest.mark.parametrize("name", ["lfd_local_corr", "lfd_local_corr_host"])
def test_binding_sets_argtypes(lib, name):
    f = getattr(lib, name)
    assert f.restype is C.c_int
    assert f.argtypes is not None and len(f.argtypes) == len(ARGS)
    assert all(t is C.c_int32 for t in f.argtypes[4:10])
    assert f.argtypes[10] is C.POINTER(C.c_int64) and f.argtypes[11] is C.POINTER(C.c_int64)
    assert callable(getattr(hb.HipDensifier, "local_corr", None)) and callable(getattr(hb.HostDensifier, "local_corr", None))


@pytest.mark.parametrize("name", ["lfd_local_corr", "lfd_local_corr_host"])
def test_null_context_is_invalid(lib, name):
    rc = getattr(lib, name)(None, None, None, None, 1, 1, 1, 1, 1, 1, None, None, None)
    assert rc == LFD_ERR_INVALID
    assert lib.lfd_last_error(None)


def test_host_context_is_refused_by_the_device_call_and_bad_arguments_by_the_twin(lib):
    ctx = C.c_void_p()
    assert lib.lfd_create_host(1, C.byref(ctx)) == 0 and ctx.value
    try:
        assert lib.lfd_local_corr(ctx, None, None, None, 1, 1, 1, 1, 1, 1, None, None, None) == LFD_ERR_STATE
        assert b"host" in lib.lfd_last_error(ctx)
        assert lib.lfd_local_corr_host(ctx, None, None, None, 1, 1, 1, 1, 1, 1, None, None, None) == LFD_ERR_INVALID       # null pointers
        assert b"lfd_local_corr_host" in lib.lfd_last_error(ctx)
        assert lib.lfd_local_corr_host(ctx, None, None, None, 1, 1, 0, 1, 1, 1, None, None, None) == LFD_ERR_INVALID       # C = 0
        assert lib.lfd_local_corr_host(ctx, None, None, None, 1, 1, 4, 1, 40000, 1, None, None, None) == LFD_ERR_INVALID   # H1 too large
        assert lib.lfd_local_corr_host(ctx, None, None, None, 0, 5, 4, 1, 3, 3, None, None, None) == 0                     # nothing to do
    finally:
        lib.lfd_destroy(ctx)
