"""CPU tier of the entry points of the spatial point cap (lfd_cap_spatial and its *_host twin): the library exports them, the header declares them
with the argument list of DESIGN.md 4.19, the binding types them, the ABI version - in the header and in the library - and the pinned structures
are unchanged, the argument checks answer on both kinds of context before anything else is looked at, and each side refuses the other's context
(a host context given to the device call: LFD_ERR_STATE; the reverse is tests/test_gpu_cap.py's)."""
import ctypes as C
import inspect
import os
import re

import pytest

from helpers import ROOT
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

LFD_ERR_INVALID, LFD_ERR_STATE = 1, 4
CAP_ARGS = ["lfd_context* ctx", "const float* xyz", "const float* err", "int64_t n", "int64_t budget", "int64_t* keep_out", "int64_t* n_keep_host",
            "double* stats_host"]
NAMES = ["lfd_cap_spatial", "lfd_cap_spatial_host"]


@pytest.fixture(scope="module")
def lib():
    return hb.load_library()


@pytest.mark.parametrize("name", NAMES)
def test_library_exports_and_header_declares(lib, name):
    assert hasattr(lib, name)
    header = open(os.path.join(ROOT, "include", "lfd_densify.h")).read()
    decl = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert decl, f"{name} is not declared in include/lfd_densify.h"
    assert [" ".join(a.split()) for a in decl.group(1).split(",")] == CAP_ARGS


def test_abi_version_and_struct_layouts_are_unchanged(lib):
    header = open(os.path.join(ROOT, "include", "lfd_densify.h")).read()
    assert re.search(r"#define\s+LFD_ABI_VERSION\s+9\b", header)
    assert lib.lfd_abi_version() == 9 == hb.LFD_ABI_VERSION
    hb.check_struct_layout(lib)
    assert C.sizeof(hb.lfd_params) == 32 and C.sizeof(hb.lfd_points) == 48 and C.sizeof(hb.lfd_batch) == 120


@pytest.mark.parametrize("name", NAMES)
def test_binding_sets_argtypes(lib, name):
    f = getattr(lib, name)
    assert f.restype is C.c_int
    assert f.argtypes is not None and len(f.argtypes) == len(CAP_ARGS)
    assert [i for i, t in enumerate(f.argtypes) if t is C.c_int64] == [3, 4]
    for cls in (hb.HipDensifier, hb.HostDensifier):
        assert list(inspect.signature(cls.cap_spatial).parameters)[1:] == ["xyz", "err", "budget"]
    assert issubclass(hb.CapInputRefused, hb.HipBackendError)


@pytest.mark.parametrize("name", NAMES)
def test_null_context_is_invalid(lib, name):
    n_keep = C.c_int64(0)
    assert getattr(lib, name)(None, None, None, 0, 1, None, C.byref(n_keep), None) == LFD_ERR_INVALID
    assert lib.lfd_last_error(None)


def test_the_other_kind_of_context_and_the_argument_checks(lib):
    ctx = C.c_void_p()
    assert lib.lfd_create_host(1, C.byref(ctx)) == 0 and ctx.value
    try:
        n_keep = C.c_int64(7)
        assert lib.lfd_cap_spatial(ctx, None, None, 0, 1, None, C.byref(n_keep), None) == LFD_ERR_STATE and b"host" in lib.lfd_last_error(ctx)
        assert lib.lfd_cap_spatial(ctx, None, None, -1, 0, None, None, None) == LFD_ERR_STATE          # the context's kind is looked at first
        assert lib.lfd_cap_spatial_host(ctx, None, None, 0, 1, None, C.byref(n_keep), None) == 0 and n_keep.value == 0      # n == 0 is valid
        for args, words in (((None, None, 5, 1, None, C.byref(n_keep), None), b"null xyz / keep_out"),
                            ((None, None, 0, 0, None, C.byref(n_keep), None), b"budget must be >= 1"),
                            ((None, None, -1, 1, None, C.byref(n_keep), None), b"n must be in [0, 2^31 - 1]"),
                            ((None, None, 1 << 31, 1, None, C.byref(n_keep), None), b"n must be in [0, 2^31 - 1]"),
                            ((None, None, 0, 1, None, None, None), b"null n_keep_host")):
            assert lib.lfd_cap_spatial_host(ctx, *args) == LFD_ERR_INVALID, args
            assert lib.lfd_last_error(ctx) == b"lfd_cap_spatial_host: " + words
    finally:
        lib.lfd_destroy(ctx)
