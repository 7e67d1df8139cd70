"""CPU tier of the forward-backward gate's entry points (lfd_cycle_gate / lfd_cycle_gate_host): the library exports them, the header declares
them with the documented argument list, the binding types them, the ABI version is unchanged, and the argument checks that need no GPU answer
as the other entry points do (a null context: LFD_ERR_INVALID; a host context given to the device call: LFD_ERR_STATE - the reverse is
tests/test_gpu_cycle_gate.py's)."""
import ctypes as C
import os
import re

import pytest

from helpers import ROOT
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

LFD_ERR_INVALID, LFD_ERR_STATE = 1, 4
ARGS = ["lfd_context* ctx", "int32_t n_pairs", "const float* const* cert", "const float* const* warp_ab", "const float* const* warp_ba", "int32_t H",
        "int32_t W", "int32_t warp_channels", "int32_t Hb", "int32_t Wb", "const float* axis_x", "const float* axis_y", "int32_t w_match",
        "int32_t h_match", "float certainty_thresh", "float cycle_thresh_px", "float* const* cert_out", "float* const* err_out", "int32_t* rejected"]
NAMES = ["lfd_cycle_gate", "lfd_cycle_gate_host"]
NULL_CALL = (1, None, None, None, 1, 1, 2, 1, 1, None, None, 1, 1, 0.2, 1.0, None, None, None)


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
    hb.check_struct_layout(lib)                              # lfd_params / lfd_batch / lfd_points as the mirrors have them
    assert C.sizeof(hb.lfd_params) == 32


@pytest.mark.parametrize("name", NAMES)
def test_binding_sets_argtypes(lib, name):
    f = getattr(lib, name)
    assert f.restype is C.c_int
    assert f.argtypes is not None and len(f.argtypes) == len(ARGS)
    assert all(t is C.c_int32 for t in (f.argtypes[1],) + tuple(f.argtypes[5:10]) + tuple(f.argtypes[12:14]))
    assert f.argtypes[14] is C.c_float and f.argtypes[15] is C.c_float
    assert callable(getattr(hb.HipDensifier, "cycle_gate", None)) and callable(getattr(hb.HostDensifier, "cycle_gate", None))


@pytest.mark.parametrize("name", NAMES)
def test_null_context_is_invalid(lib, name):
    assert getattr(lib, name)(None, *NULL_CALL) == LFD_ERR_INVALID
    assert lib.lfd_last_error(None)


def test_host_context_is_refused_by_the_device_call(lib):
    ctx = C.c_void_p()
    assert lib.lfd_create_host(1, C.byref(ctx)) == 0 and ctx.value
    try:
        assert lib.lfd_cycle_gate(ctx, *NULL_CALL) == LFD_ERR_STATE
        assert b"host" in lib.lfd_last_error(ctx)
        assert lib.lfd_cycle_gate_host(ctx, *NULL_CALL) == LFD_ERR_INVALID                  # its own entry point looks at the arguments
        assert b"lfd_cycle_gate_host" in lib.lfd_last_error(ctx)
    finally:
        lib.lfd_destroy(ctx)
