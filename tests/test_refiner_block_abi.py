"""CPU tier of the refiner-block entry points (lfd_refiner_block / lfd_refiner_block_host): the library exports them, the header declares
them with the documented argument list, the binding types them, the ABI version is unchanged, and every argument check answers
LFD_ERR_INVALID with its message on a host context (the device context's answers: tests/test_gpu_refiner_block.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from helpers import ROOT
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

LFD_ERR_INVALID, LFD_ERR_STATE = 1, 4
NAMES = ["lfd_refiner_block", "lfd_refiner_block_host"]
ARGS = ["lfd_context* ctx", "const void* x", "int32_t x_is_f32", "int32_t B", "int32_t C", "int32_t H", "int32_t W", "const float* dw_w",
        "const float* scale", "const float* shift", "const float* pw_wT", "const float* pw_b", "uint16_t* out"]


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


def test_abi_version_is_unchanged(lib):
    assert lib.lfd_abi_version() == 9 == hb.LFD_ABI_VERSION
    header = open(os.path.join(ROOT, "include", "lfd_densify.h")).read()
    assert re.search(r"#define\s+LFD_ABI_VERSION\s+9\b", header)


@pytest.mark.parametrize("name", NAMES)
def test_binding_sets_argtypes(lib, name):
    f = getattr(lib, name)
    assert f.restype is C.c_int
    assert f.argtypes is not None and len(f.argtypes) == len(ARGS)
    assert all(t is C.c_int32 for t in f.argtypes[2:7])
    assert callable(getattr(hb.HipDensifier, "refiner_block", None)) and callable(getattr(hb.HostDensifier, "refiner_block", None))


@pytest.mark.parametrize("name", NAMES)
def test_null_context_is_invalid(lib, name):
    assert getattr(lib, name)(None, None, 0, 1, 1, 1, 1, None, None, None, None, None, None) == LFD_ERR_INVALID
    assert lib.lfd_last_error(None)


def invalid_calls(C_ch=32):
    """(what, arguments after the context, expected piece of the message) for every refusal; the buffers are large enough for B C H W <= 2048."""
    x = np.zeros(2048, np.float32)
    out = np.zeros(2048, np.uint16)
    f = np.zeros(1024, np.float32)
    keep = (x, out, f)
    px, po, pf = x.ctypes.data, out.ctypes.data, f.ctypes.data
    good = dict(x=px, f32=0, B=1, C=C_ch, H=4, W=5, w=pf, s=pf, t=pf, wt=pf, pb=pf, out=po)

    def call(**kw):
        a = dict(good, **kw)
        return (a["x"], a["f32"], a["B"], a["C"], a["H"], a["W"], a["w"], a["s"], a["t"], a["wt"], a["pb"], a["out"])

    cases = [("null x", call(x=None), "null pointer"), ("null dw_w", call(w=None), "null pointer"), ("null scale", call(s=None), "null pointer"),
             ("null shift", call(t=None), "null pointer"), ("null out", call(out=None), "null pointer"),
             ("pw_wT alone", call(pb=None), "both"), ("pw_b alone", call(wt=None), "both"),
             ("C != 32 with pointwise", call(C=31), "pointwise fusion implements C == 32 only"),
             ("B < 1", call(B=0), ">= 1"), ("C < 1", call(C=0, wt=None, pb=None), ">= 1"), ("H < 1", call(H=0), ">= 1"), ("W < 1", call(W=-3), ">= 1"),
             ("H too large", call(H=32769), "at most 32768"), ("W too large", call(W=40000), "at most 32768"),
             ("too many elements", call(B=2048, H=32768, W=32768), "2^31 - 1"),
             ("too many elements, no pointwise", call(B=65536, C=32768, H=1, W=1, wt=None, pb=None), "2^31 - 1"),
             ("out inside x (bf16)", call(out=px + 2 * 100), "overlaps"), ("out inside x (f32)", call(f32=1, out=px + 4 * 639), "overlaps"),
             ("x inside out", call(x=po + 2 * 639), "overlaps")]
    return keep, cases


def test_every_refusal_has_its_message_on_a_host_context(lib):
    ctx = C.c_void_p()
    assert lib.lfd_create_host(1, C.byref(ctx)) == 0 and ctx.value
    try:
        keep, cases = invalid_calls()
        assert lib.lfd_refiner_block(ctx, *cases[0][1]) == LFD_ERR_STATE            # the device call on a host context
        assert b"host" in lib.lfd_last_error(ctx)
        for what, args, piece in cases:
            assert lib.lfd_refiner_block_host(ctx, *args) == LFD_ERR_INVALID, what
            msg = lib.lfd_last_error(ctx).decode()
            assert msg.startswith("lfd_refiner_block_host: ") and piece in msg, (what, msg)
        # the last element of x may sit right in front of out: adjacent is not overlapping
        both = np.zeros(640 + 640, np.uint16)
        args = list(cases[0][1])                                                    # (its float arrays are alive in `keep`)
        args[0], args[-1] = both.ctypes.data, both.ctypes.data + 2 * 640
        assert lib.lfd_refiner_block_host(ctx, *args) == 0
    finally:
        lib.lfd_destroy(ctx)
