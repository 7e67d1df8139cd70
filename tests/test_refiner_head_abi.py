"""CPU tier of the refiner-head entry points (lfd_refiner_head / lfd_refiner_head_host): the library exports them, the header declares them
with the documented argument list, the binding types them and has the documented signatures, the ABI version is unchanged, and every argument
check answers LFD_ERR_INVALID with its message on a host context (the device context's answers: tests/test_gpu_refiner_head.py)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from helpers import ROOT
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

LFD_ERR_INVALID, LFD_ERR_STATE = 1, 4
NAMES = ["lfd_refiner_head", "lfd_refiner_head_host"]
ARGS = ["lfd_context* ctx", "const void* z", "int32_t z_is_f32", "int32_t B", "int32_t C", "int32_t H", "int32_t W", "const float* head_w",
        "const float* head_b", "const float* prev_warp", "const int64_t* prev_warp_strides", "const float* prev_conf",
        "const int64_t* prev_conf_strides", "int32_t prev_dim", "float refine_init", "float* warp", "float* conf"]


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
    assert "lfd_refiner_head_host" in re.search(r"\*_host calls \(([^)]*)\)", header).group(1)       # the CPU-twin comment lists it


def test_abi_version_is_unchanged(lib):
    assert lib.lfd_abi_version() == 9 == hb.LFD_ABI_VERSION
    header = open(os.path.join(ROOT, "include", "lfd_densify.h")).read()
    assert re.search(r"#define\s+LFD_ABI_VERSION\s+9\b", header)


@pytest.mark.parametrize("name", NAMES)
def test_binding_sets_argtypes(lib, name):
    f = getattr(lib, name)
    assert f.restype is C.c_int
    assert f.argtypes is not None and len(f.argtypes) == len(ARGS)
    assert all(t is C.c_int32 for t in f.argtypes[2:7]) and f.argtypes[13] is C.c_int32 and f.argtypes[14] is C.c_float
    assert f.argtypes[10] is f.argtypes[12] and f.argtypes[10] is C.POINTER(C.c_int64)


@pytest.mark.parametrize("cls", [hb.HipDensifier, hb.HostDensifier])
def test_python_signatures(cls):
    sig = inspect.signature(cls.refiner_head)
    assert list(sig.parameters) == ["self", "z", "head_w", "head_b", "prev_warp", "prev_conf", "refine_init"]
    assert sig.parameters["prev_conf"].default is None and sig.parameters["refine_init"].default == 4.0


@pytest.mark.parametrize("name", NAMES)
def test_null_context_is_invalid(lib, name):
    assert getattr(lib, name)(None, None, 0, 1, 1, 1, 1, None, None, None, None, None, None, 0, 4.0, None, None) == LFD_ERR_INVALID
    assert lib.lfd_last_error(None)


def strides(*v):
    return (C.c_int64 * 4)(*v)


def invalid_calls():
    """(what, arguments after the context, expected piece of the message) for every refusal; B C H W = 1 x 8 x 4 x 5 unless changed."""
    z = np.zeros(2048, np.float32)
    f = np.zeros(1024, np.float32)
    prev = np.zeros(1024, np.float32)
    warp, conf = np.zeros(256, np.float32), np.zeros(256, np.float32)
    keep = (z, f, prev, warp, conf)
    pz, pf, pp, pw, pc = (a.ctypes.data for a in keep)
    good = dict(z=pz, f32=0, B=1, C=8, H=4, W=5, w=pf, b=pf + 4 * 512, pw=pp, sw=None, pc=pp + 4 * 512, sc=None, pd=4, ri=4.0, warp=pw, conf=pc)

    def call(**kw):
        a = dict(good, **kw)
        return (a["z"], a["f32"], a["B"], a["C"], a["H"], a["W"], a["w"], a["b"], a["pw"], a["sw"], a["pc"], a["sc"], a["pd"], a["ri"], a["warp"], a["conf"])

    cases = [("null z", call(z=None), "null pointer"), ("null head_w", call(w=None), "null pointer"), ("null head_b", call(b=None), "null pointer"),
             ("null prev_warp", call(pw=None), "null pointer"), ("null warp", call(warp=None), "null pointer"), ("null conf", call(conf=None), "null pointer"),
             ("prev_dim 2", call(pd=2), "prev_dim must be 0, 1 or 4"), ("prev_dim -1", call(pd=-1), "prev_dim must be 0, 1 or 4"),
             ("prev_conf with prev_dim 0", call(pd=0), "prev_conf must be given with prev_dim 1 or 4 and null with prev_dim 0"),
             ("prev_dim 4 without prev_conf", call(pc=None), "prev_conf must be given"), ("prev_dim 1 without prev_conf", call(pc=None, pd=1), "prev_conf must be given"),
             ("B < 1", call(B=0), ">= 1"), ("C < 1", call(C=0), ">= 1"), ("H < 1", call(H=0), ">= 1"), ("W < 1", call(W=-3), ">= 1"),
             ("H too large", call(H=32769), "at most 32768"), ("W too large", call(W=40000), "at most 32768"),
             ("too many elements", call(B=2048, C=1, H=32768, W=32768), "2^31 - 1"), ("too many planes", call(B=65536, C=32768, H=1, W=1), "2^31 - 1"),
             ("negative warp stride", call(sw=strides(40, 10, -2, 1)), "negative stride"),
             ("negative conf stride", call(sc=strides(80, 20, 4, -1)), "negative stride"),
             ("refine_init 0", call(ri=0.0), "refine_init must be finite and > 0"), ("refine_init < 0", call(ri=-4.0), "refine_init"),
             ("refine_init inf", call(ri=float("inf")), "refine_init"), ("refine_init nan", call(ri=float("nan")), "refine_init"),
             ("warp overlaps conf", call(conf=pw + 4 * 39), "warp overlaps conf"),
             ("warp inside z", call(warp=pz + 2 * 100), "an output overlaps z"), ("conf inside z (f32)", call(f32=1, conf=pz + 4 * 159), "an output overlaps z"),
             ("warp inside head_w", call(warp=pf + 4 * 47), "an output overlaps head_w"), ("conf is head_b", call(conf=pf + 4 * 512), "an output overlaps head_b"),
             ("warp inside prev_warp", call(warp=pp + 4 * 39), "an output overlaps prev_warp"),
             ("conf inside strided prev_warp", call(sw=strides(40, 5, 1, 20), conf=pp + 4 * 39), "an output overlaps prev_warp"),
             ("conf inside prev_conf", call(conf=pp + 4 * (512 + 79)), "an output overlaps prev_conf")]
    return keep, good, call, cases


def test_every_refusal_has_its_message_on_a_host_context(lib):
    ctx = C.c_void_p()
    assert lib.lfd_create_host(1, C.byref(ctx)) == 0 and ctx.value
    try:
        keep, good, call, cases = invalid_calls()
        assert lib.lfd_refiner_head(ctx, *call()) == LFD_ERR_STATE                   # the device call on a host context
        assert b"host" in lib.lfd_last_error(ctx)
        for what, args, piece in cases:
            assert lib.lfd_refiner_head_host(ctx, *args) == LFD_ERR_INVALID, what
            msg = lib.lfd_last_error(ctx).decode()
            assert msg.startswith("lfd_refiner_head_host: ") and piece in msg, (what, msg)
        assert lib.lfd_refiner_head_host(ctx, *call()) == 0                          # ... and the call they were derived from is served
        assert lib.lfd_refiner_head_host(ctx, *call(pd=0, pc=None)) == 0
        # an output may sit right behind an input: adjacent is not overlapping
        z, warp = keep[0], keep[3]
        both = np.zeros(160 + 40 + 80, np.float32)                                  # z as f32 (1, 8, 4, 5), then warp, then conf
        args = call(z=both.ctypes.data, f32=1, warp=both.ctypes.data + 4 * 160, conf=both.ctypes.data + 4 * 200)
        assert lib.lfd_refiner_head_host(ctx, *args) == 0
    finally:
        lib.lfd_destroy(ctx)


def test_a_device_entry_point_refuses_a_host_context_and_the_python_layer_says_so():
    host = hb.HostDensifier(1)
    try:
        import torch
        z = torch.zeros(1, 2, 2, 2)
        rc = host._lib.lfd_refiner_head(host._ctx, z.data_ptr(), 1, 1, 2, 2, 2, z.data_ptr(), z.data_ptr(), z.data_ptr(), None, None, None, 0, 4.0,
                                        z.data_ptr(), z.data_ptr())
        assert rc == LFD_ERR_STATE
        with pytest.raises(hb.HipBackendError, match="device entry point called on a host context"):
            host._check(rc, "lfd_refiner_head")
    finally:
        host.close()
