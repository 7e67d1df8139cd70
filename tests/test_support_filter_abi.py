"""CPU tier of the support filter's entry points (lfd_support_filter / lfd_support_filter_host): the library exports them, the header declares
them with the documented argument list, the binding types them, the ABI version and the pinned structures are unchanged, every refusal of the
contract answers with its status, and a context of the wrong kind is refused (a null context: LFD_ERR_INVALID; a host context given to the device
call: LFD_ERR_STATE - the reverse is tests/test_gpu_support_filter.py's)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import support_scene as sc
from helpers import ROOT
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

LFD_ERR_INVALID, LFD_ERR_CAPACITY, LFD_ERR_STATE = 1, 3, 4
LFD_MAX_SLOTS = 16
ARGS = ["lfd_context* ctx", "const lfd_batch* batch", "const lfd_points* in", "const int64_t* ref_offsets_in", "int32_t min_support",
        "float support_thresh_px", "const lfd_points* out", "int64_t* ref_offsets_out", "int32_t* seg_counts_out", "uint8_t* support"]
NAMES = ["lfd_support_filter", "lfd_support_filter_host"]
NULL_CALL = (None, None, None, 1, 1.0, None, None, None, None)


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
    assert C.sizeof(hb.lfd_params) == 32 and C.sizeof(hb.lfd_points) == 48 and C.sizeof(hb.lfd_batch) == 120
    assert hb.LFD_MAX_SLOTS == LFD_MAX_SLOTS


@pytest.mark.parametrize("name", NAMES)
def test_binding_sets_argtypes(lib, name):
    f = getattr(lib, name)
    assert f.restype is C.c_int
    assert f.argtypes is not None and len(f.argtypes) == len(ARGS)
    assert f.argtypes[4] is C.c_int32 and f.argtypes[5] is C.c_float
    assert callable(getattr(hb.HipDensifier, "support_filter", None)) and callable(getattr(hb.HostDensifier, "support_filter", None))


@pytest.mark.parametrize("name", NAMES)
def test_null_context_is_invalid(lib, name):
    assert getattr(lib, name)(None, *NULL_CALL) == LFD_ERR_INVALID
    assert lib.lfd_last_error(None)


def test_host_context_is_refused_by_the_device_call(lib):
    ctx = C.c_void_p()
    assert lib.lfd_create_host(1, C.byref(ctx)) == 0 and ctx.value
    try:
        assert lib.lfd_support_filter(ctx, *NULL_CALL) == LFD_ERR_STATE
        assert b"host" in lib.lfd_last_error(ctx)
        assert lib.lfd_support_filter_host(ctx, *NULL_CALL) == LFD_ERR_INVALID           # its own entry point looks at the arguments
        assert b"lfd_support_filter_host" in lib.lfd_last_error(ctx)
    finally:
        lib.lfd_destroy(ctx)


def test_every_refusal_of_the_contract(lib):
    twin = hb.HostDensifier(1)
    twin.upload_cameras(sc.cameras())
    try:
        _s, ri = sc.reference_inputs(10, 3, 12, 16)
        batch = hb.PreparedBatch([ri], sc.MATCH, sc.MATCH)
        src = hb.OutputBuffers(12 * 16, 1, 3, torch.device("cpu"))
        assert lib.lfd_triangulate_dense_host(twin._ctx, C.byref(batch.c), C.byref(sc.params()), C.byref(src.c), src.ref_offsets.data_ptr(),
                                              src.seg_counts.data_ptr()) == 0
        dst = hb.OutputBuffers(12 * 16, 1, 3, torch.device("cpu"))
        seg = torch.zeros(3, dtype=torch.int32)
        sup = torch.zeros(12 * 16, dtype=torch.uint8)
        good = dict(batch=C.byref(batch.c), pin=src.c, off_in=src.ref_offsets.data_ptr(), m=1, tau=1.6, pout=dst.c, off_out=dst.ref_offsets.data_ptr(),
                    seg=seg.data_ptr(), sup=sup.data_ptr())

        def call(**kw):
            a = {**good, **kw}
            pin = C.byref(a["pin"]) if a["pin"] is not None else None
            pout = C.byref(a["pout"]) if a["pout"] is not None else None
            return lib.lfd_support_filter_host(twin._ctx, a["batch"], pin, a["off_in"], a["m"], a["tau"], pout, a["off_out"], a["seg"], a["sup"])

        def pts(base, **kw):
            vals = {name: getattr(base, name) for name, _t in hb.lfd_points._fields_}
            vals.update(kw)
            return hb.lfd_points(**vals)

        assert call() == 0 and 0 < int(dst.ref_offsets[1]) <= int(src.ref_offsets[1])
        assert call(seg=None, sup=None) == 0                                              # the optional outputs
        assert call(pout=pts(dst.c, cell=None, slot=None)) == 0
        invalid = [dict(pin=None), dict(pout=None), dict(off_in=None), dict(off_out=None), dict(batch=None),
                   dict(pin=pts(src.c, cell=None)), dict(pin=pts(src.c, slot=None)), dict(pin=pts(src.c, xyz=None)), dict(pout=pts(dst.c, err=None)),
                   dict(m=0), dict(m=-1), dict(m=LFD_MAX_SLOTS), dict(m=LFD_MAX_SLOTS + 5),
                   dict(tau=0.0), dict(tau=-1.0), dict(tau=float("inf")), dict(tau=float("nan")),
                   dict(pin=pts(src.c, capacity=-1)), dict(pin=pts(src.c, capacity=1 << 31), pout=pts(dst.c, capacity=1 << 31)),
                   dict(pout=src.c),                                                    # in == out
                   dict(pout=pts(dst.c, xyz=src.c.rgb)),                                # one array of out inside one of in
                   dict(pout=pts(dst.c, slot=src.c.cell + 8))]
        for kw in invalid:
            assert call(**kw) == LFD_ERR_INVALID, kw
            assert lib.lfd_last_error(twin._ctx)
        assert call(m=LFD_MAX_SLOTS - 1) == 0                                             # the largest minimum there is: nothing survives it here
        assert int(dst.ref_offsets[1]) == 0
        assert call(pout=pts(dst.c, capacity=12 * 16 - 1)) == LFD_ERR_CAPACITY
        assert b"capacity" in lib.lfd_last_error(twin._ctx)
        assert call() == 0
        # the binding's own refusals name the knob
        with pytest.raises(hb.HipBackendError, match="support_thresh_px"):
            twin.support_filter(batch, src, 1, 0.0)
    finally:
        twin.close()
