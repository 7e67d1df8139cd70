"""CPU tier of the multi-view colour's entry points (lfd_colour_multiview / lfd_colour_multiview_host): the library exports them, the header
declares them with the documented argument lists, the binding types them, the ABI version and the pinned structures are unchanged, every
refusal of the contract answers with its status, nothing but the colour column is written, the tail beyond the last offset stays as it is, and
a context of the wrong kind is refused (a null context: LFD_ERR_INVALID; a host context given to the device call: LFD_ERR_STATE - the reverse
is tests/test_gpu_multiview_colour.py's)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import colour_scene as cs
from helpers import ROOT
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

LFD_ERR_INVALID, LFD_ERR_STATE = 1, 4
ARGS = ["lfd_context* ctx", "const lfd_batch* batch", "const lfd_points* in", "const int64_t* ref_offsets", "const uint8_t* const* nbr_image",
        "float support_thresh_px", "int32_t mode", "float* rgb_out", "uint8_t* status", "int64_t* counters"]
NAMES = ["lfd_colour_multiview", "lfd_colour_multiview_host"]
NULL_CALL = (None, None, None, None, 1.6, 1, None, None, None)


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
    assert re.search(r"#define\s+LFD_COLOUR_MEAN\s+1\b", header) and re.search(r"#define\s+LFD_COLOUR_MEDIAN\s+2\b", header)


def test_abi_version_and_struct_layouts_are_unchanged(lib):
    assert lib.lfd_abi_version() == 9 == hb.LFD_ABI_VERSION
    hb.check_struct_layout(lib)
    assert C.sizeof(hb.lfd_params) == 32 and C.sizeof(hb.lfd_points) == 48 and C.sizeof(hb.lfd_batch) == 120


@pytest.mark.parametrize("name", NAMES)
def test_binding_sets_argtypes(lib, name):
    f = getattr(lib, name)
    assert f.restype is C.c_int
    assert f.argtypes is not None and len(f.argtypes) == len(ARGS)
    assert f.argtypes[5] is C.c_float and f.argtypes[6] is C.c_int32
    for cls in (hb.HipDensifier, hb.HostDensifier):
        assert callable(getattr(cls, "colour_multiview", None))
    assert hb.COLOUR_MODES == {"mean": 1, "median": 2}


@pytest.mark.parametrize("name", NAMES)
def test_null_context_is_invalid(lib, name):
    assert getattr(lib, name)(None, *NULL_CALL) == LFD_ERR_INVALID
    assert lib.lfd_last_error(None)


def test_host_context_is_refused_by_the_device_call(lib):
    ctx = C.c_void_p()
    assert lib.lfd_create_host(1, C.byref(ctx)) == 0 and ctx.value
    try:
        assert lib.lfd_colour_multiview(ctx, *NULL_CALL) == LFD_ERR_STATE
        assert b"host" in lib.lfd_last_error(ctx)
        assert lib.lfd_colour_multiview_host(ctx, *NULL_CALL) == LFD_ERR_INVALID          # its own entry point looks at the arguments
        assert b"lfd_colour_multiview_host" in lib.lfd_last_error(ctx)
    finally:
        lib.lfd_destroy(ctx)


def test_every_refusal_of_the_contract(lib):
    twin = hb.HostDensifier(1)
    twin.upload_cameras(cs.cameras())
    try:
        ri = cs.make(10, 3, 12, 16, match=64, gains=(1.15, 0.85, 1.0, 1.0)).inputs
        batch = hb.PreparedBatch([ri], 64, 64)
        cap = 12 * 16 + 5                                   # (room beyond the last offset: it must stay as it is)
        src = hb.OutputBuffers(cap, 1, 3, torch.device("cpu"))
        src._f.fill_(0.25)
        assert lib.lfd_triangulate_dense_host(twin._ctx, C.byref(batch.c), C.byref(cs.params()), C.byref(src.c), src.ref_offsets.data_ptr(),
                                              src.seg_counts.data_ptr()) == 0
        n = int(src.ref_offsets[1])
        before = [t.clone() for t in (src._f, src.cell, src.slot)]
        parts = [t.clone() for t in (src.xyz, src.err, src.cell, src.slot)]
        rgb, status, counters = torch.full((cap, 3), 7.0), torch.full((cap,), 9, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64)
        images = C.cast(batch.nbr_images, C.c_void_p)
        good = dict(batch=C.byref(batch.c), pin=src.c, off=src.ref_offsets.data_ptr(), img=images, tau=1.6, mode=1, rgb=rgb.data_ptr(),
                    status=status.data_ptr(), counters=counters.data_ptr())

        def call(**kw):
            a = {**good, **kw}
            pin = C.byref(a["pin"]) if a["pin"] is not None else None
            return lib.lfd_colour_multiview_host(twin._ctx, a["batch"], pin, a["off"], a["img"], a["tau"], a["mode"], a["rgb"], a["status"],
                                                 a["counters"])

        def pts(base, **kw):
            vals = {name: getattr(base, name) for name, _t in hb.lfd_points._fields_}
            vals.update(kw)
            return hb.lfd_points(**vals)

        assert call() == 0 and n == 12 * 16
        assert counters.tolist() == [int((status[:n] > 0).sum()), int(status[:n].sum())] and int(counters[0]) == n
        assert int(status[:n].max()) == 4                                                  # reference + winner + two confirming neighbours
        for t, b in zip((src._f, src.cell, src.slot), before):
            assert np.array_equal(cs.bits(t), cs.bits(b))                                  # out of place: `in` is bitwise untouched
        assert (rgb[n:] == 7.0).all() and (status[n:] == 9).all()                          # points beyond the last offset are not touched
        first = rgb.clone()
        assert not torch.equal(first[:n], src.rgb[:n])                                     # (the stage does something here)
        assert call(status=None, counters=None) == 0 and torch.equal(rgb, first)           # the optional outputs; deterministic
        assert call(pin=pts(src.c, err=None)) == 0 and torch.equal(rgb, first)             # the errors play no part
        assert call(mode=2) == 0
        empty = (C.c_void_p * 3)()
        invalid = [dict(pin=None), dict(off=None), dict(batch=None), dict(rgb=None), dict(img=None),
                   dict(pin=pts(src.c, cell=None)), dict(pin=pts(src.c, slot=None)), dict(pin=pts(src.c, xyz=None)), dict(pin=pts(src.c, rgb=None)),
                   dict(img=C.cast(empty, C.c_void_p)),                                     # a null image in a valid slot
                   dict(mode=0), dict(mode=3), dict(mode=-1),
                   dict(tau=0.0), dict(tau=-1.0), dict(tau=float("inf")), dict(tau=float("nan")),
                   dict(pin=pts(src.c, capacity=-1)), dict(pin=pts(src.c, capacity=1 << 31)),
                   dict(rgb=src.c.xyz), dict(rgb=src.c.rgb + 12), dict(rgb=src.c.rgb - 12), dict(rgb=src.c.err), dict(rgb=src.c.cell),
                   dict(status=src.c.slot), dict(status=src.c.xyz), dict(status=src.c.rgb), dict(status=src.c.cell + 4),
                   dict(status=rgb.data_ptr() + 8)]                                        # the outputs overlap each other
        for kw in invalid:
            assert call(**kw) == LFD_ERR_INVALID, kw
            assert b"lfd_colour_multiview_host" in lib.lfd_last_error(twin._ctx) or kw.get("batch", 1) is None
        for t, b in zip((src._f, src.cell, src.slot), before):
            assert np.array_equal(cs.bits(t), cs.bits(b))
        # in place: rgb_out is exactly in->rgb; only that column changes, the tail stays, and the bits are the out-of-place call's
        status.fill_(9)
        assert call(rgb=src.c.rgb) == 0
        assert np.array_equal(cs.bits(src.rgb[:n]), cs.bits(first[:n]))
        assert np.array_equal(cs.bits(src.rgb[n:cap]), cs.bits(torch.full((cap - n, 3), 0.25))) and (status[n:] == 9).all()
        for t, b in zip((src.xyz, src.err, src.cell, src.slot), parts):
            assert np.array_equal(cs.bits(t), cs.bits(b))
        # the binding's own refusals name what is wrong
        with pytest.raises(ValueError, match="mode must be 'mean' or 'median'"):
            twin.colour_multiview(batch, src, 1.6, "mode")
        with pytest.raises(hb.HipBackendError, match="support_thresh_px"):
            twin.colour_multiview(batch, src, 0.0, "mean")
        plain = hb.PreparedBatch([hb.ReferenceInputs(ref_cam=ri.ref_cam, nbr_cams=ri.nbr_cams, cert=ri.cert, warp=ri.warp, image=ri.image)], 64, 64)
        with pytest.raises(ValueError, match="nbr_images"):
            twin.colour_multiview(plain, src, 1.6, "mean")
    finally:
        twin.close()
