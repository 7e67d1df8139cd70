"""CPU tier of the photo-consistency gate's entry points (lfd_photo_gate / lfd_photo_gate_host): the library exports them, the header declares
them with the documented argument lists, the binding types them, the ABI version and the pinned structures are unchanged, every refusal of
the contract answers with its status (LFD_ERR_INVALID, LFD_ERR_CAPACITY), `in` is never written, the tail of the per-point outputs beyond the
last offset stays as it is, and a context of the wrong kind is refused (a null context: LFD_ERR_INVALID; a host context given to the device
call: LFD_ERR_STATE - the reverse is tests/test_gpu_photo.py's)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import colour_scene as cs
import photo_scene as ps
from helpers import ROOT
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

LFD_ERR_INVALID, LFD_ERR_CAPACITY, LFD_ERR_STATE = 1, 3, 4
ARGS = ["lfd_context* ctx", "const lfd_batch* batch", "const lfd_points* in", "const int64_t* ref_offsets_in", "const uint8_t* const* nbr_image",
        "int32_t window_cells", "float min_ncc", "float min_texture", "const lfd_points* out", "int64_t* ref_offsets_out", "int32_t* seg_counts_out",
        "uint8_t* status", "float* ncc", "int64_t* counters"]
NAMES = ["lfd_photo_gate", "lfd_photo_gate_host"]
NULL_CALL = (None, None, None, None, 2, 0.8, 2.0, None, None, None, None, None, None)


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


def test_error_codes_are_the_headers(lib):
    header = open(os.path.join(ROOT, "include", "lfd_densify.h")).read()
    for name, value in (("LFD_ERR_INVALID", LFD_ERR_INVALID), ("LFD_ERR_CAPACITY", LFD_ERR_CAPACITY), ("LFD_ERR_STATE", LFD_ERR_STATE)):
        assert re.search(r"\b" + name + r"\s*=?\s*" + str(value) + r"\b", header), name


def test_abi_version_and_struct_layouts_are_unchanged(lib):
    assert lib.lfd_abi_version() == 9 == hb.LFD_ABI_VERSION
    hb.check_struct_layout(lib)
    assert C.sizeof(hb.lfd_params) == 32 and C.sizeof(hb.lfd_points) == 48 and C.sizeof(hb.lfd_batch) == 120


@pytest.mark.parametrize("name", NAMES)
def test_binding_sets_argtypes(lib, name):
    f = getattr(lib, name)
    assert f.restype is C.c_int
    assert f.argtypes is not None and len(f.argtypes) == len(ARGS)
    assert f.argtypes[5] is C.c_int32 and f.argtypes[6] is C.c_float and f.argtypes[7] is C.c_float
    for cls in (hb.HipDensifier, hb.HostDensifier):
        assert callable(getattr(cls, "photo_gate", None))
    assert hb.PHOTO_STATUSES == 5


@pytest.mark.parametrize("name", NAMES)
def test_null_context_is_invalid(lib, name):
    assert getattr(lib, name)(None, *NULL_CALL) == LFD_ERR_INVALID
    assert lib.lfd_last_error(None)


def test_host_context_is_refused_by_the_device_call(lib):
    ctx = C.c_void_p()
    assert lib.lfd_create_host(1, C.byref(ctx)) == 0 and ctx.value
    try:
        assert lib.lfd_photo_gate(ctx, *NULL_CALL) == LFD_ERR_STATE
        assert b"host" in lib.lfd_last_error(ctx)
        assert lib.lfd_photo_gate_host(ctx, *NULL_CALL) == LFD_ERR_INVALID                 # its own entry point looks at the arguments
        assert b"lfd_photo_gate_host" in lib.lfd_last_error(ctx)
    finally:
        lib.lfd_destroy(ctx)


def test_every_refusal_of_the_contract(lib):
    twin = hb.HostDensifier(1)
    twin.upload_cameras(cs.cameras())
    try:
        H, W = 12, 16
        ri = ps.make(10, 3, H, W, match=64, slide_rows=(4, 8), slide_px=3.0).inputs
        batch = hb.PreparedBatch([ri], 64, 64)
        cap = H * W + 5                                     # (room beyond the last offset: it must stay as it is)
        src, dst = hb.OutputBuffers(cap, 1, 3, torch.device("cpu")), hb.OutputBuffers(cap, 1, 3, torch.device("cpu"))
        src._f.fill_(0.25)
        assert lib.lfd_triangulate_dense_host(twin._ctx, C.byref(batch.c), C.byref(ps.params()), C.byref(src.c), src.ref_offsets.data_ptr(),
                                              src.seg_counts.data_ptr()) == 0
        n = int(src.ref_offsets[1])
        before = [t.clone() for t in (src._f, src.cell, src.slot, src.ref_offsets)]
        status, ncc = torch.full((cap,), 9, dtype=torch.uint8), torch.full((cap,), 7.0)
        counters = torch.zeros(5, dtype=torch.int64)
        images = C.cast(batch.nbr_images, C.c_void_p)
        good = dict(batch=C.byref(batch.c), pin=src.c, off=src.ref_offsets.data_ptr(), img=images, R=2, ncc_min=0.8, tex=2.0, pout=dst.c,
                    off_out=dst.ref_offsets.data_ptr(), seg=dst.seg_counts.data_ptr(), status=status.data_ptr(), ncc=ncc.data_ptr(),
                    counters=counters.data_ptr())

        def call(**kw):
            a = {**good, **kw}
            pin = C.byref(a["pin"]) if a["pin"] is not None else None
            pout = C.byref(a["pout"]) if a["pout"] is not None else None
            return lib.lfd_photo_gate_host(twin._ctx, a["batch"], pin, a["off"], a["img"], a["R"], a["ncc_min"], a["tex"], pout, a["off_out"], a["seg"],
                                           a["status"], a["ncc"], a["counters"])

        def pts(base, **kw):
            vals = {name: getattr(base, name) for name, _t in hb.lfd_points._fields_}
            vals.update(kw)
            return hb.lfd_points(**vals)

        assert call() == 0 and 100 < n <= H * W
        kept = int(dst.ref_offsets[1])
        assert counters.tolist() == np.bincount(status[:n].numpy(), minlength=5).tolist() and int(counters[4]) == n - kept > 0
        assert int(dst.seg_counts.sum()) == kept
        for t, b in zip((src._f, src.cell, src.slot, src.ref_offsets), before):
            assert np.array_equal(ps.bits(t), ps.bits(b))                                  # `in` is bitwise untouched
        assert (status[n:] == 9).all() and (ncc[n:] == 7.0).all()                          # points beyond the last offset are not touched
        first = [t.clone() for t in (dst._f, dst.cell, dst.slot)]
        counters.zero_()
        assert call(status=None, ncc=None, counters=None, seg=None) == 0                   # the optional outputs; deterministic
        assert all(np.array_equal(ps.bits(t[:kept]), ps.bits(b[:kept])) for t, b in zip((dst.xyz, dst.cell, dst.slot), (first[0].view(-1)[:3 * cap].view(cap, 3), first[1], first[2])))
        assert counters.tolist() == [0] * 5
        empty = (C.c_void_p * 3)()
        one_less = hb.OutputBuffers(cap - 1, 1, 3, torch.device("cpu"))
        invalid = [dict(pin=None), dict(pout=None), dict(off=None), dict(off_out=None), dict(batch=None), dict(img=None),
                   dict(pin=pts(src.c, cell=None)), dict(pin=pts(src.c, slot=None)), dict(pin=pts(src.c, xyz=None)), dict(pin=pts(src.c, rgb=None)),
                   dict(pin=pts(src.c, err=None)), dict(pout=pts(dst.c, xyz=None)),
                   dict(img=C.cast(empty, C.c_void_p)),                                     # a null image in a valid slot
                   dict(R=0), dict(R=4), dict(R=-1),
                   dict(ncc_min=0.0), dict(ncc_min=-0.5), dict(ncc_min=1.5), dict(ncc_min=float("nan")), dict(ncc_min=float("inf")),
                   dict(tex=-1.0), dict(tex=float("nan")), dict(tex=float("inf")),
                   dict(pin=pts(src.c, capacity=-1)), dict(pin=pts(src.c, capacity=1 << 31)), dict(pout=pts(dst.c, capacity=-1)),
                   dict(pout=src.c), dict(pout=pts(dst.c, rgb=src.c.xyz + 12)), dict(pout=pts(dst.c, slot=src.c.slot + 3)),     # in and out overlap
                   dict(status=src.c.slot), dict(status=dst.c.cell), dict(ncc=src.c.err), dict(ncc=dst.c.xyz + 4), dict(counters=src.c.rgb),
                   dict(status=ncc.data_ptr() + 8), dict(counters=ncc.data_ptr())]         # the outputs overlap each other
        for kw in invalid:
            assert call(**kw) == LFD_ERR_INVALID, kw
            assert b"lfd_photo_gate_host" in lib.lfd_last_error(twin._ctx) or kw.get("batch", 1) is None
        assert call(pout=one_less.c) == LFD_ERR_CAPACITY and b"capacity" in lib.lfd_last_error(twin._ctx)
        # a null image of the reference is the batch's to refuse
        hurt = hb.PreparedBatch([ri], 64, 64)
        hurt.image[0] = None
        assert call(batch=C.byref(hurt.c)) == LFD_ERR_INVALID and b"image" in lib.lfd_last_error(twin._ctx)
        for t, b in zip((src._f, src.cell, src.slot, src.ref_offsets), before):
            assert np.array_equal(ps.bits(t), ps.bits(b))
        # the limits of the ranges are inside them
        assert call(ncc_min=1.0) == 0 and call(tex=0.0) == 0 and call(R=1) == 0 and call(R=3) == 0
        # the binding's own refusals name what is wrong
        with pytest.raises(ValueError, match="window_cells must be an integer"):
            twin.photo_gate(batch, src, 2.0, 0.8, 2.0)
        with pytest.raises(hb.HipBackendError, match="min_ncc"):
            twin.photo_gate(batch, src, 2, 0.0, 2.0)
        with pytest.raises(ValueError, match="five elements"):
            twin.photo_gate(batch, src, 2, 0.8, 2.0, counters=torch.zeros(2, dtype=torch.int64))
        plain = hb.PreparedBatch([hb.ReferenceInputs(ref_cam=ri.ref_cam, nbr_cams=ri.nbr_cams, cert=ri.cert, warp=ri.warp, image=ri.image)], 64, 64)
        with pytest.raises(ValueError, match="nbr_images"):
            twin.photo_gate(plain, src, 2, 0.8, 2.0)
    finally:
        twin.close()
