"""CPU tier of the depth-uncertainty gate's entry points (lfd_depth_sigma_filter / lfd_depth_sigma_filter_host): the library exports them, the
header declares them with the argument list of DESIGN.md 4.11, the binding types them, the ABI version and the pinned structures are unchanged,
every refusal of the contract answers with its status and a context of the wrong kind is refused (a null context: LFD_ERR_INVALID; a host
context given to the device call: LFD_ERR_STATE - the reverse is tests/test_gpu_depth_sigma.py's)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import support_scene as sc
import wrefine_scene as ws
from helpers import ROOT
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

LFD_ERR_INVALID, LFD_ERR_CAPACITY, LFD_ERR_STATE = 1, 3, 4
ARGS = ["lfd_context* ctx", "const lfd_batch* batch", "const lfd_points* in", "const int64_t* ref_offsets_in", "const float* const* precision",
        "float iso_sigma_px", "const uint8_t* refine_status", "float support_thresh_px", "float max_rel_sigma", "const lfd_points* out",
        "int64_t* ref_offsets_out", "int32_t* seg_counts_out", "float* sigma_rel", "float* sigma_rel_out"]
NAMES = ["lfd_depth_sigma_filter", "lfd_depth_sigma_filter_host"]
NULL_CALL = (None, None, None, None, 0.5, None, 0.0, 0.0, None, None, None, None, None)


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
    assert lib.lfd_last_error.restype is C.c_char_p      # (... and the status values of the header)
    header = open(os.path.join(ROOT, "include", "lfd_densify.h")).read()
    for name, value in (("LFD_ERR_INVALID", LFD_ERR_INVALID), ("LFD_ERR_CAPACITY", LFD_ERR_CAPACITY), ("LFD_ERR_STATE", LFD_ERR_STATE)):
        assert re.search(name + r"\s*=\s*" + str(value) + r"\b", header) or re.search(r"#define\s+" + name + r"\s+" + str(value) + r"\b", header), name


@pytest.mark.parametrize("name", NAMES)
def test_binding_sets_argtypes(lib, name):
    import inspect
    f = getattr(lib, name)
    assert f.restype is C.c_int
    assert f.argtypes is not None and len(f.argtypes) == len(ARGS)
    assert [i for i, t in enumerate(f.argtypes) if t is C.c_float] == [5, 7, 8]
    for cls in (hb.HipDensifier, hb.HostDensifier):
        sig = inspect.signature(cls.depth_sigma_filter).parameters
        assert sig["with_sigma"].default is False and sig["refine_status"].default is None and sig["iso_sigma_px"].default == 0.0


@pytest.mark.parametrize("name", NAMES)
def test_null_context_is_invalid(lib, name):
    assert getattr(lib, name)(None, *NULL_CALL) == LFD_ERR_INVALID
    assert lib.lfd_last_error(None)


def test_host_context_is_refused_by_the_device_call(lib):
    ctx = C.c_void_p()
    assert lib.lfd_create_host(1, C.byref(ctx)) == 0 and ctx.value
    try:
        assert lib.lfd_depth_sigma_filter(ctx, *NULL_CALL) == LFD_ERR_STATE
        assert b"host" in lib.lfd_last_error(ctx)
        assert lib.lfd_depth_sigma_filter_host(ctx, *NULL_CALL) == LFD_ERR_INVALID          # its own entry point looks at the arguments
        assert b"lfd_depth_sigma_filter_host" in lib.lfd_last_error(ctx)
    finally:
        lib.lfd_destroy(ctx)


def test_every_refusal_of_the_contract(lib):
    twin = hb.HostDensifier(1)
    twin.upload_cameras(sc.cameras())
    try:
        ri = ws.reference_inputs(10, 3, 12, 16)
        batch = hb.PreparedBatch([ri], sc.MATCH, sc.MATCH)
        cap = 12 * 16
        dev = torch.device("cpu")
        src, dst, small = hb.OutputBuffers(cap, 1, 3, dev), hb.OutputBuffers(cap, 1, 3, dev), hb.OutputBuffers(cap - 1, 1, 3, dev)
        assert lib.lfd_triangulate_dense_host(twin._ctx, C.byref(batch.c), C.byref(sc.params()), C.byref(src.c), src.ref_offsets.data_ptr(),
                                              src.seg_counts.data_ptr()) == 0
        n = int(src.ref_offsets[1])
        before = src._f.clone()
        status = torch.zeros(cap, dtype=torch.uint8)
        sigma, sigma_out = torch.zeros(cap), torch.zeros(cap)
        good = dict(batch=C.byref(batch.c), pin=src.c, off=src.ref_offsets.data_ptr(), prec=C.cast(batch.precision, C.c_void_p), iso=0.0,
                    status=status.data_ptr(), tau=1.6, mx=0.05, pout=dst.c, off_out=dst.ref_offsets.data_ptr(), seg=dst.seg_counts.data_ptr(),
                    sigma=sigma.data_ptr(), sigma_out=sigma_out.data_ptr())

        def call(**kw):
            a = {**good, **kw}
            pin = C.byref(a["pin"]) if a["pin"] is not None else None
            pout = C.byref(a["pout"]) if a["pout"] is not None else None
            return lib.lfd_depth_sigma_filter_host(twin._ctx, a["batch"], pin, a["off"], a["prec"], a["iso"], a["status"], a["tau"], a["mx"], pout,
                                                   a["off_out"], a["seg"], a["sigma"], a["sigma_out"])

        keep = []

        def table(*holes):
            t = (C.c_void_p * 3)(*[None if j in holes else batch.precision[j] for j in range(3)])
            keep.append(t)
            return C.cast(t, C.c_void_p)

        def pts(base, **kw):
            vals = {name: getattr(base, name) for name, _t in hb.lfd_points._fields_}
            vals.update(kw)
            return hb.lfd_points(**vals)

        assert call() == 0 and n > 100
        kept = int(dst.ref_offsets[1])
        assert 0 < kept <= n and kept == int((sigma[:n] <= 0.05).sum()) and int(dst.seg_counts.sum()) == kept
        assert torch.equal(src._f.view(torch.int32), before.view(torch.int32))               # the input is read only
        assert call(seg=None, sigma=None, sigma_out=None) == 0                               # the optional outputs
        assert call(status=None, tau=0.0) == 0 and call(status=None, tau=float("nan")) == 0  # without a status the threshold is ignored
        assert call(prec=None, iso=0.5) == 0                                                 # the isotropic form
        assert call(mx=0.0) == 0 and int(dst.ref_offsets[1]) == n                            # annotate only
        assert call(pout=pts(dst.c, cell=None, slot=None)) == 0                              # out's cell / slot are optional, as in the siblings
        invalid = [dict(pin=None), dict(pout=None), dict(off=None), dict(off_out=None), dict(batch=None),
                   dict(pin=pts(src.c, xyz=None)), dict(pin=pts(src.c, rgb=None)), dict(pin=pts(src.c, err=None)),
                   dict(pout=pts(dst.c, xyz=None)), dict(pout=pts(dst.c, rgb=None)), dict(pout=pts(dst.c, err=None)),
                   dict(pin=pts(src.c, cell=None)), dict(pin=pts(src.c, slot=None)),
                   dict(prec=None, iso=0.0), dict(iso=0.5),                                  # neither, both
                   dict(prec=None, iso=-0.5), dict(prec=None, iso=float("nan")), dict(prec=None, iso=float("inf")), dict(iso=float("nan")),
                   dict(prec=table(0)), dict(prec=table(2)), dict(prec=table(0, 1, 2)),      # a null plane in a valid slot
                   dict(mx=-0.01), dict(mx=float("inf")), dict(mx=float("nan")),
                   dict(tau=0.0), dict(tau=-1.0), dict(tau=float("inf")), dict(tau=float("nan")),        # with a status
                   dict(pout=src.c),                                                         # in and out overlap
                   dict(pout=pts(dst.c, xyz=src.c.rgb)), dict(pout=pts(dst.c, err=src.c.err + 4)), dict(pout=pts(dst.c, slot=src.c.slot)),
                   dict(sigma=src.c.err), dict(sigma_out=src.c.xyz), dict(sigma=dst.c.err), dict(sigma=sigma_out.data_ptr()),
                   dict(pout=pts(dst.c, err=status.data_ptr())),
                   dict(pin=pts(src.c, capacity=-1)), dict(pout=pts(dst.c, capacity=-1)), dict(pin=pts(src.c, capacity=1 << 31), pout=pts(dst.c, capacity=1 << 31))]
        for kw in invalid:
            assert call(**kw) == LFD_ERR_INVALID, kw
            assert lib.lfd_last_error(twin._ctx)
        assert call(pout=small.c, off_out=small.ref_offsets.data_ptr(), seg=small.seg_counts.data_ptr()) == LFD_ERR_CAPACITY
        assert b"capacity" in lib.lfd_last_error(twin._ctx)
        # a plane beyond n_slots[r] is never looked at: two references, the second with one neighbour, its other entries null
        refs = [ri, ws.reference_inputs(20, 1, 12, 16)]
        ragged = hb.PreparedBatch(refs, sc.MATCH, sc.MATCH)
        assert ragged.k == 3 and not ragged.precision[4] and not ragged.precision[5]
        two, out2 = hb.OutputBuffers(2 * cap, 2, 3, dev), hb.OutputBuffers(2 * cap, 2, 3, dev)
        assert lib.lfd_triangulate_dense_host(twin._ctx, C.byref(ragged.c), C.byref(sc.params()), C.byref(two.c), two.ref_offsets.data_ptr(),
                                              two.seg_counts.data_ptr()) == 0
        st2 = torch.full((2 * cap,), 0x80, dtype=torch.uint8)
        assert lib.lfd_depth_sigma_filter_host(twin._ctx, C.byref(ragged.c), C.byref(two.c), two.ref_offsets.data_ptr(),
                                               C.cast(ragged.precision, C.c_void_p), 0.0, st2.data_ptr(), 1.6, 0.05, C.byref(out2.c),
                                               out2.ref_offsets.data_ptr(), out2.seg_counts.data_ptr(), None, None) == 0
        assert 0 < int(out2.ref_offsets[1]) <= int(out2.ref_offsets[2]) <= int(two.ref_offsets[2])
        # the binding's own refusals name the knob
        with pytest.raises(hb.HipBackendError, match="max_rel_sigma"):
            twin.depth_sigma_filter(batch, src, -1.0)
        with pytest.raises(hb.HipBackendError, match="support_thresh_px"):
            twin.depth_sigma_filter(batch, src, 0.05, refine_status=status, support_thresh_px=0.0)
        plain = hb.PreparedBatch([sc.reference_inputs(10, 3, 12, 16)[1]], sc.MATCH, sc.MATCH)
        with pytest.raises(ValueError, match="precision planes"):
            twin.depth_sigma_filter(plain, src, 0.05)
        assert twin.depth_sigma_filter(plain, src, 0.05, iso_sigma_px=0.5).collect().sigma_in == n         # (buffers: collect reports it)
    finally:
        twin.close()
