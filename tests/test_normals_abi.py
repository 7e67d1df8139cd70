"""CPU tier of the per-point normals' entry points (lfd_estimate_normals / lfd_estimate_normals_host / lfd_pack_ply_normals): the library
exports them, the header declares them with the documented argument lists, the binding types them, the ABI version and the pinned structures
are unchanged, every refusal of the contract answers with its status, the input is bitwise untouched, and a context of the wrong kind is refused
(a null context: LFD_ERR_INVALID; a host context given to a device call: LFD_ERR_STATE - the reverse is tests/test_gpu_normals.py's)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import normals_scene as ns
from helpers import ROOT
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

LFD_ERR_INVALID, LFD_ERR_STATE = 1, 4
ARGS = ["lfd_context* ctx", "const lfd_batch* batch", "const lfd_points* in", "const int64_t* ref_offsets", "int32_t radius_cells",
        "float depth_step_rel", "float reproj_thresh", "float* normals_out", "uint8_t* status", "int64_t* counters"]
PACK_ARGS = ["lfd_context* ctx", "const float* xyz", "const float* normals", "const float* rgb", "int64_t n", "uint8_t* out"]
NAMES = ["lfd_estimate_normals", "lfd_estimate_normals_host"]
NULL_CALL = (None, None, None, 1, 0.05, 1.0, None, None, None)


@pytest.fixture(scope="module")
def lib():
    return hb.load_library()


@pytest.mark.parametrize("name,args", [(NAMES[0], ARGS), (NAMES[1], ARGS), ("lfd_pack_ply_normals", PACK_ARGS)])
def test_library_exports_and_header_declares(lib, name, args):
    assert hasattr(lib, name)
    header = open(os.path.join(ROOT, "include", "lfd_densify.h")).read()
    decl = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert decl, f"{name} is not declared in include/lfd_densify.h"
    assert [" ".join(a.split()) for a in decl.group(1).split(",")] == args


def test_abi_version_and_struct_layouts_are_unchanged(lib):
    assert lib.lfd_abi_version() == 9 == hb.LFD_ABI_VERSION
    hb.check_struct_layout(lib)
    assert C.sizeof(hb.lfd_params) == 32 and C.sizeof(hb.lfd_points) == 48 and C.sizeof(hb.lfd_batch) == 120


@pytest.mark.parametrize("name", NAMES)
def test_binding_sets_argtypes(lib, name):
    f = getattr(lib, name)
    assert f.restype is C.c_int
    assert f.argtypes is not None and len(f.argtypes) == len(ARGS)
    assert f.argtypes[4] is C.c_int32 and f.argtypes[5] is C.c_float and f.argtypes[6] is C.c_float
    assert lib.lfd_pack_ply_normals.restype is C.c_int and len(lib.lfd_pack_ply_normals.argtypes) == len(PACK_ARGS)
    for cls in (hb.HipDensifier, hb.HostDensifier):
        assert callable(getattr(cls, "estimate_normals", None)) and callable(getattr(cls, "pack_ply_normals", None))


@pytest.mark.parametrize("name", NAMES)
def test_null_context_is_invalid(lib, name):
    assert getattr(lib, name)(None, *NULL_CALL) == LFD_ERR_INVALID
    assert lib.lfd_last_error(None)
    assert lib.lfd_pack_ply_normals(None, None, None, None, 0, None) == LFD_ERR_INVALID


def test_host_context_is_refused_by_the_device_calls(lib):
    ctx = C.c_void_p()
    assert lib.lfd_create_host(1, C.byref(ctx)) == 0 and ctx.value
    try:
        assert lib.lfd_estimate_normals(ctx, *NULL_CALL) == LFD_ERR_STATE
        assert b"host" in lib.lfd_last_error(ctx)
        assert lib.lfd_estimate_normals_host(ctx, *NULL_CALL) == LFD_ERR_INVALID          # its own entry point looks at the arguments
        assert b"lfd_estimate_normals_host" in lib.lfd_last_error(ctx)
        assert lib.lfd_pack_ply_normals(ctx, None, None, None, 0, None) == LFD_ERR_STATE    # as lfd_pack_ply: a device call
    finally:
        lib.lfd_destroy(ctx)


def test_every_refusal_of_the_contract(lib):
    twin = hb.HostDensifier(1)
    twin.upload_cameras(ns.cameras())
    try:
        ri = ns.reference_inputs("plane", 10, 3, 12, 16, tilt_deg=40.0)[0]
        batch = hb.PreparedBatch([ri], ns.W_MATCH, ns.H_MATCH)
        cap = 12 * 16 + 5                                   # (room beyond the last offset: it must stay as it is)
        src = hb.OutputBuffers(cap, 1, 3, torch.device("cpu"))
        assert lib.lfd_triangulate_dense_host(twin._ctx, C.byref(batch.c), C.byref(ns.params()), C.byref(src.c), src.ref_offsets.data_ptr(),
                                              src.seg_counts.data_ptr()) == 0
        n = int(src.ref_offsets[1])
        before = [t.clone() for t in (src._f, src.cell, src.slot)]
        normals, status, counters = torch.full((cap, 3), 7.0), torch.full((cap,), 9, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64)
        good = dict(batch=C.byref(batch.c), pin=src.c, off=src.ref_offsets.data_ptr(), radius=2, step=0.5, thr=0.8, normals=normals.data_ptr(),
                    status=status.data_ptr(), counters=counters.data_ptr())

        def call(**kw):
            a = {**good, **kw}
            pin = C.byref(a["pin"]) if a["pin"] is not None else None
            return lib.lfd_estimate_normals_host(twin._ctx, a["batch"], pin, a["off"], a["radius"], a["step"], a["thr"], a["normals"], a["status"],
                                                 a["counters"])

        def pts(base, **kw):
            vals = {name: getattr(base, name) for name, _t in hb.lfd_points._fields_}
            vals.update(kw)
            return hb.lfd_points(**vals)

        assert call() == 0 and n == 12 * 16
        assert counters.tolist() == [int((status[:n] & 0x80 != 0).sum()), int((status[:n] & 0x80 == 0).sum())] and int(counters[0]) == n
        for t, b in zip((src._f, src.cell, src.slot), before):
            assert np.array_equal(ns.bits(t), ns.bits(b))                                  # `in` is bitwise untouched
        assert (normals[n:] == 7.0).all() and (status[n:] == 9).all()                      # points beyond the last offset are not touched
        first = normals.clone()
        assert call(status=None, counters=None) == 0 and torch.equal(normals, first)       # the optional outputs; deterministic
        assert call(pin=pts(src.c, rgb=None, err=None)) == 0                               # colours and errors play no part
        for r in (1, 2, 3, 4):
            assert call(radius=r) == 0
        invalid = [dict(pin=None), dict(off=None), dict(batch=None), dict(normals=None),
                   dict(pin=pts(src.c, cell=None)), dict(pin=pts(src.c, slot=None)), dict(pin=pts(src.c, xyz=None)),
                   dict(radius=0), dict(radius=5), dict(radius=-1),
                   dict(step=0.0), dict(step=-1.0), dict(step=float("inf")), dict(step=float("nan")),
                   dict(thr=0.0), dict(thr=-0.5), dict(thr=float("inf")), dict(thr=float("nan")),
                   dict(pin=pts(src.c, capacity=-1)), dict(pin=pts(src.c, capacity=1 << 31)),
                   dict(normals=src.c.xyz), dict(normals=src.c.xyz + 12), dict(normals=src.c.rgb), dict(normals=src.c.err), dict(normals=src.c.cell),
                   dict(status=src.c.slot), dict(status=src.c.xyz), dict(status=src.c.cell + 4),
                   dict(status=normals.data_ptr() + 8)]                                    # the outputs overlap each other
        for kw in invalid:
            assert call(**kw) == LFD_ERR_INVALID, kw
            assert b"lfd_estimate_normals_host" in lib.lfd_last_error(twin._ctx) or kw.get("batch", 1) is None
        for t, b in zip((src._f, src.cell, src.slot), before):
            assert np.array_equal(ns.bits(t), ns.bits(b))
        # the binding's own refusals name the knob
        with pytest.raises(hb.HipBackendError, match="radius_cells"):
            twin.estimate_normals(batch, src, 5, 0.05, 0.8)
        with pytest.raises(hb.HipBackendError, match="depth_step_rel"):
            twin.estimate_normals(batch, src, 1, 0.0, 0.8)
        with pytest.raises(hb.HipBackendError, match="reproj_thresh"):
            twin.estimate_normals(batch, src, 1, 0.05, float("nan"))
        with pytest.raises(ValueError, match="radius must be an integer"):
            twin.estimate_normals(batch, src, 1.5, 0.05, 0.8)
    finally:
        twin.close()
