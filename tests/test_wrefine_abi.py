"""CPU tier of the precision-weighted re-triangulation's entry points (lfd_refine_multiview_weighted / lfd_refine_multiview_weighted_host): the
library exports them, the header declares them with lfd_refine_multiview's argument list plus the precision table, the binding types them, the
ABI version and the pinned structures are unchanged, every refusal of the contract answers with its status - a null table and a null plane in
a valid slot included - and a context of the wrong kind is refused (a null context: LFD_ERR_INVALID; a host context given to the device call:
LFD_ERR_STATE - the reverse is tests/test_gpu_wrefine.py's)."""
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

LFD_ERR_INVALID, LFD_ERR_STATE = 1, 4
ARGS = ["lfd_context* ctx", "const lfd_batch* batch", "const lfd_points* in", "const int64_t* ref_offsets", "float support_thresh_px",
        "float reproj_thresh", "float* xyz_out", "float* err_out", "uint8_t* status", "int64_t* counters", "const float* const* precision"]
NAMES = ["lfd_refine_multiview_weighted", "lfd_refine_multiview_weighted_host"]
NULL_CALL = (None, None, None, 1.0, 1.0, None, None, None, None, None)


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


@pytest.mark.parametrize("name", NAMES)
def test_binding_sets_argtypes(lib, name):
    f = getattr(lib, name)
    assert f.restype is C.c_int
    assert f.argtypes is not None and len(f.argtypes) == len(ARGS)
    assert f.argtypes[4] is C.c_float and f.argtypes[5] is C.c_float and f.argtypes[:10] == lib.lfd_refine_multiview.argtypes
    import inspect
    for cls in (hb.HipDensifier, hb.HostDensifier):
        assert inspect.signature(cls.refine_multiview).parameters["precision"].default is False
    assert callable(getattr(hb.HipDensifier, "refine_multiview", None)) and callable(getattr(hb.HostDensifier, "refine_multiview", None))


@pytest.mark.parametrize("name", NAMES)
def test_null_context_is_invalid(lib, name):
    assert getattr(lib, name)(None, *NULL_CALL) == LFD_ERR_INVALID
    assert lib.lfd_last_error(None)


def test_host_context_is_refused_by_the_device_call(lib):
    ctx = C.c_void_p()
    assert lib.lfd_create_host(1, C.byref(ctx)) == 0 and ctx.value
    try:
        assert lib.lfd_refine_multiview_weighted(ctx, *NULL_CALL) == LFD_ERR_STATE
        assert b"host" in lib.lfd_last_error(ctx)
        assert lib.lfd_refine_multiview_weighted_host(ctx, *NULL_CALL) == LFD_ERR_INVALID          # its own entry point looks at the arguments
        assert b"lfd_refine_multiview_weighted_host" in lib.lfd_last_error(ctx)
    finally:
        lib.lfd_destroy(ctx)


def test_every_refusal_of_the_contract(lib):
    twin = hb.HostDensifier(1)
    twin.upload_cameras(sc.cameras())
    try:
        ri = ws.reference_inputs(10, 3, 12, 16)
        batch = hb.PreparedBatch([ri], sc.MATCH, sc.MATCH)
        cap = 12 * 16
        src = hb.OutputBuffers(cap, 1, 3, torch.device("cpu"))
        assert lib.lfd_triangulate_dense_host(twin._ctx, C.byref(batch.c), C.byref(sc.params()), C.byref(src.c), src.ref_offsets.data_ptr(),
                                              src.seg_counts.data_ptr()) == 0
        n = int(src.ref_offsets[1])
        before = src._f.clone()
        xyz, err = torch.zeros((cap, 3)), torch.zeros(cap)
        status, counters = torch.zeros(cap, dtype=torch.uint8), torch.zeros(3, dtype=torch.int64)
        good = dict(batch=C.byref(batch.c), pin=src.c, off=src.ref_offsets.data_ptr(), tau=1.6, thr=0.8, xyz=xyz.data_ptr(), err=err.data_ptr(),
                    status=status.data_ptr(), counters=counters.data_ptr(), prec=C.cast(batch.precision, C.c_void_p))

        def call(**kw):
            a = {**good, **kw}
            pin = C.byref(a["pin"]) if a["pin"] is not None else None
            return lib.lfd_refine_multiview_weighted_host(twin._ctx, a["batch"], pin, a["off"], a["tau"], a["thr"], a["xyz"], a["err"], a["status"],
                                                          a["counters"], a["prec"])

        def table(*holes):
            """The precision table with the planes at ``holes`` nulled (kept alive by the caller's list)."""
            t = (C.c_void_p * 3)(*[None if j in holes else batch.precision[j] for j in range(3)])
            keep.append(t)
            return C.cast(t, C.c_void_p)

        keep = []

        def pts(base, **kw):
            vals = {name: getattr(base, name) for name, _t in hb.lfd_points._fields_}
            vals.update(kw)
            return hb.lfd_points(**vals)

        assert call() == 0 and n > 100 and int(counters[0]) > 0 and int(counters[:2].sum()) == int((status[:n] & 0x3f != 0).sum())
        assert int(counters[2]) == int((status[:n] & 0x40 != 0).sum()) > 0
        assert torch.equal(src._f.view(torch.int32), before.view(torch.int32))                                           # out of place: the input is read only
        assert call(status=None, counters=None) == 0                                       # the optional outputs
        assert call(pin=pts(src.c, rgb=None)) == 0                                         # the colours play no part
        invalid = [dict(pin=None), dict(off=None), dict(batch=None), dict(xyz=None), dict(err=None),
                   dict(pin=pts(src.c, cell=None)), dict(pin=pts(src.c, slot=None)), dict(pin=pts(src.c, xyz=None)), dict(pin=pts(src.c, err=None)),
                   dict(tau=0.0), dict(tau=-1.0), dict(tau=float("inf")), dict(tau=float("nan")),
                   dict(thr=0.0), dict(thr=-0.5), dict(thr=float("inf")), dict(thr=float("nan")),
                   dict(pin=pts(src.c, capacity=-1)), dict(pin=pts(src.c, capacity=1 << 31)),
                   dict(xyz=src.c.xyz + 12),                                            # partial overlap with in->xyz
                   dict(xyz=src.c.xyz),                                                 # xyz in place, err not
                   dict(err=src.c.err),                                                 # err in place, xyz not
                   dict(xyz=src.c.rgb),                                                 # inside another array of in
                   dict(err=src.c.cell),
                   dict(status=src.c.slot),
                   dict(xyz=src.c.err, err=src.c.xyz),
                   dict(err=xyz.data_ptr() + 4),                                        # the outputs overlap each other
                   dict(status=err.data_ptr()),
                   dict(prec=None), dict(prec=table(0)), dict(prec=table(2)), dict(prec=table(0, 1, 2))]
        for kw in invalid:
            assert call(**kw) == LFD_ERR_INVALID, kw
            assert lib.lfd_last_error(twin._ctx)
        # exactly in place: the same bits as out of place
        assert call() == 0
        assert call(xyz=src.c.xyz, err=src.c.err, status=None, counters=None) == 0
        assert np.array_equal(src.xyz[:n].numpy().view(np.uint32), xyz[:n].numpy().view(np.uint32))
        assert np.array_equal(src.err[:n].numpy().view(np.uint32), err[:n].numpy().view(np.uint32))
        # a plane beyond n_slots[r] is never looked at: two references, the second with one neighbour, its other entries null
        refs = [ri, ws.reference_inputs(20, 1, 12, 16)]
        ragged = hb.PreparedBatch(refs, sc.MATCH, sc.MATCH)
        assert ragged.k == 3 and not ragged.precision[4] and not ragged.precision[5]
        two = hb.OutputBuffers(2 * cap, 2, 3, torch.device("cpu"))
        assert lib.lfd_triangulate_dense_host(twin._ctx, C.byref(ragged.c), C.byref(sc.params()), C.byref(two.c), two.ref_offsets.data_ptr(),
                                              two.seg_counts.data_ptr()) == 0
        assert lib.lfd_refine_multiview_weighted_host(twin._ctx, C.byref(ragged.c), C.byref(two.c), two.ref_offsets.data_ptr(), 1.6, 0.8,
                                                      two.c.xyz, two.c.err, None, None, C.cast(ragged.precision, C.c_void_p)) == 0
        # the binding's own refusals name the knob
        with pytest.raises(hb.HipBackendError, match="support_thresh_px"):
            twin.refine_multiview(batch, src, 0.0, 0.8, precision=True)
        with pytest.raises(hb.HipBackendError, match="reproj_thresh"):
            twin.refine_multiview(batch, src, 1.6, float("nan"), precision=True)
    finally:
        twin.close()
