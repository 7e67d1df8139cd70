"""CPU tier of the far-field shell's entry points (lfd_far_accumulate / lfd_far_emit and their _host twins): the library
exports them, the header declares them with the documented argument lists, the binding types them, the ABI version and the pinned
structures are unchanged, every refusal of the contract answers with its status (LFD_ERR_INVALID, LFD_ERR_STATE, LFD_ERR_CAPACITY), a table
or counters that overlap the batch's planes are refused, a refused call adds nothing, and a context of the wrong kind is refused (a null
context: LFD_ERR_INVALID; a host context given to the device call: LFD_ERR_STATE - the reverse is tests/test_gpu_far.py's)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import far_scene as fs
from helpers import ROOT
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

LFD_ERR_INVALID, LFD_ERR_CAPACITY, LFD_ERR_STATE = 1, 3, 4
ACC_ARGS = ["lfd_context* ctx", "const lfd_batch* batch", "float far_thresh_px", "float far_certainty", "int32_t far_min_views",
            "int32_t shell_cells", "uint64_t* table", "int64_t* counters"]
EMIT_ARGS = ["lfd_context* ctx", "const uint64_t* table", "int32_t shell_cells", "int64_t min_samples", "const double* centre", "double radius",
             "float* xyz", "float* rgb", "float* normal", "int32_t* samples", "int64_t capacity", "int64_t* n_out"]
ARGS = {"lfd_far_accumulate": ACC_ARGS, "lfd_far_accumulate_host": ACC_ARGS, "lfd_far_emit": EMIT_ARGS, "lfd_far_emit_host": EMIT_ARGS}
NULL_ACC = (None, 0.8, 0.5, 2, 32, None, None)
NULL_EMIT = (None, 32, 1, None, 1.0, None, None, None, None, 0, None)
NULL_CALL = {"lfd_far_accumulate": NULL_ACC, "lfd_far_accumulate_host": NULL_ACC, "lfd_far_emit": NULL_EMIT, "lfd_far_emit_host": NULL_EMIT}
MATCH = 64


@pytest.fixture(scope="module")
def lib():
    return hb.load_library()


@pytest.mark.parametrize("name", sorted(ARGS))
def test_library_exports_and_header_declares(lib, name):
    assert hasattr(lib, name)
    header = open(os.path.join(ROOT, "include", "lfd_densify.h")).read()
    decl = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert decl, f"{name} is not declared in include/lfd_densify.h"
    assert [" ".join(a.split()) for a in decl.group(1).split(",")] == ARGS[name]


def test_abi_version_and_struct_layouts_are_unchanged(lib):
    assert lib.lfd_abi_version() == 9 == hb.LFD_ABI_VERSION
    hb.check_struct_layout(lib)
    assert C.sizeof(hb.lfd_params) == 32 and C.sizeof(hb.lfd_points) == 48 and C.sizeof(hb.lfd_batch) == 120


@pytest.mark.parametrize("name", sorted(ARGS))
def test_binding_sets_argtypes(lib, name):
    f = getattr(lib, name)
    assert f.restype is C.c_int
    assert f.argtypes is not None and len(f.argtypes) == len(ARGS[name])
    if "accumulate" in name:
        assert f.argtypes[2] is C.c_float and f.argtypes[3] is C.c_float and f.argtypes[4] is C.c_int32 and f.argtypes[5] is C.c_int32
    else:
        assert f.argtypes[2] is C.c_int32 and f.argtypes[3] is C.c_int64 and f.argtypes[5] is C.c_double and f.argtypes[10] is C.c_int64
    for cls in (hb.HipDensifier, hb.HostDensifier):
        assert callable(getattr(cls, "far_accumulate", None)) and callable(getattr(cls, "far_emit", None))
    assert hb.FAR_QUANTITIES == 7


@pytest.mark.parametrize("name", sorted(ARGS))
def test_null_context_is_invalid(lib, name):
    assert getattr(lib, name)(None, *NULL_CALL[name]) == LFD_ERR_INVALID
    assert lib.lfd_last_error(None)


def test_host_context_is_refused_by_the_device_calls(lib):
    ctx = C.c_void_p()
    assert lib.lfd_create_host(1, C.byref(ctx)) == 0 and ctx.value
    try:
        for name in ("lfd_far_accumulate", "lfd_far_emit"):
            assert getattr(lib, name)(ctx, *NULL_CALL[name]) == LFD_ERR_STATE
            assert b"host" in lib.lfd_last_error(ctx)
            assert getattr(lib, name + "_host")(ctx, *NULL_CALL[name]) == LFD_ERR_INVALID          # its own entry point looks at the arguments
            assert (name + "_host").encode() in lib.lfd_last_error(ctx)
    finally:
        lib.lfd_destroy(ctx)


def test_every_refusal_of_the_accumulate_contract(lib):
    twin = hb.HostDensifier(1)
    twin.upload_cameras(fs.cameras())
    try:
        ri = fs.make(1, fs.others(1, 3), 12, 16, match=MATCH, masks=True).inputs
        batch = hb.PreparedBatch([ri], MATCH, MATCH)
        S = 8
        table = hb.far_table(S, torch.device("cpu"))
        counters = torch.zeros(1, dtype=torch.int64)
        good = dict(batch=C.byref(batch.c), tau=0.8, cert=0.5, views=2, S=S, table=table.data_ptr(), counters=counters.data_ptr())

        def call(**kw):
            a = {**good, **kw}
            return lib.lfd_far_accumulate_host(twin._ctx, a["batch"], a["tau"], a["cert"], a["views"], a["S"], a["table"], a["counters"])

        assert call() == 0
        first, n_far = table.clone(), int(counters[0])
        assert n_far > 10 and int(first[:, 6].sum()) == n_far
        assert call(counters=None) == 0 and torch.equal(table, 2 * first) and int(counters[0]) == n_far      # added to; the counters are optional
        tb = 6 * S * S * 7 * 8
        planes = [ri.cert[0], ri.cert[2], ri.warp[1], ri.image, ri.mask_a, ri.mask_b[0], ri.mask_b[2]]
        invalid = [dict(batch=None), dict(table=None),
                   dict(tau=0.0), dict(tau=-1.0), dict(tau=float("inf")), dict(tau=float("nan")),
                   dict(cert=0.0), dict(cert=-0.5), dict(cert=float("nan")), dict(cert=float("inf")),
                   dict(views=0), dict(views=9), dict(views=-1), dict(S=7), dict(S=513), dict(S=0),
                   dict(counters=table.data_ptr() + 8), dict(counters=table.data_ptr() + tb - 4)]
        invalid += [dict(table=p.data_ptr()) for p in planes]
        invalid += [dict(table=p.data_ptr() - tb + 1) for p in planes]                   # the table's last byte reaches into the plane
        invalid += [dict(table=p.data_ptr() + p.numel() * p.element_size() - 1) for p in planes]      # its first byte is the plane's last
        invalid += [dict(counters=p.data_ptr()) for p in planes]
        for kw in invalid:
            assert call(**kw) == LFD_ERR_INVALID, kw
            assert b"lfd_far_accumulate_host" in lib.lfd_last_error(twin._ctx) or kw.get("batch", 1) is None
        assert torch.equal(table, 2 * first) and int(counters[0]) == n_far                # a refused call adds nothing
        # the limits themselves are accepted
        for kw in (dict(views=1), dict(views=8), dict(cert=1.0), dict(S=8)):
            assert call(**kw) == 0, kw
        big = hb.far_table(512, torch.device("cpu"))
        assert call(S=512, table=big.data_ptr()) == 0 and int(big[:, 6].sum()) == n_far
        # the binding's own refusals name what is wrong
        with pytest.raises(hb.HipBackendError, match="far_thresh_px"):
            twin.far_accumulate(batch, 0.0, 0.5, 2, 8)
        with pytest.raises(ValueError, match="table must be a contiguous int64"):
            twin.far_accumulate(batch, 0.8, 0.5, 2, 8, table=torch.zeros((6 * 64, 6), dtype=torch.int64))
        with pytest.raises(ValueError, match="counters must be a contiguous int64"):
            twin.far_accumulate(batch, 0.8, 0.5, 2, 8, counters=torch.zeros(2, dtype=torch.int64))
    finally:
        twin.close()


def test_every_refusal_of_the_emit_contract(lib):
    twin = hb.HostDensifier(1)
    twin.upload_cameras(fs.cameras())
    try:
        ri = fs.make(1, fs.others(1, 3), 12, 16, match=MATCH).inputs
        S = 8
        table = twin.far_accumulate(hb.PreparedBatch([ri], MATCH, MATCH), 0.8, 0.5, 2, S)
        before = table.clone()
        n = int((table[:, 6] >= 1).sum())
        assert n >= 2
        cap = n + 3
        xyz, rgb, nrm = (torch.full((cap, 3), 7.0) for _ in range(3))
        smp = torch.full((cap,), -5, dtype=torch.int32)
        c3 = (C.c_double * 3)(0.5, -1.0, 2.0)
        n_out = C.c_int64(-1)
        good = dict(table=table.data_ptr(), S=S, ms=1, centre=c3, radius=10.0, xyz=xyz.data_ptr(), rgb=rgb.data_ptr(), nrm=nrm.data_ptr(),
                    smp=smp.data_ptr(), cap=cap, n_out=C.byref(n_out))

        def call(**kw):
            a = {**good, **kw}
            return lib.lfd_far_emit_host(twin._ctx, a["table"], a["S"], a["ms"], a["centre"], a["radius"], a["xyz"], a["rgb"], a["nrm"], a["smp"],
                                         a["cap"], a["n_out"])

        assert call() == 0 and n_out.value == n
        assert (xyz[n:] == 7.0).all() and (smp[n:] == -5).all() and (smp[:n] >= 1).all()      # nothing beyond the count is written
        assert call(nrm=None, smp=None) == 0 and n_out.value == n                              # the optional outputs
        nan, inf = float("nan"), float("inf")
        tb = 6 * S * S * 7 * 8
        invalid = [dict(table=None), dict(centre=None), dict(xyz=None), dict(rgb=None), dict(n_out=None),
                   dict(S=7), dict(S=513), dict(ms=0), dict(ms=-3), dict(radius=0.0), dict(radius=-1.0), dict(radius=nan), dict(radius=inf),
                   dict(centre=(C.c_double * 3)(nan, 0.0, 0.0)), dict(centre=(C.c_double * 3)(0.0, inf, 0.0)),
                   dict(cap=-1), dict(cap=1 << 31),
                   dict(xyz=table.data_ptr()), dict(rgb=table.data_ptr() + tb - 4), dict(nrm=table.data_ptr() - 12 * cap + 4),
                   dict(smp=table.data_ptr() + 16), dict(rgb=xyz.data_ptr()), dict(nrm=rgb.data_ptr() + 12), dict(smp=xyz.data_ptr() + 12 * cap - 4)]
        for kw in invalid:
            assert call(**kw) == LFD_ERR_INVALID, kw
            assert b"lfd_far_emit_host" in lib.lfd_last_error(twin._ctx)
        # too small a capacity: the count that is needed, the first records, LFD_ERR_CAPACITY
        full = xyz[:n].clone()
        xyz.fill_(7.0)
        assert call(cap=n - 1) == LFD_ERR_CAPACITY and n_out.value == n
        assert torch.equal(xyz[:n - 1], full[:n - 1]) and (xyz[n - 1:] == 7.0).all()
        assert call(cap=0) == LFD_ERR_CAPACITY and n_out.value == n
        assert call(ms=int(table[:, 6].max()) + 1, cap=0) == 0 and n_out.value == 0           # nothing qualifies: no capacity is needed
        assert torch.equal(table, before)                                                     # reads only
    finally:
        twin.close()
