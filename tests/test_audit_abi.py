"""CPU tier of the epipolar audit's entry points (lfd_epipolar_audit and its _host twin): the library exports them, the
header declares them with the documented argument lists, the binding types them, the ABI version and the pinned structures are unchanged,
every refusal of the contract answers with its status and a message that names the call, a table or a cell map that overlaps the batch's
planes or each other is refused, a refused call adds nothing, and a context of the wrong kind is refused (a null context: LFD_ERR_INVALID;
a host context given to the device call: LFD_ERR_STATE - the reverse is tests/test_gpu_audit.py's)."""
import ctypes as C
import os
import re

import pytest
import torch

import audit_scene as asc
from helpers import ROOT
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

LFD_ERR_INVALID, LFD_ERR_STATE = 1, 4
ARGS = ["lfd_context* ctx", "const lfd_batch* batch", "float audit_certainty", "uint64_t* table", "uint8_t* best"]
NAMES = ("lfd_epipolar_audit", "lfd_epipolar_audit_host")
NULL_CALL = (None, 0.5, None, None)
MATCH = 64


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
    assert f.argtypes is not None and len(f.argtypes) == len(ARGS) and f.argtypes[2] is C.c_float
    for cls in (hb.HipDensifier, hb.HostDensifier):
        assert callable(getattr(cls, "epipolar_audit", None))
    assert hb.AUDIT_QUANTITIES == 66 and hb.AUDIT_NONE == 255


@pytest.mark.parametrize("name", NAMES)
def test_null_context_is_invalid(lib, name):
    assert getattr(lib, name)(None, *NULL_CALL) == LFD_ERR_INVALID
    assert lib.lfd_last_error(None)


def test_host_context_is_refused_by_the_device_call(lib):
    ctx = C.c_void_p()
    assert lib.lfd_create_host(1, C.byref(ctx)) == 0 and ctx.value
    try:
        assert lib.lfd_epipolar_audit(ctx, *NULL_CALL) == LFD_ERR_STATE
        assert b"host" in lib.lfd_last_error(ctx)
        assert lib.lfd_epipolar_audit_host(ctx, *NULL_CALL) == LFD_ERR_INVALID               # its own entry point looks at the arguments
        assert b"lfd_epipolar_audit_host: null table" in lib.lfd_last_error(ctx)
    finally:
        lib.lfd_destroy(ctx)


def test_every_refusal_of_the_contract(lib):
    twin = hb.HostDensifier(1)
    twin.upload_cameras(asc.cameras())
    try:
        H, W = 12, 16
        ri = asc.make(1, asc.neighbours(1, 3), H, W, match=MATCH, masks=True).inputs
        batch = hb.PreparedBatch([ri], MATCH, MATCH)
        table = hb.audit_table(1, 3, torch.device("cpu"))
        best = torch.zeros((1, H * W), dtype=torch.uint8)
        good = dict(batch=C.byref(batch.c), cert=0.5, table=table.data_ptr(), best=best.data_ptr())

        def call(**kw):
            a = {**good, **kw}
            return lib.lfd_epipolar_audit_host(twin._ctx, a["batch"], a["cert"], a["table"], a["best"])

        assert call() == 0
        first, first_best = table.clone(), best.clone()
        assert int(first[:, 0].sum()) > 100
        assert call(best=None) == 0 and torch.equal(table, 2 * first)                      # added to; the cell map is optional
        tb, bb = 3 * 66 * 8, H * W
        planes = [ri.cert[0], ri.cert[2], ri.warp[1], ri.image, ri.mask_a, ri.mask_b[0], ri.mask_b[2]]
        messages = {"table": b"null table", "cert": b"audit_certainty must be finite and > 0"}
        invalid = [dict(batch=None), dict(table=None), dict(cert=0.0), dict(cert=-0.5), dict(cert=float("nan")), dict(cert=float("inf")),
                   dict(best=table.data_ptr() + 8), dict(best=table.data_ptr() + tb - 1), dict(best=table.data_ptr() - bb + 1)]
        invalid += [dict(table=p.data_ptr()) for p in planes]
        invalid += [dict(table=p.data_ptr() - tb + 1) for p in planes]                   # the table's last byte reaches into the plane
        invalid += [dict(table=p.data_ptr() + p.numel() * p.element_size() - 1) for p in planes]      # its first byte is the plane's last
        invalid += [dict(best=p.data_ptr()) for p in planes]
        invalid += [dict(best=p.data_ptr() + p.numel() * p.element_size() - 1) for p in planes]
        for kw in invalid:
            assert call(**kw) == LFD_ERR_INVALID, kw
            err = lib.lfd_last_error(twin._ctx)
            assert b"lfd_epipolar_audit_host" in err or kw.get("batch", 1) is None
            (key,) = kw
            if key in messages and (kw[key] is None or key == "cert"):
                assert messages[key] in err
            elif key != "batch":                                                           # (which of the two overlaps is named depends on the heap)
                assert b"table and best overlap" in err or b"must overlap nothing of the batch" in err
        assert torch.equal(table, 2 * first) and torch.equal(best, first_best)             # a refused call adds and writes nothing
        assert call(cert=1.0) == 0                                                         # the limit itself is accepted
        # more than 65535 references (the grid's second dimension)
        small = asc.make(1, [0], 2, 2, match=MATCH).inputs
        many = hb.PreparedBatch([small] * 65536, MATCH, MATCH)
        big = torch.zeros((65536, 66), dtype=torch.int64)
        assert lib.lfd_epipolar_audit_host(twin._ctx, C.byref(many.c), 0.5, big.data_ptr(), None) == LFD_ERR_INVALID
        assert b"at most 65535 references" in lib.lfd_last_error(twin._ctx) and int(big.abs().sum()) == 0
        # the binding's own refusals name what is wrong
        with pytest.raises(hb.HipBackendError, match="audit_certainty"):
            twin.epipolar_audit(batch, 0.0)
        with pytest.raises(ValueError, match="table must be a contiguous int64"):
            twin.epipolar_audit(batch, 0.5, table=torch.zeros((3, 65), dtype=torch.int64))
        with pytest.raises(ValueError, match="best must be a contiguous uint8"):
            twin.epipolar_audit(batch, 0.5, best=torch.zeros((1, H * W + 1), dtype=torch.uint8))
    finally:
        twin.close()
