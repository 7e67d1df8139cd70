"""CPU tier of the gain compensation's entry points (lfd_gain_accumulate / lfd_gain_apply and their _host twins): the library exports them,
the header declares them with the documented argument lists, the binding types them, the ABI version and the pinned structures are
unchanged, every refusal of the contract answers with its status, nothing of the input is written, and a context of the wrong kind is
refused (a null context: LFD_ERR_INVALID; a host context given to the device call: LFD_ERR_STATE - the reverse is
tests/test_gpu_gain.py's)."""
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
ACC_ARGS = ["lfd_context* ctx", "const lfd_batch* batch", "const lfd_points* in", "const int64_t* ref_offsets", "const uint8_t* const* nbr_image",
            "float support_thresh_px", "uint64_t* table"]
APPLY_ARGS = ["lfd_context* ctx", "const float* rgb", "int64_t n", "const int64_t* ref_offsets", "int32_t n_refs", "const float* factors",
              "float* rgb_out"]
ARGS = {"lfd_gain_accumulate": ACC_ARGS, "lfd_gain_accumulate_host": ACC_ARGS, "lfd_gain_apply": APPLY_ARGS, "lfd_gain_apply_host": APPLY_ARGS}
NULL_CALL = {"lfd_gain_accumulate": (None, None, None, None, 1.6, None), "lfd_gain_accumulate_host": (None, None, None, None, 1.6, None),
             "lfd_gain_apply": (None, 0, None, 1, None, None), "lfd_gain_apply_host": (None, 0, None, 1, None, None)}


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
        assert f.argtypes[5] is C.c_float
    else:
        assert f.argtypes[2] is C.c_int64 and f.argtypes[4] is C.c_int32
    for cls in (hb.HipDensifier, hb.HostDensifier):
        assert callable(getattr(cls, "gain_accumulate", None)) and callable(getattr(cls, "gain_apply", None))
    assert hb.GAIN_QUANTITIES == 7


@pytest.mark.parametrize("name", sorted(ARGS))
def test_null_context_is_invalid(lib, name):
    assert getattr(lib, name)(None, *NULL_CALL[name]) == LFD_ERR_INVALID
    assert lib.lfd_last_error(None)


def test_host_context_is_refused_by_the_device_calls(lib):
    ctx = C.c_void_p()
    assert lib.lfd_create_host(1, C.byref(ctx)) == 0 and ctx.value
    try:
        for name in ("lfd_gain_accumulate", "lfd_gain_apply"):
            assert getattr(lib, name)(ctx, *NULL_CALL[name]) == LFD_ERR_STATE
            assert b"host" in lib.lfd_last_error(ctx)
            assert getattr(lib, name + "_host")(ctx, *NULL_CALL[name]) == LFD_ERR_INVALID          # its own entry point looks at the arguments
            assert (name + "_host").encode() in lib.lfd_last_error(ctx)
    finally:
        lib.lfd_destroy(ctx)


def test_every_refusal_of_the_accumulate_contract(lib):
    twin = hb.HostDensifier(1)
    twin.upload_cameras(cs.cameras())
    try:
        ri = cs.make(10, 3, 12, 16, match=64, gains=(1.15, 0.85, 1.0, 1.0)).inputs
        batch = hb.PreparedBatch([ri], 64, 64)
        cap = 12 * 16 + 5
        src = hb.OutputBuffers(cap, 1, 3, torch.device("cpu"))
        src._f.fill_(0.25)
        assert lib.lfd_triangulate_dense_host(twin._ctx, C.byref(batch.c), C.byref(cs.params()), C.byref(src.c), src.ref_offsets.data_ptr(),
                                              src.seg_counts.data_ptr()) == 0
        n = int(src.ref_offsets[1])
        before = [t.clone() for t in (src._f, src.cell, src.slot)]
        table = torch.zeros((3, 7), dtype=torch.int64)
        images = C.cast(batch.nbr_images, C.c_void_p)
        good = dict(batch=C.byref(batch.c), pin=src.c, off=src.ref_offsets.data_ptr(), img=images, tau=1.6, table=table.data_ptr())

        def call(**kw):
            a = {**good, **kw}
            pin = C.byref(a["pin"]) if a["pin"] is not None else None
            return lib.lfd_gain_accumulate_host(twin._ctx, a["batch"], pin, a["off"], a["img"], a["tau"], a["table"])

        def pts(base, **kw):
            vals = {name: getattr(base, name) for name, _t in hb.lfd_points._fields_}
            vals.update(kw)
            return hb.lfd_points(**vals)

        assert call() == 0 and n == 12 * 16
        first = table.clone()
        assert int(first[:, 0].min()) >= 64 and int(first[:, 0].max()) <= n               # every slot confirms most points of this scene
        assert (first[:, 1:] >= first[:, :1] * int(0.05 * 2 ** 24)).all() and (first[:, 1:] <= first[:, :1] * int(0.95 * 2 ** 24)).all()
        assert call(pin=pts(src.c, err=None)) == 0 and torch.equal(table, 2 * first)       # the errors play no part; the table is added to
        empty = (C.c_void_p * 3)()
        invalid = [dict(pin=None), dict(off=None), dict(batch=None), dict(img=None), dict(table=None),
                   dict(pin=pts(src.c, cell=None)), dict(pin=pts(src.c, slot=None)), dict(pin=pts(src.c, xyz=None)), dict(pin=pts(src.c, rgb=None)),
                   dict(img=C.cast(empty, C.c_void_p)),                                     # a null image in a valid slot
                   dict(tau=0.0), dict(tau=-1.0), dict(tau=float("inf")), dict(tau=float("nan")),
                   dict(pin=pts(src.c, capacity=-1)), dict(pin=pts(src.c, capacity=1 << 31)),
                   dict(table=src.c.xyz), dict(table=src.c.rgb), dict(table=src.c.rgb + 12 * cap - 8), dict(table=src.c.err), dict(table=src.c.cell),
                   dict(table=src.c.slot), dict(table=src.c.xyz - 3 * 7 * 8 + 4)]           # the table's last bytes reach into xyz
        for kw in invalid:
            assert call(**kw) == LFD_ERR_INVALID, kw
            assert b"lfd_gain_accumulate_host" in lib.lfd_last_error(twin._ctx) or kw.get("batch", 1) is None
        assert torch.equal(table, 2 * first)                                               # a refused call adds nothing
        for t, b in zip((src._f, src.cell, src.slot), before):
            assert np.array_equal(cs.bits(t), cs.bits(b))                                  # `in` is bitwise untouched
        # the binding's own refusals name what is wrong
        with pytest.raises(hb.HipBackendError, match="support_thresh_px"):
            twin.gain_accumulate(batch, src, 0.0)
        with pytest.raises(ValueError, match="table must be a contiguous int64"):
            twin.gain_accumulate(batch, src, 1.6, table=torch.zeros((3, 6), dtype=torch.int64))
        plain = hb.PreparedBatch([hb.ReferenceInputs(ref_cam=ri.ref_cam, nbr_cams=ri.nbr_cams, cert=ri.cert, warp=ri.warp, image=ri.image)], 64, 64)
        with pytest.raises(ValueError, match="nbr_images"):
            twin.gain_accumulate(plain, src, 1.6)
    finally:
        twin.close()


def test_every_refusal_of_the_apply_contract(lib):
    twin = hb.HostDensifier(1)
    try:
        n = 10
        rgb = torch.linspace(0.0, 0.9, 3 * (n + 2)).reshape(n + 2, 3).contiguous()          # two points beyond the last offset
        out = torch.full((n + 2, 3), 7.0)
        offs = torch.tensor([0, 4, 4, n], dtype=torch.int64)
        f = torch.tensor([[2.0, 1.0, 0.5], [9.0, 9.0, 9.0], [1.0, 1.5, 0.25]], dtype=torch.float32)
        good = dict(rgb=rgb.data_ptr(), n=n + 2, off=offs.data_ptr(), refs=3, f=f.data_ptr(), out=out.data_ptr())

        def call(**kw):
            a = {**good, **kw}
            return lib.lfd_gain_apply_host(twin._ctx, a["rgb"], a["n"], a["off"], a["refs"], a["f"], a["out"])

        assert call() == 0
        want = np.minimum(rgb[:n].numpy() * np.repeat(f.numpy(), [4, 0, 6], axis=0), np.float32(1.0))
        assert np.array_equal(cs.bits(out[:n]), cs.bits(want)) and (out[n:] == 7.0).all()   # points beyond the last offset are not touched
        assert (want == 1.0).any()
        invalid = [dict(rgb=None), dict(out=None), dict(off=None), dict(f=None), dict(n=-1), dict(n=1 << 31), dict(refs=0), dict(refs=-2),
                   dict(out=rgb.data_ptr() + 4), dict(out=rgb.data_ptr() - 4), dict(out=f.data_ptr()), dict(out=offs.data_ptr())]
        for kw in invalid:
            assert call(**kw) == LFD_ERR_INVALID, kw
            assert b"lfd_gain_apply_host" in lib.lfd_last_error(twin._ctx)
        keep = rgb.clone()
        assert call(out=rgb.data_ptr()) == 0                                                # in place
        assert np.array_equal(cs.bits(rgb[:n]), cs.bits(want)) and np.array_equal(cs.bits(rgb[n:]), cs.bits(keep[n:]))
        assert call(n=0) == 0
        with pytest.raises(ValueError, match="ref_counts"):
            twin.gain_apply(keep, [3, 3], f[:2])
        with pytest.raises(ValueError, match="factors must be"):
            twin.gain_apply(keep, [6, 6], f)
    finally:
        twin.close()
