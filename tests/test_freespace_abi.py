"""CPU tier of the free-space filter's entry points (lfd_freespace_filter / lfd_freespace_filter_host): the library exports them, the header
declares them with the argument list of DESIGN.md 4.15, the binding types them, the ABI version and the pinned structures are unchanged, every
refusal of the contract answers LFD_ERR_INVALID with a message, the inputs stay untouched, and a context of the wrong kind is refused (a host
context given to the device call: LFD_ERR_STATE; the reverse is tests/test_gpu_freespace.py's)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import freespace_scene as fs
from helpers import ROOT
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

LFD_ERR_INVALID, LFD_ERR_STATE = 1, 4
ARGS = ["lfd_context* ctx", "const float* xyz", "const float* rgb", "const float* err", "int64_t n", "const int64_t* ref_offsets_host",
        "int32_t n_refs", "const float* cam_P_host", "const int32_t* cam_wh_host", "int32_t pw", "int32_t ph", "float tol",
        "int32_t min_violations", "float* xyz_out", "float* rgb_out", "float* err_out", "int64_t* ref_offsets_out_host", "uint8_t* violations",
        "uint8_t* supports", "int64_t* n_out_host"]
NAMES = ["lfd_freespace_filter", "lfd_freespace_filter_host"]
NULL_CALL = (None, None, None, 0, None, 1, None, None, 1, 1, 0.02, 1, None, None, None, None, None, None, None)


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
    assert [i for i, t in enumerate(f.argtypes) if t is C.c_float] == [11]
    assert [i for i, t in enumerate(f.argtypes) if t is C.c_int64] == [4] and [i for i, t in enumerate(f.argtypes) if t is C.c_int32] == [6, 9, 10, 12]
    for cls in (hb.HipDensifier, hb.HostDensifier):
        sig = inspect.signature(cls.freespace_filter).parameters
        assert list(sig)[1:] == ["xyz", "rgb", "err", "ref_counts", "cam_P", "cam_wh", "plane", "tol", "min_violations", "with_counts"]
        assert sig["with_counts"].default is False


@pytest.mark.parametrize("name", NAMES)
def test_null_context_is_invalid(lib, name):
    assert getattr(lib, name)(None, *NULL_CALL) == LFD_ERR_INVALID
    assert lib.lfd_last_error(None)


def test_host_context_is_refused_by_the_device_call(lib):
    ctx = C.c_void_p()
    assert lib.lfd_create_host(1, C.byref(ctx)) == 0 and ctx.value
    try:
        assert lib.lfd_freespace_filter(ctx, *NULL_CALL) == LFD_ERR_STATE
        assert b"host" in lib.lfd_last_error(ctx)
        assert lib.lfd_freespace_filter_host(ctx, *NULL_CALL) == LFD_ERR_INVALID            # its own entry point looks at the arguments
        assert b"lfd_freespace_filter_host" in lib.lfd_last_error(ctx)
    finally:
        lib.lfd_destroy(ctx)


def test_every_refusal_of_the_contract(lib):
    twin = hb.HostDensifier(1)
    try:
        n = 300
        xyz, _counts, P, wh = fs.ring_cloud(3, n, 2)
        rng = np.random.default_rng(0)
        rgb = rng.uniform(0, 1, (n, 3)).astype(np.float32)
        err = rng.uniform(0, 1, (n,)).astype(np.float32)
        xo, ro, eo = np.zeros_like(xyz), np.zeros_like(rgb), np.zeros_like(err)
        viol, supp = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        offs = np.array([0, 100, 100, 300], np.int64)
        offs_out = np.full(4, -1, np.int64)
        n_out = C.c_int64(-1)
        i64p, f32p, i32p = C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_int32)
        p = lambda a: a.ctypes.data                                         # noqa: E731
        good = dict(xyz=p(xyz), rgb=p(rgb), err=p(err), n=n, offs=offs, n_refs=3, P=P, wh=wh, pw=96, ph=62, tol=0.02, m=1, xo=p(xo), ro=p(ro),
                    eo=p(eo), offs_out=offs_out, viol=p(viol), supp=p(supp), n_out=C.byref(n_out))

        def call(**kw):
            a = {**good, **kw}
            o = a["offs"].ctypes.data_as(i64p) if a["offs"] is not None else None
            oo = a["offs_out"].ctypes.data_as(i64p) if a["offs_out"] is not None else None
            cp = a["P"].ctypes.data_as(f32p) if a["P"] is not None else None
            cw = a["wh"].ctypes.data_as(i32p) if a["wh"] is not None else None
            return lib.lfd_freespace_filter_host(twin._ctx, a["xyz"], a["rgb"], a["err"], a["n"], o, a["n_refs"], cp, cw, a["pw"], a["ph"],
                                                 C.c_float(a["tol"]), a["m"], a["xo"], a["ro"], a["eo"], oo, a["viol"], a["supp"], a["n_out"])

        before = [a.copy() for a in (xyz, rgb, err, offs, P, wh)]
        assert call() == 0 and 0 < n_out.value < n and offs_out[0] == 0 and offs_out[3] == n_out.value and offs_out[1] == offs_out[2]
        dropped = (viol >= 1) & (viol > supp)
        assert int((~dropped).sum()) == n_out.value
        for a, b in zip((xyz, rgb, err, offs, P, wh), before):             # the inputs are read only
            assert a.tobytes() == b.tobytes()
        assert call(rgb=None, ro=None, err=None, eo=None, viol=None, supp=None) == 0         # the optional arrays
        assert call(viol=None) == 0 and call(supp=None) == 0                                # each count output on its own
        assert call(m=255) == 0 and n_out.value == n
        assert call(n=0, offs=np.zeros(4, np.int64), xyz=None, xo=None, rgb=None, ro=None, err=None, eo=None, viol=None, supp=None) == 0
        assert n_out.value == 0 and not offs_out.any()
        nan_P, inf_P, zero_wh = P.copy(), P.copy(), wh.copy()
        nan_P[1, 5], inf_P[2, 11], zero_wh[0, 1] = np.nan, np.inf, 0
        neg_wh = wh.copy()
        neg_wh[2, 0] = -4
        invalid = [dict(offs=None), dict(offs_out=None), dict(n_out=None), dict(xyz=None), dict(xo=None), dict(P=None), dict(wh=None),
                   dict(rgb=None), dict(ro=None), dict(err=None), dict(eo=None),              # half of an optional pair
                   dict(n=-1), dict(n=1 << 31, offs=np.array([0, 100, 100, 1 << 31], np.int64)),
                   dict(n_refs=0), dict(n_refs=-3),
                   dict(offs=np.array([1, 100, 100, 300], np.int64)), dict(offs=np.array([0, 100, 100, 299], np.int64)),
                   dict(offs=np.array([0, 200, 100, 300], np.int64)), dict(offs=np.array([0, -5, 100, 300], np.int64)),
                   dict(pw=0), dict(ph=0), dict(pw=-8), dict(wh=zero_wh), dict(wh=neg_wh),
                   dict(pw=1 << 15, ph=1 << 15), dict(pw=(1 << 31) - 1, ph=1), dict(pw=26755, ph=26755),     # 3 pw ph beyond 2^31 - 1
                   dict(P=nan_P), dict(P=inf_P),
                   dict(tol=0.0), dict(tol=1.0), dict(tol=-0.02), dict(tol=1.5), dict(tol=float("nan")), dict(tol=float("inf")),
                   dict(m=0), dict(m=-1), dict(m=256),
                   dict(xo=p(xyz)), dict(xo=p(xyz) + 12 * (n - 1)), dict(ro=p(rgb)), dict(eo=p(err)), dict(viol=p(err)), dict(supp=p(xyz) + 7),
                   dict(xo=p(rgb)), dict(eo=p(xyz))]
        for kw in invalid:
            assert call(**kw) == LFD_ERR_INVALID, kw
            assert lib.lfd_last_error(twin._ctx).startswith(b"lfd_freespace_filter_host: "), kw
        assert call(pw=26754, ph=26754, n=0, offs=np.zeros(4, np.int64)) == 0                # 3 pw ph = 2^31 - 1 - 100 099: the largest legal planes
        with pytest.raises(hb.HipBackendError, match="min_violations"):
            twin.freespace_filter(torch.from_numpy(xyz), None, None, [100, 0, 200], P, wh, (8, 6), 0.02, 256)
        with pytest.raises(ValueError, match="ref_counts"):
            twin.freespace_filter(torch.from_numpy(xyz), None, None, [100, 0, 199], P, wh, (8, 6), 0.02, 1)
        with pytest.raises(ValueError, match="one camera per reference"):
            twin.freespace_filter(torch.from_numpy(xyz), None, None, [100, 0, 200], P[:2], wh[:2], (8, 6), 0.02, 1)
        with pytest.raises(ValueError, match="rgb"):
            twin.freespace_filter(torch.from_numpy(xyz), torch.from_numpy(rgb[:10]), None, [100, 0, 200], P, wh, (8, 6), 0.02, 1)
    finally:
        twin.close()
