"""CPU tier of the depth-map renderer's entry points (lfd_render_depth / lfd_render_depth_host): the library exports them, the header declares
them with the argument list of DESIGN.md 4.22, the binding types them, the ABI version and the pinned structures are unchanged, every refusal of
the contract answers LFD_ERR_INVALID with its message and writes nothing, the inputs stay untouched, and a context of the wrong kind is refused."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import depth_ref as dr
from helpers import ROOT
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

LFD_ERR_INVALID, LFD_ERR_STATE = 1, 4
ARGS = ["lfd_context* ctx", "const float* xyz", "int64_t n", "const float* normals", "const float* cam_P_host", "const int32_t* cam_wh_host",
        "int32_t n_cams", "int32_t pw", "int32_t ph", "int32_t splat_cells", "int32_t window_cells", "float tol", "int32_t cams_per_batch",
        "float* depth_out", "int32_t* index_out", "float* normal_out"]
NAMES = ["lfd_render_depth", "lfd_render_depth_host"]
NULL_CALL = (None, 0, None, None, None, 1, 1, 1, 1, 3, 0.02, 0, None, None, None)


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
    assert [i for i, t in enumerate(f.argtypes) if t is C.c_int64] == [2] and [i for i, t in enumerate(f.argtypes) if t is C.c_int32] == [6, 7, 8, 9, 10, 12]
    for cls in (hb.HipDensifier, hb.HostDensifier):
        sig = inspect.signature(cls.render_depth).parameters
        assert list(sig)[1:] == ["xyz", "normals", "cam_P", "cam_wh", "plane", "splat_cells", "window_cells", "tol", "with_index", "cams_per_batch"]
        assert (sig["splat_cells"].default, sig["window_cells"].default, sig["tol"].default, sig["cams_per_batch"].default) == (1, 3, 0.02, 0)


@pytest.mark.parametrize("name", NAMES)
def test_null_context_is_invalid(lib, name):
    assert getattr(lib, name)(None, *NULL_CALL) == LFD_ERR_INVALID
    assert lib.lfd_last_error(None)


def test_host_context_is_refused_by_the_device_call(lib):
    ctx = C.c_void_p()
    assert lib.lfd_create_host(1, C.byref(ctx)) == 0 and ctx.value
    try:
        assert lib.lfd_render_depth(ctx, *NULL_CALL) == LFD_ERR_STATE
        assert b"host" in lib.lfd_last_error(ctx)
        assert lib.lfd_render_depth_host(ctx, *NULL_CALL) == LFD_ERR_INVALID                # its own entry point looks at the arguments
        assert b"lfd_render_depth_host" in lib.lfd_last_error(ctx)
    finally:
        lib.lfd_destroy(ctx)


def test_every_refusal_of_the_contract(lib):
    twin = hb.HostDensifier(1)
    try:
        n, pw, ph = 300, 9, 7
        xyz, normals, P, wh = dr.random_scene(n, 2)
        cells = 3 * pw * ph
        depth = np.full(cells + 1, 7.0, np.float32)                        # one guard element behind each output
        index = np.full(cells + 1, -7, np.int32)
        normal = np.full(3 * cells + 1, 7.0, np.float32)
        f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        p = lambda a: a.ctypes.data                                         # noqa: E731
        good = dict(xyz=p(xyz), n=n, nrm=p(normals), P=P, wh=wh, n_cams=3, pw=pw, ph=ph, r=1, R=3, tol=0.02, per=0, do=p(depth), io=p(index),
                    no=p(normal))

        def call(**kw):
            a = {**good, **kw}
            cp = a["P"].ctypes.data_as(f32p) if a["P"] is not None else None
            cw = a["wh"].ctypes.data_as(i32p) if a["wh"] is not None else None
            return lib.lfd_render_depth_host(twin._ctx, a["xyz"], a["n"], a["nrm"], cp, cw, a["n_cams"], a["pw"], a["ph"], a["r"], a["R"],
                                             C.c_float(a["tol"]), a["per"], a["do"], a["io"], a["no"])

        def untouched():
            return (depth == 7.0).all() and (index == -7).all() and (normal == 7.0).all()

        nan_P, inf_P, zero_wh, neg_wh = P.copy(), P.copy(), wh.copy(), wh.copy()
        nan_P[1, 5], inf_P[2, 11], zero_wh[0, 1], neg_wh[2, 0] = np.nan, np.inf, 0, -4
        invalid = [(dict(P=None), "null cam_P_host"), (dict(wh=None), "null cam_P_host"), (dict(do=None), "null depth_out"),
                   (dict(xyz=None), "null xyz"), (dict(nrm=None), "both be given"), (dict(no=None), "both be given"),
                   (dict(n=-1), "n must be"), (dict(n=1 << 31), "n must be"), (dict(n_cams=0), "n_cams"), (dict(n_cams=-3), "n_cams"),
                   (dict(pw=0), "at least 1 x 1"), (dict(ph=0), "at least 1 x 1"), (dict(pw=-8), "at least 1 x 1"),
                   (dict(wh=zero_wh), "image size"), (dict(wh=neg_wh), "image size"),
                   (dict(pw=1 << 15, ph=1 << 15), "2^31 - 1 cells"), (dict(pw=(1 << 31) - 1, ph=1), "2^31 - 1 cells"),
                   (dict(pw=26755, ph=26755), "2^31 - 1 cells"),
                   (dict(P=nan_P), "not finite"), (dict(P=inf_P), "not finite"),
                   (dict(r=-1), "splat_cells"), (dict(r=4), "splat_cells"), (dict(R=-1), "window_cells"), (dict(R=9), "window_cells"),
                   (dict(tol=0.0), "tol"), (dict(tol=1.0), "tol"), (dict(tol=-0.02), "tol"), (dict(tol=float("nan")), "tol"),
                   (dict(tol=float("inf")), "tol"), (dict(per=-1), "cams_per_batch"),
                   (dict(do=p(xyz)), "overlap"), (dict(io=p(xyz) + 12 * (n - 1)), "overlap"), (dict(no=p(normals) + 4), "overlap"),
                   (dict(do=p(normals)), "overlap"), (dict(io=p(depth) + 8), "overlap each other"), (dict(no=p(index)), "overlap each other")]
        before = [a.copy() for a in (xyz, normals, P, wh)]
        for kw, message in invalid:
            assert call(**kw) == LFD_ERR_INVALID, kw
            error = lib.lfd_last_error(twin._ctx)
            assert error.startswith(b"lfd_render_depth_host: ") and message.encode() in error, (kw, error)
            assert untouched(), kw                                          # a refused call writes nothing
        assert call() == 0
        assert (depth[:cells] != 7.0).all() and (index[:cells] != -7).all() and (normal[:3 * cells] != 7.0).all()
        assert depth[cells] == 7.0 and index[cells] == -7 and normal[3 * cells] == 7.0          # ... and a good one nothing behind its outputs
        want = dr.render(xyz, normals, P, wh, pw, ph, 1, 3, 0.02)
        dr.assert_equal((depth[:cells].reshape(3, ph, pw), index[:cells].reshape(3, ph, pw), normal[:3 * cells].reshape(3, ph, pw, 3)), want)
        for a, b in zip((xyz, normals, P, wh), before):                     # the inputs are read only
            assert a.tobytes() == b.tobytes()
        assert call(io=None) == 0 and call(nrm=None, no=None) == 0 and call(nrm=None, no=None, io=None) == 0      # the optional arrays
        assert call(n=0, xyz=None) == 0 and not depth[:cells].any() and (index[:cells] == -1).all() and not normal[:3 * cells].any()
        assert call(per=1) == 0 and call(per=1000) == 0 and call(r=0, R=0) == 0 and call(r=3, R=8) == 0
        with pytest.raises(hb.HipBackendError, match="window_cells"):
            twin.render_depth(torch.from_numpy(xyz), None, P, wh, (8, 6), 1, 9)
        with pytest.raises(ValueError, match="one camera each"):
            twin.render_depth(torch.from_numpy(xyz), None, P, wh[:2], (8, 6))
        with pytest.raises(ValueError, match="normals"):
            twin.render_depth(torch.from_numpy(xyz), torch.from_numpy(normals[:10]), P, wh, (8, 6))
        with pytest.raises(ValueError, match="2\\^31 - 1 cells"):
            twin.render_depth(torch.from_numpy(xyz), None, P, wh, (1 << 15, 1 << 15))
    finally:
        twin.close()
