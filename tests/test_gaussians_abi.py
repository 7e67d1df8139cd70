"""CPU tier of the entry points of the Gaussian-ready output (lfd_knn_dist2 / lfd_pack_gaussians and their *_host twins): the library exports
them, the header declares them with the argument lists of DESIGN.md 4.17, the binding types them, the ABI version and the pinned structures are
unchanged, every refusal of the contract answers LFD_ERR_INVALID with a message - the three data refusals in words the binding turns into
KnnInputRefused -, a context of the wrong kind is refused (a host context given to the device calls: LFD_ERR_STATE; the reverse is
tests/test_gpu_gaussians.py's), and the inputs are bitwise untouched."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from helpers import ROOT
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from lichtfeld_densification_plugin_amd.core import writers

LFD_ERR_INVALID, LFD_ERR_STATE = 1, 4
KNN_ARGS = ["lfd_context* ctx", "const float* xyz", "int64_t n", "double cell_size", "float* dist2_out", "double* stats_host"]
PACK_ARGS = ["lfd_context* ctx", "const float* xyz", "const float* normals", "const float* rgb", "const float* dist2", "int64_t n",
             "float opacity_logit", "double log_flatten", "double max_scale", "uint8_t* out"]
ARGS = {"lfd_knn_dist2": KNN_ARGS, "lfd_knn_dist2_host": KNN_ARGS, "lfd_pack_gaussians": PACK_ARGS, "lfd_pack_gaussians_host": PACK_ARGS}
KNN_NULL = (None, 0, 0.0, None, None)
PACK_NULL = (None, None, None, None, 0, 0.0, 0.0, 0.0, None)


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
    doubles, floats = ([3], []) if "knn" in name else ([7, 8], [6])
    assert [i for i, t in enumerate(f.argtypes) if t is C.c_double] == doubles and [i for i, t in enumerate(f.argtypes) if t is C.c_float] == floats
    for cls in (hb.HipDensifier, hb.HostDensifier):
        sig = inspect.signature(cls.knn_dist2).parameters
        assert list(sig)[1:] == ["xyz", "cell_size"] and sig["cell_size"].default == 0.0
        sig = inspect.signature(cls.pack_gaussians).parameters
        assert list(sig)[1:] == ["xyz", "normals", "rgb", "dist2", "opacity", "flatten", "max_scale"]
        assert (sig["opacity"].default, sig["flatten"].default, sig["max_scale"].default) == (0.1, 1.0, 0.0)
    assert issubclass(hb.KnnInputRefused, hb.HipBackendError)


@pytest.mark.parametrize("name", sorted(ARGS))
def test_null_context_is_invalid(lib, name):
    assert getattr(lib, name)(None, *(KNN_NULL if "knn" in name else PACK_NULL)) == LFD_ERR_INVALID
    assert lib.lfd_last_error(None)


def test_host_context_is_refused_by_the_device_calls(lib):
    ctx = C.c_void_p()
    assert lib.lfd_create_host(1, C.byref(ctx)) == 0 and ctx.value
    try:
        assert lib.lfd_knn_dist2(ctx, *KNN_NULL) == LFD_ERR_STATE and b"host" in lib.lfd_last_error(ctx)
        assert lib.lfd_pack_gaussians(ctx, *PACK_NULL) == LFD_ERR_STATE and b"host" in lib.lfd_last_error(ctx)
        assert lib.lfd_knn_dist2_host(ctx, *KNN_NULL) == 0                               # n == 0 is valid
        assert lib.lfd_pack_gaussians_host(ctx, *PACK_NULL) == 0
        assert lib.lfd_knn_dist2_host(ctx, None, 5, 0.0, None, None) == LFD_ERR_INVALID    # its own entry point looks at the arguments
        assert b"lfd_knn_dist2_host" in lib.lfd_last_error(ctx)
    finally:
        lib.lfd_destroy(ctx)


def test_every_refusal_of_the_contract(lib):
    twin = hb.HostDensifier(1)
    try:
        rng = np.random.default_rng(0)
        n = 300
        xyz = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
        out = np.zeros(n, np.float32)
        stats = (C.c_double * 4)(-1, -1, -1, -1)
        p = lambda a: a.ctypes.data                                         # noqa: E731
        good = dict(xyz=p(xyz), n=n, h=0.0, out=p(out), stats=stats)

        def call(**kw):
            a = {**good, **kw}
            return lib.lfd_knn_dist2_host(twin._ctx, a["xyz"], a["n"], C.c_double(a["h"]), a["out"], a["stats"])

        before = xyz.copy()
        assert call() == 0 and stats[0] > 0 and 1 <= stats[1] <= n and 1 <= stats[2] <= n and 0 <= stats[3] <= n and (out > 0).all()
        assert xyz.tobytes() == before.tobytes()                             # the input is read only
        first = out.copy()
        assert call(stats=None) == 0 and out.tobytes() == first.tobytes()    # the optional array
        assert call(h=0.37) == 0 and out.tobytes() == first.tobytes() and stats[0] == 0.37
        assert call(n=0, xyz=None, out=None) == 0 and list(stats) == [0.0, 0.0, 0.0, 0.0]
        for kw in (dict(xyz=None), dict(out=None), dict(n=-1), dict(n=1 << 31), dict(h=-0.5), dict(h=float("inf")), dict(h=float("nan")),
                   dict(out=p(xyz)), dict(out=p(xyz) + 12 * n - 4)):
            assert call(**kw) == LFD_ERR_INVALID, kw
            msg = lib.lfd_last_error(twin._ctx)
            assert msg.startswith(b"lfd_knn_dist2_host: "), kw
            assert b"key range" not in msg and b"non-finite coordinate" not in msg and b"fewer than four points" not in msg
        # the three data refusals, decided before anything is sorted, in words of their own
        for k in (1, 2, 3):
            assert call(n=k) == LFD_ERR_INVALID and b"fewer than four points" in lib.lfd_last_error(twin._ctx)
        for value in (np.nan, np.inf, -np.inf):
            bad = xyz.copy()
            bad[17, 2] = value
            assert call(xyz=p(bad)) == LFD_ERR_INVALID and b"non-finite coordinate" in lib.lfd_last_error(twin._ctx)
        assert call(h=1e-12) == LFD_ERR_INVALID and b"key range" in lib.lfd_last_error(twin._ctx)
        assert call(h=3e-8) == LFD_ERR_INVALID and b"key range" in lib.lfd_last_error(twin._ctx)
        line = np.zeros((n, 3), np.float32)
        line[:, 0] = np.linspace(-3.0e38, 3.0e38, n)
        assert call(xyz=p(line), h=1.0) == LFD_ERR_INVALID and b"key range" in lib.lfd_last_error(twin._ctx)
        assert call(xyz=p(line)) == 0 and np.isinf(out).all()                # the automatic size keys any finite cloud; its d2 overflow f32, as brute force's do
        assert call() == 0 and out.tobytes() == first.tobytes()              # and the context still works

        # lfd_pack_gaussians_host
        nrm, rgb, d2 = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.ones(n, np.float32)
        body = np.zeros(68 * n + 4, np.uint8)
        gp = dict(xyz=p(xyz), nrm=p(nrm), rgb=p(rgb), d2=p(d2), n=n, op=-2.0, lf=0.0, ms=0.0, out=p(body))

        def pack(**kw):
            a = {**gp, **kw}
            return lib.lfd_pack_gaussians_host(twin._ctx, a["xyz"], a["nrm"], a["rgb"], a["d2"], a["n"], C.c_float(a["op"]), C.c_double(a["lf"]),
                                               C.c_double(a["ms"]), a["out"])
        assert pack() == 0 and body[68 * n:].tobytes() == b"\0\0\0\0"        # nothing behind the n records
        for kw in (dict(xyz=None), dict(nrm=None), dict(rgb=None), dict(d2=None), dict(out=None), dict(n=-1), dict(n=1 << 31), dict(op=float("nan")),
                   dict(op=float("inf")), dict(lf=0.1), dict(lf=float("nan")), dict(lf=float("-inf")), dict(ms=-1.0), dict(ms=float("inf")),
                   dict(ms=float("nan")), dict(out=p(body) + 1)):
            assert pack(**kw) == LFD_ERR_INVALID, kw
            assert lib.lfd_last_error(twin._ctx).startswith(b"lfd_pack_gaussians_host: "), kw
    finally:
        twin.close()


def test_the_header_of_the_file_and_the_numpy_records():
    head = writers.gaussian_ply_header(12345).decode("ascii")
    lines = head.split("\n")
    assert lines[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 12345"] and lines[-2:] == ["end_header", ""]
    assert lines[3:-2] == [f"property float {p}" for p in
                           ("x y z nx ny nz f_dc_0 f_dc_1 f_dc_2 opacity scale_0 scale_1 scale_2 rot_0 rot_1 rot_2 rot_3").split()]
    assert writers._GAUSS_REC.itemsize == 68
    import knn_ref as kr
    import test_knn_host as th
    xyz, nrm, rgb, d2 = th.make_inputs(9, 400)
    for knobs in (dict(), dict(opacity=0.4, flatten=0.3, max_scale=0.2)):
        assert writers.gaussian_records(xyz, nrm, rgb, d2, **knobs).tobytes() == kr.gaussian_records_ref(xyz, nrm, rgb, d2, **knobs).tobytes()
    with pytest.raises(ValueError, match="68 bytes per vertex"):
        writers.write_gaussian_ply_packed(os.devnull, 3, b"\0" * 67)
