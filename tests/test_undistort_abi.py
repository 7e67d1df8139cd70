"""CPU tier of the image undistortion's entry points (lfd_undistort_image / lfd_host_undistort_image): the library exports them, the header
declares them with the argument lists of DESIGN.md 4.13, the binding types them, the ABI version and the pinned structures are unchanged, every
refusal of the contract answers LFD_ERR_INVALID, and a host context given to the device call is refused with LFD_ERR_STATE (what a device
context refuses is tests/test_gpu_undistort.py's)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from helpers import ROOT
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

LFD_ERR_INVALID, LFD_ERR_STATE = 1, 4
HOST_ARGS = ["const uint8_t* src", "int32_t w", "int32_t h", "int32_t channels", "int32_t nearest", "const double intr[4]", "const double dist[8]",
             "uint8_t* dst", "uint8_t* valid255", "int64_t* n_invalid_host"]
ARGS = {"lfd_undistort_image": ["lfd_context* ctx"] + HOST_ARGS, "lfd_host_undistort_image": HOST_ARGS}


@pytest.fixture(scope="module")
def lib():
    return hb.load_library()


@pytest.mark.parametrize("name", list(ARGS))
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


@pytest.mark.parametrize("name", list(ARGS))
def test_binding_sets_argtypes(lib, name):
    f = getattr(lib, name)
    assert f.restype is C.c_int
    types = list(f.argtypes)
    assert len(types) == len(ARGS[name])
    types = types[1:] if name == "lfd_undistort_image" else types
    assert types[1:5] == [C.c_int32] * 4 and types[5] is types[6] and types[5]._type_ is C.c_double and types[9]._type_ is C.c_int64
    sig = inspect.signature(hb.HipDensifier.undistort_image).parameters
    assert list(sig)[1:] == ["src", "distortion", "nearest", "with_valid", "count", "workspace"]
    assert list(inspect.signature(hb.host_undistort_image).parameters) == ["src", "distortion", "nearest", "with_valid"]
    assert not hasattr(hb.HostDensifier, "undistort_image")            # the twin needs no context: a module-level function


def test_null_context_and_host_context_are_refused_by_the_device_call(lib):
    src, dst = np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4, 3), np.uint8)
    intr, dist = (C.c_double * 4)(10.0, 10.0, 2.0, 2.0), (C.c_double * 8)()
    assert lib.lfd_undistort_image(None, src.ctypes.data, 4, 4, 3, 0, intr, dist, dst.ctypes.data, None, None) == LFD_ERR_INVALID
    ctx = C.c_void_p()
    assert lib.lfd_create_host(1, C.byref(ctx)) == 0 and ctx.value
    try:
        assert lib.lfd_undistort_image(ctx, src.ctypes.data, 4, 4, 3, 0, intr, dist, dst.ctypes.data, None, None) == LFD_ERR_STATE
        assert b"host" in lib.lfd_last_error(ctx)
    finally:
        lib.lfd_destroy(ctx)


def test_every_refusal_of_the_contract(lib):
    w, h = 12, 10
    src = np.random.default_rng(0).integers(0, 256, (h, w, 3), dtype=np.uint8)
    big = np.zeros(4 * w * h * 3, np.uint8)                             # room for overlapping placements
    dst, valid = np.zeros_like(src), np.zeros((h, w), np.uint8)
    n_bad = C.c_int64(-1)
    good = dict(src=src.ctypes.data, w=w, h=h, ch=3, nearest=0, intr=(40.0, 41.0, 6.5, 4.5), dist=(0.05, 0, 0, 0, 0, 0, 0, 0), dst=dst.ctypes.data,
                valid=valid.ctypes.data, n=C.byref(n_bad))

    def call(**kw):
        a = {**good, **kw}
        intr = (C.c_double * 4)(*a["intr"]) if a["intr"] is not None else None
        dist = (C.c_double * 8)(*a["dist"]) if a["dist"] is not None else None
        return lib.lfd_host_undistort_image(a["src"], a["w"], a["h"], a["ch"], a["nearest"], intr, dist, a["dst"], a["valid"], a["n"])

    before = src.copy()
    assert call() == 0 and n_bad.value == 0 and np.array_equal(src, before)             # the input is read only
    assert call(valid=None, n=None) == 0 and call(ch=1) == 0 and call(nearest=1) == 0 and call(nearest=7) == 0
    inf, nan = float("inf"), float("nan")
    base = big.ctypes.data
    invalid = [dict(src=None), dict(dst=None), dict(intr=None), dict(dist=None),
               dict(w=0), dict(h=0), dict(w=-3), dict(h=-1), dict(w=1 << 16, h=1 << 15), dict(w=(1 << 31) - 1, h=2),
               dict(ch=0), dict(ch=2), dict(ch=4), dict(ch=-1),
               dict(intr=(0.0, 41.0, 6.5, 4.5)), dict(intr=(40.0, -1.0, 6.5, 4.5)), dict(intr=(inf, 41.0, 6.5, 4.5)), dict(intr=(40.0, nan, 6.5, 4.5)),
               dict(intr=(40.0, 41.0, inf, 4.5)), dict(intr=(40.0, 41.0, 6.5, nan))]
    invalid += [dict(dist=tuple(bad if e == k else 0.0 for e in range(8))) for k in range(8) for bad in (inf, nan)]
    invalid += [dict(src=base, dst=base), dict(src=base, dst=base + w * h * 3 - 1), dict(src=base + 5, dst=base),          # src and dst overlap
                dict(src=base, dst=base + w * h * 3, valid=base + w * h * 3 - 1),                                             # valid255 and src
                dict(src=base, dst=base + w * h * 3, valid=base + 2 * w * h * 3 - 1)]                                         # valid255 and dst
    for kw in invalid:
        n_bad.value = -1
        assert call(**kw) == LFD_ERR_INVALID, kw
        assert n_bad.value == -1, kw                                     # nothing was written
    assert call(src=base, dst=base + w * h * 3, valid=base + 2 * w * h * 3) == 0           # adjacent is not overlapping
