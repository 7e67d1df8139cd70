"""CPU tier of the entry points of the footprint-adaptive thinning (lfd_thin_footprint and its *_host twin): the library exports them, the header
declares them with the argument list of DESIGN.md 4.24, the binding types them, the ABI version - in the header and in the library - and the pinned
structures are unchanged, every refusal of lfd_thin_check answers with its message before anything else is looked at, the n = 0 call gives zero
outputs, and each side refuses the other's context (a host context given to the device call: LFD_ERR_STATE; the reverse is
tests/test_gpu_thin.py's)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from helpers import ROOT
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

LFD_ERR_INVALID, LFD_ERR_STATE = 1, 4
THIN_ARGS = ["lfd_context* ctx", "const float* xyz", "const float* err", "int64_t n", "const int64_t* ref_offsets_host", "int32_t n_refs",
             "const double* ref_rows_host", "double thin_cells", "int64_t* keep_out", "int64_t* n_keep_host", "int64_t* ref_offsets_out_host",
             "double* stats_host"]
NAMES = ["lfd_thin_footprint", "lfd_thin_footprint_host"]
I64P, F64P = C.POINTER(C.c_int64), C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def lib():
    return hb.load_library()


@pytest.mark.parametrize("name", NAMES)
def test_library_exports_and_header_declares(lib, name):
    assert hasattr(lib, name)
    header = open(os.path.join(ROOT, "include", "lfd_densify.h")).read()
    decl = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert decl, f"{name} is not declared in include/lfd_densify.h"
    assert [" ".join(a.split()) for a in decl.group(1).split(",")] == THIN_ARGS


def test_abi_version_and_struct_layouts_are_unchanged(lib):
    header = open(os.path.join(ROOT, "include", "lfd_densify.h")).read()
    assert re.search(r"#define\s+LFD_ABI_VERSION\s+9\b", header)
    assert lib.lfd_abi_version() == 9 == hb.LFD_ABI_VERSION
    hb.check_struct_layout(lib)
    assert C.sizeof(hb.lfd_params) == 32 and C.sizeof(hb.lfd_points) == 48 and C.sizeof(hb.lfd_batch) == 120


@pytest.mark.parametrize("name", NAMES)
def test_binding_sets_argtypes(lib, name):
    f = getattr(lib, name)
    assert f.restype is C.c_int
    assert f.argtypes is not None and len(f.argtypes) == len(THIN_ARGS)
    assert [i for i, t in enumerate(f.argtypes) if t is C.c_int64] == [3] and f.argtypes[5] is C.c_int32 and f.argtypes[7] is C.c_double
    for cls in (hb.HipDensifier, hb.HostDensifier):
        assert list(inspect.signature(cls.thin_footprint).parameters)[1:] == ["xyz", "err", "ref_counts", "ref_rows", "thin_cells"]
    assert issubclass(hb.ThinInputRefused, hb.HipBackendError) and hb.THIN_LEVELS == 21


@pytest.mark.parametrize("name", NAMES)
def test_null_context_is_invalid(lib, name):
    n_keep = C.c_int64(0)
    assert getattr(lib, name)(None, None, None, 0, None, 1, None, 2.0, None, C.byref(n_keep), None, None) == LFD_ERR_INVALID
    assert lib.lfd_last_error(None)


def test_the_other_kind_of_context_the_argument_checks_and_the_empty_call(lib):
    ctx = C.c_void_p()
    assert lib.lfd_create_host(1, C.byref(ctx)) == 0 and ctx.value
    try:
        n_keep = C.c_int64(7)
        xyz = np.random.default_rng(0).uniform(0, 1, (5, 3)).astype(np.float32)
        err = np.zeros(5, np.float32)
        keep = np.full(5, -1, np.int64)
        offs, offs_out = np.array([0, 2, 5], np.int64), np.full(3, -1, np.int64)
        rows = np.array([[0, 0, 1, 10, 0.01], [0, 1, 0, 10, 0.02]], np.float64)
        stats = np.full(43, -1.0, np.float64)
        ptr = lambda a, t=C.c_void_p: None if a is None else a.ctypes.data_as(t)      # noqa: E731

        def call(fn, xyz=xyz, err=None, n=5, offs=offs, n_refs=2, rows=rows, cells=2.0, keep=keep, n_keep=C.byref(n_keep), offs_out=offs_out, stats=None):
            return fn(ctx, ptr(xyz), ptr(err), n, ptr(offs, I64P), n_refs, ptr(rows, F64P), C.c_double(cells), ptr(keep), n_keep, ptr(offs_out, I64P),
                      ptr(stats, F64P))
        assert call(lib.lfd_thin_footprint) == LFD_ERR_STATE and b"host" in lib.lfd_last_error(ctx)
        assert call(lib.lfd_thin_footprint, n=-1, offs=None) == LFD_ERR_STATE           # the context's kind is looked at first
        # n == 0 is valid: zero outputs
        empty = np.zeros(3, np.int64)
        assert call(lib.lfd_thin_footprint_host, xyz=None, n=0, offs=empty, keep=None, stats=stats) == 0
        assert n_keep.value == 0 and offs_out.tolist() == [0, 0, 0] and stats.tolist() == [0.0] * 43
        bad_tan = [rows.copy() for _ in range(4)]
        for b, v in zip(bad_tan, (0.0, -0.01, np.inf, np.nan)):
            b[1, 4] = v
        overlap = np.zeros(20, np.float32)
        for kw, words in ((dict(offs=None), b"null ref_offsets_host / ref_offsets_out_host / n_keep_host / ref_rows_host"),
                          (dict(offs_out=None), b"null ref_offsets_host / ref_offsets_out_host / n_keep_host / ref_rows_host"),
                          (dict(n_keep=None), b"null ref_offsets_host / ref_offsets_out_host / n_keep_host / ref_rows_host"),
                          (dict(rows=None), b"null ref_offsets_host / ref_offsets_out_host / n_keep_host / ref_rows_host"),
                          (dict(n=-1), b"n must be in [0, 2^31 - 1]"), (dict(n=1 << 31), b"n must be in [0, 2^31 - 1]"),
                          (dict(n_refs=0), b"n_refs must be >= 1"),
                          (dict(xyz=None), b"null xyz / keep_out"), (dict(keep=None), b"null xyz / keep_out"),
                          (dict(offs=np.array([1, 2, 5], np.int64)), b"ref_offsets_host must start at 0 and end at n"),
                          (dict(offs=np.array([0, 2, 4], np.int64)), b"ref_offsets_host must start at 0 and end at n"),
                          (dict(offs=np.array([0, 6, 5], np.int64)), b"ref_offsets_host must not decrease"),
                          (dict(cells=0.0), b"thin_cells must be finite and > 0"), (dict(cells=-1.0), b"thin_cells must be finite and > 0"),
                          (dict(cells=float("inf")), b"thin_cells must be finite and > 0"), (dict(cells=float("nan")), b"thin_cells must be finite and > 0"),
                          (dict(rows=bad_tan[0]), b"every tan_cell must be finite and > 0"), (dict(rows=bad_tan[1]), b"every tan_cell must be finite and > 0"),
                          (dict(rows=bad_tan[2]), b"every tan_cell must be finite and > 0"), (dict(rows=bad_tan[3]), b"every tan_cell must be finite and > 0"),
                          (dict(xyz=overlap, keep=overlap[2:]), b"in and out arrays overlap"),
                          (dict(err=overlap, keep=overlap[4:]), b"in and out arrays overlap")):
            assert call(lib.lfd_thin_footprint_host, **kw) == LFD_ERR_INVALID, kw
            assert lib.lfd_last_error(ctx) == b"lfd_thin_footprint_host: " + words
        bad = xyz.copy()
        bad[3, 1] = np.nan
        assert call(lib.lfd_thin_footprint_host, xyz=bad) == LFD_ERR_INVALID
        assert lib.lfd_last_error(ctx) == b"lfd_thin_footprint_host: non-finite coordinate in the input"
        # and a plain call still works behind the refusals: five distinct points, all kept
        assert call(lib.lfd_thin_footprint_host, err=err, cells=1e-9, stats=stats) == 0
        assert n_keep.value == 5 and keep.tolist() == [0, 1, 2, 3, 4] and offs_out.tolist() == [0, 2, 5] and stats[20] == 5 and stats[41] == 5
    finally:
        lib.lfd_destroy(ctx)
