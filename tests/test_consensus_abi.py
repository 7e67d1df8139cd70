"""CPU tier of the consensus filter's entry points (lfd_consensus_filter / lfd_consensus_filter_host): the library exports them, the header
declares them with the argument list of DESIGN.md 4.12, the binding types them, the ABI version and the pinned structures are unchanged, every
refusal of the contract answers LFD_ERR_INVALID with a message - the key-range one in words the binding turns into ConsensusInputRefused - and a
context of the wrong kind is refused (a host context given to the device call: LFD_ERR_STATE; the reverse is tests/test_gpu_consensus.py's)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from helpers import ROOT
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

LFD_ERR_INVALID, LFD_ERR_STATE = 1, 4
ARGS = ["lfd_context* ctx", "const float* xyz", "const float* rgb", "const float* err", "int64_t n", "const int64_t* ref_offsets_host",
        "int32_t n_refs", "float radius", "int32_t min_refs", "float* xyz_out", "float* rgb_out", "float* err_out",
        "int64_t* ref_offsets_out_host", "uint8_t* consensus", "int64_t* n_out_host"]
NAMES = ["lfd_consensus_filter", "lfd_consensus_filter_host"]
NULL_CALL = (None, None, None, 0, None, 1, 1.0, 1, None, None, None, None, None, None)


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
    assert re.search(r"#define\s+LFD_CONSENSUS_CAP\s+8\b", header) and hb.LFD_CONSENSUS_CAP == 8


def test_abi_version_and_struct_layouts_are_unchanged(lib):
    assert lib.lfd_abi_version() == 9 == hb.LFD_ABI_VERSION
    hb.check_struct_layout(lib)
    assert C.sizeof(hb.lfd_params) == 32 and C.sizeof(hb.lfd_points) == 48 and C.sizeof(hb.lfd_batch) == 120


@pytest.mark.parametrize("name", NAMES)
def test_binding_sets_argtypes(lib, name):
    f = getattr(lib, name)
    assert f.restype is C.c_int
    assert f.argtypes is not None and len(f.argtypes) == len(ARGS)
    assert [i for i, t in enumerate(f.argtypes) if t is C.c_float] == [7]
    assert [i for i, t in enumerate(f.argtypes) if t is C.c_int64] == [4] and [i for i, t in enumerate(f.argtypes) if t is C.c_int32] == [6, 8]
    for cls in (hb.HipDensifier, hb.HostDensifier):
        sig = inspect.signature(cls.consensus_filter).parameters
        assert list(sig)[1:] == ["xyz", "rgb", "err", "ref_counts", "radius", "min_refs", "with_consensus"] and sig["with_consensus"].default is False
    assert issubclass(hb.ConsensusInputRefused, hb.HipBackendError)


@pytest.mark.parametrize("name", NAMES)
def test_null_context_is_invalid(lib, name):
    assert getattr(lib, name)(None, *NULL_CALL) == LFD_ERR_INVALID
    assert lib.lfd_last_error(None)


def test_host_context_is_refused_by_the_device_call(lib):
    ctx = C.c_void_p()
    assert lib.lfd_create_host(1, C.byref(ctx)) == 0 and ctx.value
    try:
        assert lib.lfd_consensus_filter(ctx, *NULL_CALL) == LFD_ERR_STATE
        assert b"host" in lib.lfd_last_error(ctx)
        assert lib.lfd_consensus_filter_host(ctx, *NULL_CALL) == LFD_ERR_INVALID            # its own entry point looks at the arguments
        assert b"lfd_consensus_filter_host" in lib.lfd_last_error(ctx)
    finally:
        lib.lfd_destroy(ctx)


def test_every_refusal_of_the_contract(lib):
    twin = hb.HostDensifier(1)
    try:
        rng = np.random.default_rng(0)
        n = 300
        xyz = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
        rgb = rng.uniform(0, 1, (n, 3)).astype(np.float32)
        err = rng.uniform(0, 1, (n,)).astype(np.float32)
        xo, ro, eo = np.zeros_like(xyz), np.zeros_like(rgb), np.zeros_like(err)
        cons = np.zeros(n, np.uint8)
        offs = np.array([0, 100, 100, 300], np.int64)
        offs_out = np.full(4, -1, np.int64)
        n_out = C.c_int64(-1)
        i64p = C.POINTER(C.c_int64)
        p = lambda a: a.ctypes.data                                         # noqa: E731
        good = dict(xyz=p(xyz), rgb=p(rgb), err=p(err), n=n, offs=offs, n_refs=3, radius=0.2, m=1, xo=p(xo), ro=p(ro), eo=p(eo), offs_out=offs_out,
                    cons=p(cons), n_out=C.byref(n_out))

        def call(**kw):
            a = {**good, **kw}
            o = a["offs"].ctypes.data_as(i64p) if a["offs"] is not None else None
            oo = a["offs_out"].ctypes.data_as(i64p) if a["offs_out"] is not None else None
            return lib.lfd_consensus_filter_host(twin._ctx, a["xyz"], a["rgb"], a["err"], a["n"], o, a["n_refs"], a["radius"], a["m"], a["xo"],
                                                 a["ro"], a["eo"], oo, a["cons"], a["n_out"])

        before = xyz.copy()
        assert call() == 0 and 0 < n_out.value < n and offs_out[0] == 0 and offs_out[3] == n_out.value and offs_out[1] == offs_out[2]
        assert int((cons >= 1).sum()) == n_out.value and np.array_equal(xyz, before)        # the input is read only
        assert call(rgb=None, ro=None, err=None, eo=None, cons=None) == 0                    # the optional arrays
        assert call(m=8) == 0 and n_out.value == 0 and not offs_out.any()
        assert call(n=0, offs=np.zeros(4, np.int64), xyz=None, xo=None, rgb=None, ro=None, err=None, eo=None, cons=None) == 0 and n_out.value == 0
        invalid = [dict(offs=None), dict(offs_out=None), dict(n_out=None), dict(xyz=None), dict(xo=None),
                   dict(rgb=None), dict(ro=None), dict(err=None), dict(eo=None),              # half of an optional pair
                   dict(n=-1), dict(n=1 << 31, offs=np.array([0, 100, 100, 1 << 31], np.int64)),
                   dict(n_refs=0), dict(n_refs=-3),
                   dict(offs=np.array([1, 100, 100, 300], np.int64)), dict(offs=np.array([0, 100, 100, 299], np.int64)),
                   dict(offs=np.array([0, 200, 100, 300], np.int64)), dict(offs=np.array([0, -5, 100, 300], np.int64)),
                   dict(radius=0.0), dict(radius=-1.0), dict(radius=float("inf")), dict(radius=float("nan")), dict(radius=1e-30), dict(radius=1e30),
                   dict(m=0), dict(m=-1), dict(m=9),
                   dict(xo=p(xyz)), dict(xo=p(xyz) + 12 * (n - 1)), dict(ro=p(rgb)), dict(eo=p(err)), dict(cons=p(err)), dict(xo=p(rgb)), dict(eo=p(xyz))]
        for kw in invalid:
            assert call(**kw) == LFD_ERR_INVALID, kw
            assert lib.lfd_last_error(twin._ctx).startswith(b"lfd_consensus_filter_host: "), kw
            assert b"key range" not in lib.lfd_last_error(twin._ctx)
        # the key range: a tiny radius on a wide cloud - more cells than a 63-bit key can number.  Decided before anything is sorted, in words of its own
        wide = (xyz * np.float32(5000.0)).astype(np.float32)
        assert call(xyz=p(wide), radius=1e-4) == LFD_ERR_INVALID and b"key range" in lib.lfd_last_error(twin._ctx)
        line = np.zeros((n, 3), np.float32)
        line[:, 0] = np.linspace(0.0, 2.0e6, n)                                              # one axis alone: more than 2^30 cells along it
        assert call(xyz=p(line), radius=1e-3) == LFD_ERR_INVALID and b"key range" in lib.lfd_last_error(twin._ctx)
        with pytest.raises(hb.ConsensusInputRefused, match="key range"):
            twin.consensus_filter(torch.from_numpy(wide), None, None, [100, 0, 200], 1e-4, 1)
        with pytest.raises(hb.HipBackendError, match="min_refs") as e:
            twin.consensus_filter(torch.from_numpy(xyz), None, None, [100, 0, 200], 0.1, 9)
        assert not isinstance(e.value, hb.ConsensusInputRefused)
        with pytest.raises(ValueError, match="ref_counts"):
            twin.consensus_filter(torch.from_numpy(xyz), None, None, [100, 0, 199], 0.1, 1)
        with pytest.raises(ValueError, match="rgb"):
            twin.consensus_filter(torch.from_numpy(xyz), torch.from_numpy(rgb[:10]), None, [100, 0, 200], 0.1, 1)
    finally:
        twin.close()
