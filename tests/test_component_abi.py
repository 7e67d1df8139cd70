"""CPU tier of the component filter's entry points (lfd_component_filter / lfd_component_filter_host): the library exports them, the header
declares them with the argument list of DESIGN.md 4.29 and states the contract, the binding types them, the ABI version and the pinned
structures are unchanged (new symbols change no layout), every refusal of the contract answers LFD_ERR_INVALID with its message - the key-range
one in the consensus filter's words, which the binding turns into ConsensusInputRefused - and a context of the wrong kind is refused (a host
context given to the device call: LFD_ERR_STATE; the reverse is tests/test_gpu_component.py's)."""
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
        "int32_t n_refs", "float radius", "int32_t min_points", "float* xyz_out", "float* rgb_out", "float* err_out",
        "int64_t* ref_offsets_out_host", "uint32_t* size", "uint32_t* label", "int64_t* summary_host", "int64_t* n_out_host"]
NAMES = ["lfd_component_filter", "lfd_component_filter_host"]
NULL_CALL = (None, None, None, 0, None, 1, 1.0, 2, None, None, None, None, None, None, None, None)


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
    # the consensus filter's declaration with min_points in place of min_refs and the three optional outputs in place of its one
    cons = re.search(r"int\s+" + name.replace("component", "consensus") + r"\s*\(([^)]*)\)\s*;", header)
    want = [" ".join(a.split()) for a in cons.group(1).split(",")]
    assert want[:8] + want[9:13] + want[14:] == ARGS[:8] + ARGS[9:13] + ARGS[16:]
    # additive: the new symbols change no layout, and the ABI version is still the 9 the existing ABI tests assert
    assert lib.lfd_abi_version() == 9 == hb.LFD_ABI_VERSION
    hb.check_struct_layout(lib)
    assert C.sizeof(hb.lfd_params) == 32 and C.sizeof(hb.lfd_points) == 48 and C.sizeof(hb.lfd_batch) == 120


def test_the_header_states_the_contract():
    header = " ".join(open(os.path.join(ROOT, "include", "lfd_densify.h")).read().split())
    text = header[header.index("Connected-component filter on the final cloud (DESIGN 4.29"):header.index("int lfd_component_filter(")]
    for words in ("agree(i, j)", "transitive closure", "non-finite coordinate links to nothing", "smallest INPUT index", "size(i) >= min_points",
                  "min_points in 2 .. 2^31 - 1", "i64 [66]", "[34 + b]", "cannot hang", "bit for bit"):
        assert words in text, words
    shared = open(os.path.join(ROOT, "lichtfeld-densification-plugin_amd", "csrc", "lfd_component.hpp")).read()
    assert "TERMINATION" in shared and "lfd_consensus_agree(" in shared and "d2 <=" not in shared          # the link test is called, not copied


@pytest.mark.parametrize("name", NAMES)
def test_binding_sets_argtypes(lib, name):
    f = getattr(lib, name)
    assert f.restype is C.c_int
    assert f.argtypes is not None and len(f.argtypes) == len(ARGS)
    assert [i for i, t in enumerate(f.argtypes) if t is C.c_float] == [7]
    assert [i for i, t in enumerate(f.argtypes) if t is C.c_int64] == [4] and [i for i, t in enumerate(f.argtypes) if t is C.c_int32] == [6, 8]
    for cls in (hb.HipDensifier, hb.HostDensifier):
        sig = inspect.signature(cls.component_filter).parameters
        assert list(sig)[1:] == ["xyz", "rgb", "err", "ref_counts", "radius", "min_points", "with_sizes", "with_labels"]
        assert sig["with_sizes"].default is False and sig["with_labels"].default is False
    assert hb.COMPONENT_SUMMARY_WORDS == 66


@pytest.mark.parametrize("name", NAMES)
def test_null_context_is_invalid(lib, name):
    assert getattr(lib, name)(None, *NULL_CALL) == LFD_ERR_INVALID
    assert lib.lfd_last_error(None)


def test_host_context_is_refused_by_the_device_call(lib):
    ctx = C.c_void_p()
    assert lib.lfd_create_host(1, C.byref(ctx)) == 0 and ctx.value
    try:
        assert lib.lfd_component_filter(ctx, *NULL_CALL) == LFD_ERR_STATE
        assert b"host" in lib.lfd_last_error(ctx)
        assert lib.lfd_component_filter_host(ctx, *NULL_CALL) == LFD_ERR_INVALID            # its own entry point looks at the arguments
        assert b"lfd_component_filter_host" in lib.lfd_last_error(ctx)
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
        size, label = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        summ = np.full(66, -1, np.int64)
        offs = np.array([0, 100, 100, 300], np.int64)
        offs_out = np.full(4, -1, np.int64)
        n_out = C.c_int64(-1)
        i64p = C.POINTER(C.c_int64)
        p = lambda a: a.ctypes.data                                         # noqa: E731
        good = dict(xyz=p(xyz), rgb=p(rgb), err=p(err), n=n, offs=offs, n_refs=3, radius=0.2, m=3, xo=p(xo), ro=p(ro), eo=p(eo), offs_out=offs_out,
                    size=p(size), label=p(label), summ=summ, n_out=C.byref(n_out))

        def call(**kw):
            a = {**good, **kw}
            o = a["offs"].ctypes.data_as(i64p) if a["offs"] is not None else None
            oo = a["offs_out"].ctypes.data_as(i64p) if a["offs_out"] is not None else None
            sm = a["summ"].ctypes.data_as(i64p) if a["summ"] is not None else None
            return lib.lfd_component_filter_host(twin._ctx, a["xyz"], a["rgb"], a["err"], a["n"], o, a["n_refs"], a["radius"], a["m"], a["xo"],
                                                 a["ro"], a["eo"], oo, a["size"], a["label"], sm, a["n_out"])

        def message():
            return lib.lfd_last_error(twin._ctx).decode()

        before = xyz.copy()
        assert call() == 0 and 0 < n_out.value < n and offs_out[0] == 0 and offs_out[3] == n_out.value and offs_out[1] == offs_out[2]
        assert int((size >= 3).sum()) == n_out.value and np.array_equal(xyz, before)        # the input is read only
        assert summ[0] > 1 and summ[34:].sum() == n and summ[2:34].sum() == summ[0] and summ[1] == size.max()
        assert call(rgb=None, ro=None, err=None, eo=None, size=None, label=None, summ=None) == 0      # the optional arrays
        assert call(m=2 ** 31 - 1) == 0 and n_out.value == 0 and not offs_out.any()
        assert call(n=0, offs=np.zeros(4, np.int64), xyz=None, xo=None, rgb=None, ro=None, err=None, eo=None, size=None, label=None) == 0
        assert n_out.value == 0 and not summ.any()
        same = "lfd_component_filter_host: "
        invalid = [(dict(offs=None), "null ref_offsets_host"), (dict(offs_out=None), "null ref_offsets_host"), (dict(n_out=None), "null ref_offsets_host"),
                   (dict(xyz=None), "null xyz / xyz_out"), (dict(xo=None), "null xyz / xyz_out"),
                   (dict(rgb=None), "both be given or both be null"), (dict(ro=None), "both be given"), (dict(err=None), "both be given"),
                   (dict(eo=None), "both be given"),
                   (dict(n=-1), "n must be in"), (dict(n=1 << 31, offs=np.array([0, 100, 100, 1 << 31], np.int64)), "n must be in"),
                   (dict(n_refs=0), "n_refs must be >= 1"), (dict(n_refs=-3), "n_refs must be >= 1"),
                   (dict(offs=np.array([1, 100, 100, 300], np.int64)), "must start at 0 and end at n"),
                   (dict(offs=np.array([0, 100, 100, 299], np.int64)), "must start at 0 and end at n"),
                   (dict(offs=np.array([0, 200, 100, 300], np.int64)), "must not decrease"),
                   (dict(radius=0.0), "radius must be finite and > 0"), (dict(radius=-1.0), "radius must be finite and > 0"),
                   (dict(radius=float("inf")), "radius must be finite and > 0"), (dict(radius=float("nan")), "radius must be finite and > 0"),
                   (dict(radius=1e-30), "normal f32"), (dict(radius=1e30), "normal f32"),
                   (dict(m=1), "min_points must be in [2, 2^31 - 1]"), (dict(m=0), "min_points must be in"), (dict(m=-7), "min_points must be in"),
                   (dict(xo=p(xyz)), "overlap"), (dict(xo=p(xyz) + 12 * (n - 1)), "overlap"), (dict(ro=p(rgb)), "overlap"), (dict(eo=p(err)), "overlap"),
                   (dict(xo=p(rgb)), "overlap"), (dict(eo=p(xyz)), "overlap"),
                   (dict(size=p(xyz)), "overlap"), (dict(size=p(err)), "overlap"), (dict(label=p(rgb)), "overlap"),
                   (dict(label=p(xyz) + 12 * n - 4), "overlap"), (dict(size=p(err) + 4 * (n - 1)), "overlap")]
        for kw, text in invalid:
            assert call(**kw) == LFD_ERR_INVALID, kw
            assert message().startswith(same) and text in message(), (kw, message())
            assert "key range" not in message()
        # the key range: a tiny radius on a wide cloud - more cells than a 63-bit key can number.  The consensus filter's refusal, in its words
        wide = (xyz * np.float32(5000.0)).astype(np.float32)
        assert call(xyz=p(wide), radius=1e-4) == LFD_ERR_INVALID and "key range" in message()
        line = np.zeros((n, 3), np.float32)
        line[:, 0] = np.linspace(0.0, 2.0e6, n)                                              # one axis alone: more than 2^30 cells along it
        assert call(xyz=p(line), radius=1e-3) == LFD_ERR_INVALID and "key range" in message() and "2^30 cells" in message()
        with pytest.raises(hb.ConsensusInputRefused, match="key range"):
            twin.component_filter(torch.from_numpy(wide), None, None, [100, 0, 200], 1e-4, 2)
        with pytest.raises(hb.HipBackendError, match="min_points") as e:
            twin.component_filter(torch.from_numpy(xyz), None, None, [100, 0, 200], 0.1, 1)
        assert not isinstance(e.value, hb.ConsensusInputRefused)
        with pytest.raises(ValueError, match="ref_counts"):
            twin.component_filter(torch.from_numpy(xyz), None, None, [100, 0, 199], 0.1, 2)
        with pytest.raises(ValueError, match="rgb"):
            twin.component_filter(torch.from_numpy(xyz), torch.from_numpy(rgb[:10]), None, [100, 0, 200], 0.1, 2)
    finally:
        twin.close()
