"""CPU tier of the pose refinement's entry points (lfd_pose_accumulate and its _host twin): the library exports them, the
header declares them with the documented argument lists, the binding types them, the ABI version and the pinned structures are unchanged,
every refusal of the contract answers with its status and a message that names the call, a table that overlaps the batch's planes is
refused, a refused call adds nothing, and a context of the wrong kind is refused (a null context: LFD_ERR_INVALID; a host context given to
the device call: LFD_ERR_STATE - the reverse is tests/test_gpu_pose.py's).  And the shared routines of csrc/lfd_pose.hpp under
AddressSanitizer and UndefinedBehaviorSanitizer: tests/abi/pose_sanitize.cpp, a host program with its own main, compiled with
-fsanitize=address,undefined and run as a process of its own."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

import pose_scene as ps
from helpers import ROOT
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

LFD_ERR_INVALID, LFD_ERR_STATE = 1, 4
ARGS = ["lfd_context* ctx", "const lfd_batch* batch", "float pose_certainty", "float pose_inlier_px", "int64_t* table"]
NAMES = ("lfd_pose_accumulate", "lfd_pose_accumulate_host")
NULL_CALL = (None, 0.5, 8.0, None)
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
    assert f.argtypes is not None and len(f.argtypes) == len(ARGS) and f.argtypes[2] is C.c_float and f.argtypes[3] is C.c_float
    for cls in (hb.HipDensifier, hb.HostDensifier):
        assert callable(getattr(cls, "pose_accumulate", None))
    assert hb.POSE_QUANTITIES == 32 and tuple(hb.pose_table(2, 3, torch.device("cpu")).shape) == (6, 32)


@pytest.mark.parametrize("name", NAMES)
def test_null_context_is_invalid(lib, name):
    assert getattr(lib, name)(None, *NULL_CALL) == LFD_ERR_INVALID
    assert lib.lfd_last_error(None)


def test_host_context_is_refused_by_the_device_call(lib):
    ctx = C.c_void_p()
    assert lib.lfd_create_host(1, C.byref(ctx)) == 0 and ctx.value
    try:
        assert lib.lfd_pose_accumulate(ctx, *NULL_CALL) == LFD_ERR_STATE
        assert b"host" in lib.lfd_last_error(ctx)
        assert lib.lfd_pose_accumulate_host(ctx, *NULL_CALL) == LFD_ERR_INVALID              # its own entry point looks at the arguments
        assert b"lfd_pose_accumulate_host: null table" in lib.lfd_last_error(ctx)
    finally:
        lib.lfd_destroy(ctx)


def test_every_refusal_of_the_contract(lib):
    twin = hb.HostDensifier(1)
    twin.upload_cameras(ps.cameras(ps.TABLE_WRONG))
    try:
        H, W = 12, 16
        ri = ps.make(1, ps.neighbours(1, 3), H, W, match=MATCH, masks=True, noise_px=0.7).inputs
        batch = hb.PreparedBatch([ri], MATCH, MATCH)
        table = hb.pose_table(1, 3, torch.device("cpu"))
        good = dict(batch=C.byref(batch.c), cert=0.5, px=8.0, table=table.data_ptr())

        def call(**kw):
            a = {**good, **kw}
            return lib.lfd_pose_accumulate_host(twin._ctx, a["batch"], a["cert"], a["px"], a["table"])

        assert call() == 0
        first = table.clone()
        assert int(first[:, 0].sum()) > 100 and int(first[:, 3].min()) > 0
        assert call() == 0 and torch.equal(table, 2 * first)                               # added to
        tb = 3 * 32 * 8
        planes = [ri.cert[0], ri.cert[2], ri.warp[1], ri.image, ri.mask_a, ri.mask_b[0], ri.mask_b[2]]
        messages = {"table": b"null table", "cert": b"pose_certainty must be finite and > 0", "px": b"pose_inlier_px must be in (0, 64]"}
        invalid = [dict(batch=None), dict(table=None), dict(cert=0.0), dict(cert=-0.5), dict(cert=float("nan")), dict(cert=float("inf")),
                   dict(px=0.0), dict(px=-1.0), dict(px=64.5), dict(px=float("nan")), dict(px=float("inf"))]
        invalid += [dict(table=p.data_ptr()) for p in planes]
        invalid += [dict(table=p.data_ptr() - tb + 1) for p in planes]                   # the table's last byte reaches into the plane
        invalid += [dict(table=p.data_ptr() + p.numel() * p.element_size() - 1) for p in planes]      # its first byte is the plane's last
        for kw in invalid:
            assert call(**kw) == LFD_ERR_INVALID, kw
            err = lib.lfd_last_error(twin._ctx)
            assert b"lfd_pose_accumulate_host" in err or kw.get("batch", 1) is None
            (key,) = kw
            if key in messages and (kw[key] is None or key != "table"):
                assert messages[key] in err
            elif key != "batch":
                assert b"must overlap nothing of the batch" in err
        assert torch.equal(table, 2 * first)                                               # a refused call adds nothing
        assert call(cert=1.0, px=64.0) == 0                                                # the limits themselves are accepted
        # more than 65535 references (the grid's second dimension)
        small = ps.make(1, [0], 2, 2, match=MATCH).inputs
        many = hb.PreparedBatch([small] * 65536, MATCH, MATCH)
        big = torch.zeros((65536, 32), dtype=torch.int64)
        assert lib.lfd_pose_accumulate_host(twin._ctx, C.byref(many.c), 0.5, 8.0, big.data_ptr()) == LFD_ERR_INVALID
        assert b"at most 65535 references" in lib.lfd_last_error(twin._ctx) and int(big.abs().sum()) == 0
        # more than 2^24 cells per reference (the sums' overflow bound): planes that are never touched
        import dataclasses
        wide = dataclasses.replace(small, cert=[torch.empty((4097, 4096), dtype=torch.float32)], warp=[torch.empty((4097, 4096, 2), dtype=torch.float32)])
        one = torch.zeros((1, 32), dtype=torch.int64)
        assert lib.lfd_pose_accumulate_host(twin._ctx, C.byref(hb.PreparedBatch([wide], MATCH, MATCH).c), 0.5, 8.0, one.data_ptr()) == LFD_ERR_INVALID
        assert b"at most 2^24 grid cells" in lib.lfd_last_error(twin._ctx) and int(one.abs().sum()) == 0
        # the binding's own refusals name what is wrong
        with pytest.raises(hb.HipBackendError, match="pose_certainty"):
            twin.pose_accumulate(batch, 0.0, 8.0)
        with pytest.raises(hb.HipBackendError, match="pose_inlier_px"):
            twin.pose_accumulate(batch, 0.5, 65.0)
        with pytest.raises(ValueError, match="table must be a contiguous int64"):
            twin.pose_accumulate(batch, 0.5, 8.0, table=torch.zeros((3, 31), dtype=torch.int64))
    finally:
        twin.close()


def test_the_pose_routines_run_clean_under_asan_and_ubsan(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = os.path.join(str(tmp_path), "pose_sanitize")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "lichtfeld-densification-plugin_amd", "csrc"), os.path.join(ROOT, "tests", "abi", "pose_sanitize.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    print(ran.stdout)
    assert ran.stdout.strip().endswith("ok (0 mismatches)") and "runtime error" not in ran.stderr and "AddressSanitizer" not in ran.stderr
