"""The spatial point cap on the device (lfd_cap_spatial through HipDensifier) against the CPU twin and the NumPy reference of
tests/cap_ref.py, all given the SAME arrays: the index list equal element for element and the statistics equal bit for bit, on the clouds (a) - (g)
and on one cloud of 70 001 points with a budget of 4 099 (several workgroups, every pass of the sort, a level with many multi-point cells); a small
call behind a larger one on the same context; the refusals, the argument checks and the other context's entry points; and one end-to-end run of
the driver per cap mode on the device whose file is the host backend's byte for byte."""
import ctypes as C
import os
import struct

import numpy as np
import pytest
import torch

import cap_ref as cr
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LFD_ERR_INVALID, LFD_ERR_STATE = 1, 4
CLOUDS = cr.clouds()


@pytest.fixture(scope="module")
def dens():
    d = hb.HipDensifier(DEV)
    yield d
    d.close()


@pytest.fixture(scope="module")
def twin():
    d = hb.HostDensifier(16)
    yield d
    d.close()


@pytest.fixture(scope="module")
def reference():
    """name -> (keep, stats) of the reference, computed once"""
    return {name: cr.cap_ref(xyz, err, m) for name, xyz, err, m in CLOUDS}


def f64_bits(stats):
    return struct.pack("<4d", *[float(v) for v in stats])


def three(dens, twin, xyz, err, m, want=None):
    """device == twin == reference: the index list and the four statistics"""
    x = torch.from_numpy(xyz).to(DEV)
    e = None if err is None else torch.from_numpy(err).to(DEV)
    before = x.clone()
    got = dens.cap_spatial(x, e, m)
    assert got.is_cuda and got.dtype == torch.int64 and torch.equal(x, before)      # the input is read only
    host = twin.cap_spatial(torch.from_numpy(xyz), None if err is None else torch.from_numpy(err), m)
    keep, stats = want if want is not None else cr.cap_ref(xyz, err, m)
    assert got.cpu().numpy().tolist() == host.numpy().tolist() == keep.tolist()
    assert f64_bits(dens.cap_stats) == f64_bits(twin.cap_stats) == f64_bits(stats)
    return got.cpu().numpy(), dens.cap_stats


@pytest.mark.parametrize("case", CLOUDS, ids=[c[0] for c in CLOUDS])
def test_device_equals_twin_equals_reference(dens, twin, reference, case):
    name, xyz, err, m = case
    keep, stats = three(dens, twin, xyz, err, m, reference[name])
    print(name, "kept", keep.size, "stats", stats)


def test_several_workgroups_every_sort_pass_and_multi_point_cells(dens, twin):
    rng = np.random.default_rng(70001)
    n, m = 70001, 4099
    xyz = np.column_stack([rng.uniform(-3, 5, n), rng.uniform(0, 2, n), rng.normal(0, 0.01, n)]).astype(np.float32)
    xyz[1000:1400] = xyz[999]                                             # a run of duplicates that spans waves
    err = (rng.integers(0, 16, n) / 16.0).astype(np.float32)              # few values: ties in every cell
    keep, stats = three(dens, twin, xyz, err, m)
    assert keep.size == m and stats[1] >= m > stats[2] and n / stats[1] > 3      # many cells hold several points
    keys = cr.keys_ref(xyz)[0]
    assert int(keys.max()) >> 56 != 0                                     # the last of the eight sort passes has work to do
    three(dens, twin, xyz, None, m)
    print("70 001 points:", stats)


def test_a_small_call_after_a_larger_one_and_a_cap_that_does_not_act(dens, twin, reference):
    name, xyz, err, m = next(c for c in CLOUDS if c[0] == "g-m1000")
    three(dens, twin, xyz, err, m, reference[name])
    for small in ("a-m2", "b-n65-m32", "c-identical"):
        name, xyz, err, m = next(c for c in CLOUDS if c[0] == small)
        three(dens, twin, xyz, err, m, reference[name])
    xyz = np.random.default_rng(5).uniform(0, 1, (300, 3)).astype(np.float32)
    for m in (300, 5000):
        keep, _ = three(dens, twin, xyz, None, m)
        assert keep.tolist() == list(range(300))


def test_refusals_argument_checks_and_the_other_context_s_entry_points(dens, twin):
    keep = dens.cap_spatial(torch.zeros((0, 3), dtype=torch.float32, device=DEV), None, 3)
    assert keep.shape == (0,) and dens.cap_stats == (0, 0, 0, 0.0)
    xyz = np.random.default_rng(0).uniform(-1, 1, (300, 3)).astype(np.float32)
    for value in (np.nan, np.inf, -np.inf):
        bad = xyz.copy()
        bad[257, 1] = value
        with pytest.raises(hb.CapInputRefused, match="lfd_cap_spatial: non-finite coordinate in the input"):
            dens.cap_spatial(torch.from_numpy(bad).to(DEV), None, 100)
    x = torch.from_numpy(xyz).to(DEV)
    e = torch.zeros(300, dtype=torch.float32, device=DEV)
    out = torch.zeros(300, dtype=torch.int64, device=DEV)
    n_keep = C.c_int64(0)
    lib, ctx = dens._lib, dens._ctx
    for args, words in (((None, None, 5, 1, out.data_ptr(), C.byref(n_keep), None), b"null xyz / keep_out"),
                        ((x.data_ptr(), None, 300, 100, None, C.byref(n_keep), None), b"null xyz / keep_out"),
                        ((x.data_ptr(), None, 300, 100, out.data_ptr(), None, None), b"null n_keep_host"),
                        ((x.data_ptr(), None, 300, 0, out.data_ptr(), C.byref(n_keep), None), b"budget must be >= 1"),
                        ((x.data_ptr(), None, -1, 100, out.data_ptr(), C.byref(n_keep), None), b"n must be in [0, 2^31 - 1]"),
                        ((x.data_ptr(), None, 1 << 31, 100, out.data_ptr(), C.byref(n_keep), None), b"n must be in [0, 2^31 - 1]"),
                        ((x.data_ptr(), None, 300, 100, x.data_ptr() + 8, C.byref(n_keep), None), b"in and out arrays overlap"),
                        ((x.data_ptr(), e.data_ptr(), 300, 100, e.data_ptr(), C.byref(n_keep), None), b"in and out arrays overlap")):
        assert lib.lfd_cap_spatial(ctx, *args) == LFD_ERR_INVALID, words
        assert lib.lfd_last_error(ctx) == b"lfd_cap_spatial: " + words
    three(dens, twin, xyz, None, 100)                                     # the context still works behind the refusals
    assert lib.lfd_cap_spatial_host(ctx, None, None, 0, 1, None, C.byref(n_keep), None) == LFD_ERR_STATE
    assert twin._lib.lfd_cap_spatial(twin._ctx, None, None, 0, 1, None, C.byref(n_keep), None) == LFD_ERR_STATE


@pytest.mark.parametrize("mode", ["sampled", "dense"])
@pytest.mark.parametrize("cap_mode", ["random", "spatial"])
def test_the_driver_on_the_device_writes_the_host_backend_s_file(tmp_path, cap_mode, mode):
    """dense_init with max_points under either cap mode, device backend against host backend: the same file.  The scene keeps the comparison
    about this stage, as tests/test_gpu_gaussians.py's does: the same matcher fields in both runs, tie-free certainties and no noise."""
    import cycle_scene
    from lichtfeld_densification_plugin_amd import densify
    scene = cycle_scene.make_scene(str(tmp_path / "scene"), n_cams=4)

    def run(backend, name):
        args = densify.build_argparser().parse_args(["--scene_root", scene["root"], "--images_subdir", "images_4", "--num_refs", "0.75", "--nns_per_ref", "3",
                                                     "--matches_per_ref", "2500", "--seed", "3", "--pack_workers", "1", "--backend", backend,
                                                     "--triangulation_mode", mode, "--max_points", "1500", "--cap_mode", cap_mode,
                                                     "--out_name", name, "--estimate_normals"])
        matcher = cycle_scene.matcher_for(scene, noise_px=0.0, outlier_frac=0.0, cert_mode="tiefree")
        kw = {"device": DEV} if backend == "device" else {}
        assert densify.dense_init(args, matcher=matcher, **kw) == 0
        return open(os.path.join(scene["root"], "sparse", "0", name), "rb").read()
    on_device, on_host = run("device", f"cap_device_{cap_mode}_{mode}.ply"), run("host", f"cap_host_{cap_mode}_{mode}.ply")
    head_d, body_d = on_device.split(b"end_header\n", 1)
    head_h, body_h = on_host.split(b"end_header\n", 1)
    rows_d, rows_h = np.frombuffer(body_d, np.uint8).reshape(-1, 27), np.frombuffer(body_h, np.uint8).reshape(-1, 27)
    print(cap_mode, mode, "vertices:", rows_d.shape[0], rows_h.shape[0], "rows that differ:",
          int((rows_d != rows_h).any(axis=1).sum()) if rows_d.shape == rows_h.shape else "-")
    assert b"element vertex 1500\n" in head_d and head_d == head_h
    assert on_device == on_host
