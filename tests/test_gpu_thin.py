"""The footprint-adaptive thinning on the device (lfd_thin_footprint through HipDensifier) against the CPU twin and the brute-force
reference of tests/thin_ref.py, all given the SAME arrays: the index list, the kept counts per reference and the per-level statistics equal element
for element, at the sizes where the shared driver's plan (lfd_api.hip cloud_plan) and its one-workgroup scan change regime, with one, three and 300
references, empty ones among them, a workgroup that spans three references and a cell heavier than a wave; a small call behind a large one on the
same context; the refusals; and one end-to-end run of the driver on the device whose file is the host backend's byte for byte."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import thin_ref as tr
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LFD_ERR_INVALID, LFD_ERR_STATE = 1, 4


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


def three(dens, twin, xyz, err, counts, rows, thin_cells, reference=True):
    """device == twin (== reference): the index list, the kept counts and the statistics"""
    x = torch.from_numpy(xyz).to(DEV)
    e = None if err is None else torch.from_numpy(err).to(DEV)
    before = x.clone()
    got, got_counts = dens.thin_footprint(x, e, counts, rows, thin_cells)
    assert got.is_cuda and got.dtype == torch.int64 and torch.equal(x, before)      # the index stays on the device, the input is read only
    host, host_counts = twin.thin_footprint(torch.from_numpy(xyz), None if err is None else torch.from_numpy(err), counts, rows, thin_cells)
    keep = got.cpu().numpy()
    assert np.array_equal(keep, host.numpy()) and got_counts.tolist() == host_counts.tolist()
    for a, b in zip(dens.thin_stats[:2], twin.thin_stats[:2]):
        assert a.tolist() == b.tolist()
    assert dens.thin_stats[2] == twin.thin_stats[2]
    if reference:
        want, want_counts, want_stats = tr.thin_ref(xyz, err, counts, rows, thin_cells)
        assert np.array_equal(keep, want) and got_counts.tolist() == want_counts.tolist()
        assert dens.thin_stats[0].tolist() == want_stats[0].tolist() and dens.thin_stats[1].tolist() == want_stats[1].tolist()
        assert dens.thin_stats[2] == want_stats[2]
    return keep, got_counts, dens.thin_stats


def plan(n):
    """cloud_plan's integers: radix workgroups, workgroups with a thread per point"""
    G = min(1024, (n + 4095) // 4096)
    chunk = (((n + G - 1) // G) + 511) // 512 * 512
    return (n + chunk - 1) // chunk, (n + 255) // 256


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4097])
def test_sizes_around_one_workgroup_and_two_radix_workgroups(dens, twin, n):
    G, n_wg = plan(n)
    assert (G, n_wg) == {1: (1, 1), 255: (1, 1), 256: (1, 1), 257: (1, 2), 4097: (2, 17)}[n]
    counts = [n // 3, n - n // 3 - n // 4, n // 4]
    xyz, err, rows = tr.random_case(n, counts, n)
    keep, _, stats = three(dens, twin, xyz, err, counts, rows, 2.0)
    three(dens, twin, xyz, None, counts, rows, 2.0)
    print(n, "kept", keep.size, "levels", np.flatnonzero(stats[0]).tolist())


def test_more_than_1024_workgroups_in_the_scan(dens, twin):
    n = 266241
    G, n_wg = plan(n)
    assert n_wg == 1041 > 1024 and (n_wg + 1023) // 1024 == 2 and G == 66 and n_wg <= 4096      # two counts per thread of the one-workgroup scan
    counts = [90000, 0, 100000, 76241]
    xyz, err, rows = tr.random_case(n, counts, 7, dupes=1000)             # 1 000 points in one cell: heavier than a wave, across workgroups
    keep, kept, stats = three(dens, twin, xyz, err, counts, rows, 2.0)
    assert np.count_nonzero(keep < 1000) == 1 and kept[1] == 0 and 0 < keep.size < n
    assert int(stats[1].sum()) == keep.size and np.count_nonzero(stats[0]) >= 2
    print("266 241 points: kept", keep.size, "points", stats[0].tolist(), "cells", stats[1].tolist())


def test_the_grid_cap_device_against_twin(dens, twin):
    n = 1052673
    G, n_wg = plan(n)
    assert n_wg == 4113 > 4096 and G == 258                             # grid = min(n_wg, 4096): the striding kernels run a second trip
    counts = [400000, 252673, 400000]
    xyz, err, rows = tr.random_case(n, counts, 8)
    keep, _, stats = three(dens, twin, xyz, err, counts, rows, 1.0, reference=False)
    assert 0 < keep.size < n
    print("1 052 673 points: kept", keep.size)


@pytest.mark.parametrize("n_refs", [1, 3, 300])
def test_one_three_and_300_references_with_empty_ones(dens, twin, n_refs):
    rng = np.random.default_rng(n_refs)
    counts = rng.integers(0, 60, n_refs)
    counts[rng.integers(0, n_refs, n_refs // 4)] = 0                      # empty references, wherever they fall
    counts[0] = max(int(counts[0]), 7)
    if n_refs >= 3:
        counts[1] = 0                                                     # one in the middle ...
    if n_refs > 3:
        counts[-2:] = 0                                                   # ... and two at the end
    n = int(counts.sum())
    xyz, err, rows = tr.random_case(n, counts, 100 + n_refs)
    keep, kept, _ = three(dens, twin, xyz, err, counts, rows, 2.0)
    assert (kept[counts == 0] == 0).all()
    print(n_refs, "references,", n, "points, kept", keep.size)


def test_a_workgroup_that_spans_three_references(dens, twin):
    counts = [100, 60, 400]                                               # points 0 .. 255: three references; 256 .. 511: one; the tail: one
    xyz, err, rows = tr.random_case(560, counts, 9)
    rows[:, 4] = [0.002, 0.02, 0.2]                                       # three footprints an order of magnitude apart: a wrong reference shows
    keep, kept, stats = three(dens, twin, xyz, err, counts, rows, 2.0)
    assert np.count_nonzero(stats[0]) >= 3 and (kept > 0).all()


def test_a_small_call_after_a_large_one(dens, twin):
    counts = [30000, 40001]
    xyz, err, rows = tr.random_case(70001, counts, 10)
    three(dens, twin, xyz, err, counts, rows, 2.0)
    xyz, err, rows = tr.random_case(65, [65], 11)
    three(dens, twin, xyz, err, [65], rows, 2.0)
    same = np.repeat(xyz[:1], 50, axis=0)
    keep, _, stats = three(dens, twin, same, err[:50], [50], rows, 2.0)
    assert keep.tolist() == [int(np.argmin(err[:50]))] and stats[2] == 0.0


def test_refusals_argument_checks_and_the_other_context_s_entry_points(dens, twin):
    rows = np.array([[0.0, 0.0, 1.0, 10.0, 0.01]])
    keep, kept = dens.thin_footprint(torch.zeros((0, 3), dtype=torch.float32, device=DEV), None, [0], rows, 2.0)
    assert keep.shape == (0,) and kept.tolist() == [0] and int(dens.thin_stats[0].sum()) == 0
    xyz = np.random.default_rng(0).uniform(-1, 1, (300, 3)).astype(np.float32)
    for value in (np.nan, np.inf, -np.inf):
        bad = xyz.copy()
        bad[257, 1] = value
        with pytest.raises(hb.ThinInputRefused, match="lfd_thin_footprint: non-finite coordinate in the input"):
            dens.thin_footprint(torch.from_numpy(bad).to(DEV), None, [300], rows, 2.0)
    x = torch.from_numpy(xyz).to(DEV)
    out = torch.zeros(300, dtype=torch.int64, device=DEV)
    n_keep = C.c_int64(0)
    i64p, f64p = C.POINTER(C.c_int64), C.POINTER(C.c_double)
    offs, offs_out = np.array([0, 300], np.int64), np.zeros(2, np.int64)
    lib, ctx = dens._lib, dens._ctx

    def call(fn, c, xp=x.data_ptr(), n=300, o=offs, r=rows, tc=2.0, kp=out.data_ptr(), nk=C.byref(n_keep), oo=offs_out):
        return fn(c, xp, None, n, o.ctypes.data_as(i64p) if o is not None else None, 1, r.ctypes.data_as(f64p) if r is not None else None,
                  C.c_double(tc), kp, nk, oo.ctypes.data_as(i64p) if oo is not None else None, None)
    for kw, words in ((dict(kp=None), b"null xyz / keep_out"), (dict(tc=0.0), b"thin_cells must be finite and > 0"),
                      (dict(tc=float("inf")), b"thin_cells must be finite and > 0"), (dict(n=-1), b"n must be in [0, 2^31 - 1]"),
                      (dict(o=np.array([0, 299], np.int64)), b"ref_offsets_host must start at 0 and end at n"),
                      (dict(r=np.array([[0.0, 0.0, 1.0, 10.0, 0.0]])), b"every tan_cell must be finite and > 0"),
                      (dict(kp=x.data_ptr() + 8), b"in and out arrays overlap")):
        assert call(lib.lfd_thin_footprint, ctx, **kw) == LFD_ERR_INVALID, words
        assert lib.lfd_last_error(ctx) == b"lfd_thin_footprint: " + words
    three(dens, twin, xyz, None, [300], rows, 2.0)                        # the context still works behind the refusals
    assert call(lib.lfd_thin_footprint_host, ctx) == LFD_ERR_STATE
    assert call(twin._lib.lfd_thin_footprint, twin._ctx) == LFD_ERR_STATE


@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_the_driver_on_the_device_writes_the_host_backend_s_file(tmp_path, mode, monkeypatch):
    """dense_init with footprint_thin_cells, device backend against host backend: the same file, fewer points than without the knob, and the
    index of the device run never leaves the GPU.  The scene keeps the comparison about this stage, as tests/test_gpu_cap.py's does."""
    import cycle_scene
    from lichtfeld_densification_plugin_amd import densify
    scene = cycle_scene.make_scene(str(tmp_path / "scene"), n_cams=4)
    seen = []
    real = hb.HipDensifier.thin_footprint

    def spy(self, *a, **kw):
        keep, counts = real(self, *a, **kw)
        seen.append(keep.is_cuda)
        return keep, counts
    monkeypatch.setattr(hb.HipDensifier, "thin_footprint", spy)

    def run(backend, name, cells):
        args = densify.build_argparser().parse_args(["--scene_root", scene["root"], "--images_subdir", "images_4", "--num_refs", "0.75", "--nns_per_ref", "3",
                                                     "--matches_per_ref", "2500", "--seed", "3", "--pack_workers", "1", "--backend", backend,
                                                     "--triangulation_mode", mode, "--footprint_thin_cells", cells, "--out_name", name,
                                                     "--estimate_normals"])
        matcher = cycle_scene.matcher_for(scene, noise_px=0.0, outlier_frac=0.0, cert_mode="tiefree")
        kw = {"device": DEV} if backend == "device" else {}
        assert densify.dense_init(args, matcher=matcher, **kw) == 0
        return open(os.path.join(scene["root"], "sparse", "0", name), "rb").read()
    on_device, on_host = run("device", f"thin_device_{mode}.ply", "2"), run("host", f"thin_host_{mode}.ply", "2")
    off = run("host", f"thin_off_{mode}.ply", "0")
    count = lambda blob: int(blob.split(b"element vertex ", 1)[1].split(b"\n", 1)[0])      # noqa: E731
    print(mode, "vertices:", count(on_device), count(on_host), "knob off:", count(off))
    assert seen == [True]
    assert 0 < count(on_device) < count(off)
    assert on_device == on_host
