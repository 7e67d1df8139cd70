"""The cross-reference consensus filter on the device (lfd_consensus_filter through HipDensifier.consensus_filter) against the CPU twin - both
sides are given the SAME cloud - at the smallest sizes that take every path: one lane, one workgroup and a ragged second one, several radix
passes and many workgroups with reference and cell boundaries inside them, thousands of points in one cell, empty references, a single
reference, non-finite points, no points.  Every output - counts, kept points, colours, errors, per-reference counts - equals the twin's bit for
bit (the test is f32 with every rounding written out; what is counted does not depend on how neighbours are found), so does a second launch, a
launch after a larger one, the cloud the dense kernel made and, through the driver, the written file."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import support_scene as sc
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LFD_ERR_STATE = 4


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


def bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def cloud(kind, n, n_refs, seed, empty=()):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        xyz = rng.uniform(-1.0, 1.0, (n, 3))
    elif kind == "cell":
        xyz = rng.uniform(0.0, 0.01, (n, 3))
    else:
        centres = rng.uniform(-3.0, 3.0, (40, 3))
        xyz = centres[rng.integers(0, 40, n)] + rng.normal(0.0, 0.03, (n, 3))
    live = np.asarray([g for g in range(n_refs) if g not in empty])
    counts = np.bincount(live[rng.integers(0, len(live), n)], minlength=n_refs).astype(np.int64) if n else np.zeros(n_refs, np.int64)
    rgb = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
    err = rng.uniform(0.0, 2.0, (n,)).astype(np.float32)
    return xyz.astype(np.float32), rgb, err, counts


def both(dens, twin, xyz, rgb, err, counts, radius, m, with_consensus=True, travel=True):
    """one call on each side over the same cloud; returns the device's outputs after comparing every one of them with the twin's"""
    t = lambda a, dev: torch.from_numpy(np.ascontiguousarray(a)).to(dev) if a is not None else None      # noqa: E731
    r, e = (rgb, err) if travel else (None, None)
    d = dens.consensus_filter(t(xyz, DEV), t(r, DEV), t(e, DEV), counts, radius, m, with_consensus)
    h = twin.consensus_filter(t(xyz, "cpu"), t(r, "cpu"), t(e, "cpu"), counts, radius, m, with_consensus)
    for i, name in enumerate(("xyz", "rgb", "err")):
        assert (d[i] is None) == (h[i] is None), name
        if d[i] is not None:
            assert d[i].shape == h[i].shape and np.array_equal(bits(d[i]), bits(h[i])), name
    assert np.array_equal(d[3], h[3])
    assert (d[4] is None) == (h[4] is None) == (not with_consensus)
    if with_consensus:
        assert np.array_equal(bits(d[4]), bits(h[4]))
    return d


SIZES = [(1, 7, 0.5), (2, 7, 3.0), (257, 7, 0.3), (5000, 7, 0.08)]


@pytest.mark.parametrize("n,n_refs,radius", SIZES)
@pytest.mark.parametrize("m", [1, 3, 8])
def test_small_clouds_equal_the_twin(dens, twin, n, n_refs, radius, m):
    xyz, rgb, err, counts = cloud("uniform", n, n_refs, seed=n)
    d = both(dens, twin, xyz, rgb, err, counts, radius, m, True)
    k = both(dens, twin, xyz, rgb, err, counts, radius, m, False, travel=False)
    assert np.array_equal(bits(d[0]), bits(k[0])) and np.array_equal(d[3], k[3])          # the same kept set with and without the counts
    c = d[4].cpu().numpy()
    assert int(d[0].shape[0]) == int((c >= m).sum())
    if n == 5000:
        assert 0 < int((c >= 1).sum()) < n and c.max() >= 3


@pytest.mark.parametrize("m,with_consensus", [(1, True), (3, False), (8, True)])
def test_a_clustered_cloud_of_many_workgroups_and_radix_passes(dens, twin, m, with_consensus):
    xyz, rgb, err, counts = cloud("clustered", 100003, 40, seed=7)                            # ~6e8 cells: four radix passes, 391 workgroups
    d = both(dens, twin, xyz, rgb, err, counts, 0.01, m, with_consensus)
    assert 0 < int(d[0].shape[0]) < 100003 or m == 8


def test_thousands_of_points_of_five_references_in_one_cell(dens, twin):
    xyz, rgb, err, counts = cloud("cell", 3000, 5, seed=3)
    d = both(dens, twin, xyz, rgb, err, counts, 10.0, 3, True)
    assert (d[4].cpu().numpy() == 4).all() and int(d[0].shape[0]) == 3000
    both(dens, twin, xyz, rgb, err, counts, 0.0015, 2, True)                                  # ... and a radius at which only some agree
    both(dens, twin, xyz, rgb, err, counts, 10.0, 5, False)


def test_the_lattice_threshold(dens, twin):
    xyz = np.array([[0, 0, 0], [3, 4, 0]], np.float32)
    rgb, err = np.zeros((2, 3), np.float32), np.zeros(2, np.float32)
    for radius, c in ((5.0, 1), (float(np.nextafter(np.float32(5.0), np.float32(0.0))), 0)):
        d = both(dens, twin, xyz, rgb, err, [1, 1], radius, 1)
        assert d[4].cpu().tolist() == [c, c] and d[3].tolist() == [c, c]


def test_empty_references_a_single_reference_non_finite_points_and_no_points(dens, twin):
    xyz, rgb, err, counts = cloud("clustered", 2000, 9, seed=5, empty=(0, 1, 4, 8))
    assert counts[[0, 1, 4, 8]].tolist() == [0, 0, 0, 0]
    d = both(dens, twin, xyz, rgb, err, counts, 0.06, 2)
    assert 0 < int(d[0].shape[0]) < 2000 and not d[3][[0, 1, 4, 8]].any()
    d = both(dens, twin, xyz, rgb, err, [2000], 10.0, 1)
    assert int(d[0].shape[0]) == 0 and not d[4].any()
    bad = xyz.copy()
    rng = np.random.default_rng(6)
    at = rng.choice(2000, 90, replace=False)
    bad[at[:30], 0], bad[at[30:60], 2], bad[at[60:], 1] = np.nan, np.inf, -np.inf
    rgb[5, 0], err[9] = np.nan, np.inf                                                     # what travels along is copied, not looked at
    d = both(dens, twin, bad, rgb, err, counts, 0.06, 1)
    assert not d[4].cpu().numpy()[at].any() and int(d[0].shape[0]) > 0
    d = both(dens, twin, np.full((300, 3), np.nan, np.float32), rgb[:300], err[:300], [100, 200], 1.0, 1)
    assert int(d[0].shape[0]) == 0 and not d[4].any()
    d = both(dens, twin, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros((0,), np.float32), [0, 0, 0], 1.0, 1)
    assert d[0].shape == (0, 3) and d[3].tolist() == [0, 0, 0]


def test_two_launches_give_equal_bits_and_a_smaller_launch_reuses_the_workspace(dens, twin):
    big = cloud("clustered", 20000, 12, seed=9)
    small = cloud("uniform", 700, 5, seed=10)
    a = both(dens, twin, *big, 0.03, 2)
    s = both(dens, twin, *small, 0.2, 1)                                                   # after a larger one: the workspace holds stale keys behind it
    b = both(dens, twin, *big, 0.03, 2)
    for x, y in zip(a, b):
        assert np.array_equal(bits(x), bits(y))
    assert 0 < int(s[0].shape[0]) < 700


def test_the_cloud_of_the_dense_kernel(dens, twin):
    dens.upload_cameras(sc.cameras())
    refs = [sc.reference_inputs(r, 3, 48, 64, device=DEV)[1] for r in (10, 11, 12, 13)]
    out = dens.triangulate_dense(hb.PreparedBatch(refs, sc.MATCH, sc.MATCH), sc.params())
    counts = np.diff(np.asarray(out.ref_offsets))
    assert counts.shape == (4,) and counts.min() > 1000
    d = dens.consensus_filter(out.xyz, out.rgb, out.err, counts, 0.05, 2, True)
    h = twin.consensus_filter(out.xyz.cpu(), out.rgb.cpu(), out.err.cpu(), counts, 0.05, 2, True)
    for x, y in zip(d, h):
        assert np.array_equal(bits(x), bits(y))
    c = d[4].cpu().numpy()
    assert 0.1 * c.size < (c >= 2).sum() < 0.9 * c.size and c.max() == 3
    dens.check_launches()


def test_both_contexts_refuse_each_other_s_entry_point(dens, twin):
    lib = hb.load_library()
    null = (None, None, None, 0, None, 1, 1.0, 1, None, None, None, None, None, None)
    assert lib.lfd_consensus_filter_host(dens._ctx, *null) == LFD_ERR_STATE and lib.lfd_last_error(dens._ctx)
    assert lib.lfd_consensus_filter(twin._ctx, *null) == LFD_ERR_STATE
    with pytest.raises(ValueError, match="on cuda"):
        dens.consensus_filter(torch.zeros(4, 3), None, None, [4], 1.0, 1)
    wide = torch.from_numpy((np.random.default_rng(0).uniform(-1, 1, (500, 3)) * 5000.0).astype(np.float32)).to(DEV)
    with pytest.raises(hb.ConsensusInputRefused, match="key range"):
        dens.consensus_filter(wide, None, None, [200, 300], 1e-4, 1)
    with pytest.raises(hb.HipBackendError, match="min_refs") as e:
        dens.consensus_filter(wide, None, None, [200, 300], 1.0, 0)
    assert not isinstance(e.value, hb.ConsensusInputRefused)


@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_the_driver_on_the_device_writes_the_host_run_s_file(tmp_path_factory, mode):
    """The tie-free, noise-free slab scene of tests/cycle_scene.py (see tests/test_gpu_cycle_gate.py for why): one run of the GUI entry point per
    backend with the filter on; the files are compared byte for byte."""
    import cycle_scene
    from test_consensus_driver import RADIUS, gui_run
    root = str(tmp_path_factory.mktemp("consensus_gpu"))
    scene = cycle_scene.make_scene(root)
    kw = dict(occlusion_steps=True, out_of_range=0.3, noise_px=0.0, outlier_frac=0.0, cert_mode="tiefree")
    exp = {"min_consensus_refs": 1, "consensus_radius": RADIUS[mode]}
    host_out, dev_out, off_out = (os.path.join(root, name) for name in ("host.ply", "dev.ply", "off.ply"))
    assert gui_run(scene, host_out, mode, exp, matcher_kw=kw) == (0, host_out)
    assert gui_run(scene, dev_out, mode, exp, backend="device", device=DEV, matcher_kw=kw) == (0, dev_out)
    assert gui_run(scene, off_out, mode, {}, backend="device", device=DEV, matcher_kw=kw) == (0, off_out)
    host, dev, off = (open(p, "rb").read() for p in (host_out, dev_out, off_out))
    count = lambda raw: int(raw.split(b"element vertex ")[1].split(b"\n")[0])              # noqa: E731
    body = lambda raw: np.frombuffer(raw.split(b"end_header\n", 1)[1], np.uint8)            # noqa: E731
    print(f"{mode}: host {count(host)} points, device {count(dev)} (filter off: {count(off)}); bytes that differ: "
          f"{int((body(host) != body(dev)).sum()) if count(host) == count(dev) else 'n/a'}")
    assert 0 < count(dev) < count(off)
    assert dev == host
