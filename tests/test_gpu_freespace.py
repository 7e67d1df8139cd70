"""The free-space filter on the device (lfd_freespace_filter through HipDensifier.freespace_filter) against the CPU twin - both sides are given
the SAME cloud and cameras - at the smallest sizes that take every path: one lane, one workgroup and a ragged second one, many workgroups with
reference boundaries inside them, a 1 x 1 plane on which every splat collides, more references than any chunk of cameras, non-finite points only,
empty references, a single reference, no points.  Every output - the two counts, kept points, colours, errors, per-reference counts - equals the
twin's bit for bit (f64 projection and f32 test with every rounding written out; an integer minimum does not depend on the order), so does a
second launch, a launch after a larger one, the cloud the dense kernel made and, through the driver, the written file."""
import os

import numpy as np
import pytest
import torch

import freespace_ref as fr
import freespace_scene as fs
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


def travel(n, seed):
    rng = np.random.default_rng(seed)
    rgb, err = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32), rng.uniform(0.0, 2.0, (n,)).astype(np.float32)
    if n > 9:
        rgb[5, 0], err[9] = np.nan, np.inf                                 # what travels along is copied, not looked at
    return rgb, err


def both(dens, twin, xyz, counts, P, wh, plane, tol, m, with_counts=True, along=True):
    """one call on each side over the same cloud; returns the device's outputs after comparing every one of them with the twin's"""
    t = lambda a, dev: torch.from_numpy(np.ascontiguousarray(a)).to(dev) if a is not None else None      # noqa: E731
    rgb, err = travel(len(xyz), len(xyz)) if along else (None, None)
    d = dens.freespace_filter(t(xyz, DEV), t(rgb, DEV), t(err, DEV), counts, P, wh, plane, tol, m, with_counts)
    h = twin.freespace_filter(t(xyz, "cpu"), t(rgb, "cpu"), t(err, "cpu"), counts, P, wh, plane, tol, m, with_counts)
    for i, name in enumerate(("xyz", "rgb", "err")):
        assert (d[i] is None) == (h[i] is None), name
        if d[i] is not None:
            assert d[i].shape == h[i].shape and np.array_equal(bits(d[i]), bits(h[i])), name
    assert np.array_equal(d[3], h[3])
    for i in (4, 5):
        assert (d[i] is None) == (h[i] is None) == (not with_counts)
        if with_counts:
            assert np.array_equal(bits(d[i]), bits(h[i])), ("violations", "supports")[i - 4]
    return d


@pytest.mark.parametrize("n", [1, 2, 257, 5000])
@pytest.mark.parametrize("plane", [(8, 6), (96, 62)])
def test_small_clouds_equal_the_twin(dens, twin, n, plane):
    xyz, counts, P, wh = fs.ring_cloud(7, n, seed=n)
    for m in (1, 2):
        d = both(dens, twin, xyz, counts, P, wh, plane, 0.02, m, True)
        k = both(dens, twin, xyz, counts, P, wh, plane, 0.02, m, False, along=False)
        assert np.array_equal(bits(d[0]), bits(k[0])) and np.array_equal(d[3], k[3])      # the same kept set with and without the counts
        v, s = d[4].cpu().numpy().astype(np.int64), d[5].cpu().numpy().astype(np.int64)
        assert int(d[0].shape[0]) == int(fr.keep_mask(v, s, m).sum())
    if n == 5000:
        assert 0 < int(d[0].shape[0]) < n and v.max() >= 3 and s.max() >= 3


@pytest.mark.parametrize("m,with_counts", [(1, True), (3, False)])
def test_a_clustered_cloud_of_many_workgroups(dens, twin, m, with_counts):
    xyz, counts, P, wh = fs.ring_cloud(40, 100003, seed=7, clustered=True)                    # 391 workgroups, reference boundaries inside them
    assert (np.cumsum(counts)[:-1] % 256 != 0).sum() >= 30
    d = both(dens, twin, xyz, counts, P, wh, (64, 41), 0.02, m, with_counts)
    assert 0 < int(d[0].shape[0]) < 100003


def test_every_splat_collides_on_a_one_cell_plane(dens, twin):
    xyz, counts, P, wh = fs.ring_cloud(5, 3000, seed=3)
    d = both(dens, twin, xyz, counts, P, wh, (1, 1), 0.02, 1)
    assert 0 < int(d[0].shape[0]) < 3000
    both(dens, twin, xyz, counts, P, wh, (1, 1), 0.2, 2, False)


def test_three_hundred_references(dens, twin):
    from test_freespace_host import saturating_cloud
    xyz, counts, P, wh = saturating_cloud(300)                                            # beyond any chunk of cameras a kernel could stage
    assert counts.tolist() == [10] * 300
    d = both(dens, twin, xyz, counts, P, wh, (8, 6), 0.02, 255)
    assert d[4][0].item() == 255 and d[3][0] == 9 and int(d[0].shape[0]) == 2999


def test_non_finite_points_empty_references_a_single_reference_and_no_points(dens, twin):
    xyz, counts, P, wh = fs.ring_cloud(9, 2000, seed=5, empty=(0, 1, 4, 8))
    assert counts[[0, 1, 4, 8]].tolist() == [0, 0, 0, 0]
    d = both(dens, twin, xyz, counts, P, wh, (96, 62), 0.02, 1)
    assert 0 < int(d[0].shape[0]) < 2000 and not d[3][[0, 1, 4, 8]].any()
    d = both(dens, twin, xyz, [2000], P[:1], wh[:1], (96, 62), 0.02, 1)
    assert int(d[0].shape[0]) == 2000 and not d[4].any() and not d[5].any()
    bad = xyz.copy()
    at = np.random.default_rng(6).choice(2000, 90, replace=False)
    bad[at[:30], 0], bad[at[30:60], 2], bad[at[60:], 1] = np.nan, np.inf, -np.inf
    d = both(dens, twin, bad, counts, P, wh, (96, 62), 0.02, 1)
    assert not d[4].cpu().numpy()[at].any() and not d[5].cpu().numpy()[at].any() and 0 < int(d[0].shape[0]) < 2000
    only = np.full((300, 3), np.nan, np.float32)
    only[100:200], only[200:] = np.inf, 1e30
    d = both(dens, twin, only, [100, 150, 50], P[:3], wh[:3], (8, 6), 0.02, 1)
    assert int(d[0].shape[0]) == 300 and not d[4].any() and not d[5].any()
    d = both(dens, twin, np.zeros((0, 3), np.float32), [0, 0, 0], P[:3], wh[:3], (8, 6), 0.02, 1)
    assert d[0].shape == (0, 3) and d[3].tolist() == [0, 0, 0]


def test_two_launches_give_equal_bits_and_the_z_buffers_are_refilled(dens, twin):
    big = fs.ring_cloud(12, 20000, seed=9)
    small = fs.ring_cloud(5, 700, seed=10)
    a = both(dens, twin, *big, (96, 62), 0.02, 2)
    s = both(dens, twin, *small, (96, 62), 0.02, 1)            # after a larger one with another cloud: stale depths would lie in the same planes
    b = both(dens, twin, *big, (96, 62), 0.02, 2)
    for x, y in zip(a, b):
        assert np.array_equal(bits(x), bits(y))
    fresh = hb.HipDensifier(DEV)
    try:
        t = lambda arr: torch.from_numpy(arr).to(DEV)            # noqa: E731
        f = fresh.freespace_filter(t(small[0]), None, None, small[1], small[2], small[3], (96, 62), 0.02, 1, True)
    finally:
        fresh.close()
    assert np.array_equal(bits(f[0]), bits(s[0])) and np.array_equal(bits(f[4]), bits(s[4])) and np.array_equal(bits(f[5]), bits(s[5]))
    assert 0 < int(s[0].shape[0]) < 700


def test_the_cloud_of_the_dense_kernel(dens, twin):
    cams = sc.cameras()
    dens.upload_cameras(cams)
    ref_ids = (10, 11, 12, 13)
    refs = [sc.reference_inputs(r, 3, 48, 64, device=DEV)[1] for r in ref_ids]
    out = dens.triangulate_dense(hb.PreparedBatch(refs, sc.MATCH, sc.MATCH), sc.params())
    counts = np.diff(np.asarray(out.ref_offsets))
    assert counts.shape == (4,) and counts.min() > 1000
    P, wh = fr.cameras(cams, ref_ids)
    d = dens.freespace_filter(out.xyz, out.rgb, out.err, counts, P, wh, (64, 48), 0.02, 1, True)
    h = twin.freespace_filter(out.xyz.cpu(), out.rgb.cpu(), out.err.cpu(), counts, P, wh, (64, 48), 0.02, 1, True)
    for x, y in zip(d, h):
        assert np.array_equal(bits(x), bits(y))
    assert d[5].cpu().numpy().max() >= 1
    dens.check_launches()


def test_both_contexts_refuse_each_other_s_entry_point(dens, twin):
    lib = hb.load_library()
    null = (None, None, None, 0, None, 1, None, None, 1, 1, 0.02, 1, None, None, None, None, None, None, None)
    assert lib.lfd_freespace_filter_host(dens._ctx, *null) == LFD_ERR_STATE and lib.lfd_last_error(dens._ctx)
    assert lib.lfd_freespace_filter(twin._ctx, *null) == LFD_ERR_STATE
    _xyz, _counts, P, wh = fs.ring_cloud(2, 4, seed=1)
    with pytest.raises(ValueError, match="on cuda"):
        dens.freespace_filter(torch.zeros(4, 3), None, None, [4, 0], P, wh, (8, 6), 0.02, 1)
    with pytest.raises(hb.HipBackendError, match="tol"):
        dens.freespace_filter(torch.zeros(4, 3, device=DEV), None, None, [4, 0], P, wh, (8, 6), 1.0, 1)


@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_the_driver_on_the_device_writes_the_host_run_s_file(tmp_path_factory, mode):
    """The tie-free, noise-free slab scene of tests/cycle_scene.py (see tests/test_gpu_cycle_gate.py for why): one run of the GUI entry point per
    backend with the filter on; the files are compared byte for byte."""
    import cycle_scene
    from test_freespace_driver import ON, gui_run
    root = str(tmp_path_factory.mktemp("freespace_gpu"))
    scene = cycle_scene.make_scene(root)
    kw = dict(occlusion_steps=True, out_of_range=0.3, noise_px=0.0, outlier_frac=0.0, cert_mode="tiefree")
    host_out, dev_out, off_out = (os.path.join(root, name) for name in ("host.ply", "dev.ply", "off.ply"))
    assert gui_run(scene, host_out, mode, ON, matcher_kw=kw) == (0, host_out)
    assert gui_run(scene, dev_out, mode, ON, backend="device", device=DEV, matcher_kw=kw) == (0, dev_out)
    assert gui_run(scene, off_out, mode, {}, backend="device", device=DEV, matcher_kw=kw) == (0, off_out)
    host, dev, off = (open(p, "rb").read() for p in (host_out, dev_out, off_out))
    count = lambda raw: int(raw.split(b"element vertex ")[1].split(b"\n")[0])              # noqa: E731
    body = lambda raw: np.frombuffer(raw.split(b"end_header\n", 1)[1], np.uint8)            # noqa: E731
    print(f"{mode}: host {count(host)} points, device {count(dev)} (filter off: {count(off)}); bytes that differ: "
          f"{int((body(host) != body(dev)).sum()) if count(host) == count(dev) else 'n/a'}")
    assert 0 < count(dev) < count(off)
    assert dev == host
