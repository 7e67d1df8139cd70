"""The connected-component filter on the device (lfd_component_filter through HipDensifier.component_filter) against the CPU twin - both sides
are given the SAME cloud - at the smallest sizes that take every path: one lane, one workgroup and a ragged second one, thousands of points in
one cell, a 2 000-point chain whose neighbouring links the sort puts into different workgroups, a lattice whose 4 096 points are all united
into one root, many workgroups and several radix passes, non-finite points, empty references, no points.  The partition of a graph into
components does not depend on the order in which the thousands of concurrent unions happen, so every output - size and label of every point,
the summary, kept points, colours, errors, per-reference counts - equals the sequential twin's bit for bit; so does a second launch, a launch
after a larger one and, through the driver, the written file.  (The twin itself is held against the brute-force reference on the CPU tier.)"""
import os

import numpy as np
import pytest
import torch

import component_cases as cases
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


def travel(n, seed=1):
    rng = np.random.default_rng(seed)
    rgb, err = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32), rng.uniform(0.0, 2.0, (n,)).astype(np.float32)
    if n > 9:
        rgb[5, 0], err[9] = np.nan, np.inf                                                     # what travels along is copied, not looked at
    return rgb, err


def both(dens, twin, xyz, counts, radius, m, sizes=True, labels=True, rgb=None, err=None):
    """one call on each side over the same cloud; returns the device's outputs after comparing every one of them with the twin's"""
    t = lambda a, dev: torch.from_numpy(np.ascontiguousarray(a)).to(dev) if a is not None else None      # noqa: E731
    d = dens.component_filter(t(xyz, DEV), t(rgb, DEV), t(err, DEV), counts, radius, m, sizes, labels)
    h = twin.component_filter(t(xyz, "cpu"), t(rgb, "cpu"), t(err, "cpu"), counts, radius, m, sizes, labels)
    for i, name in enumerate(("xyz", "rgb", "err", "kept", "size", "label", "summary")):
        assert (d[i] is None) == (h[i] is None), name
        if d[i] is not None:
            assert tuple(d[i].shape) == tuple(h[i].shape) and np.array_equal(bits(d[i]), bits(h[i])), name
    assert (d[4] is None) == (not sizes) and (d[5] is None) == (not labels)
    return d


def every_way(dens, twin, xyz, counts, radius, m):
    """with and without rgb / err, with and without size / label: the kept set is the same"""
    rgb, err = travel(xyz.shape[0])
    d = both(dens, twin, xyz, counts, radius, m, True, True, rgb, err)
    for sizes, labels, r, e in ((False, False, None, None), (True, False, rgb, None), (False, True, None, err)):
        k = both(dens, twin, xyz, counts, radius, m, sizes, labels, r, e)
        assert np.array_equal(bits(d[0]), bits(k[0])) and np.array_equal(d[3], k[3]) and np.array_equal(d[6], k[6])
    s = d[4].cpu().numpy()
    assert int(d[0].shape[0]) == int((s >= m).sum()) and int(d[6][34:].sum()) == xyz.shape[0]
    return d


@pytest.mark.parametrize("n,radius", [(1, 0.5), (2, 3.0), (257, 0.15), (257, 0.3)])      # 257: one workgroup and a ragged second one
def test_small_clouds_equal_the_twin(dens, twin, n, radius):
    xyz = np.random.default_rng(n).uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    counts = [n // 3, 0, n - n // 3]
    d = every_way(dens, twin, xyz, counts, radius, 2)
    every_way(dens, twin, xyz, counts, radius, 40)
    if n == 257:
        assert 1 < int(d[6][1]) and int(d[6][0]) > 1                      # neither all singletons nor one component


def test_five_thousand_points_in_one_cell(dens, twin):
    xyz, counts, radius = cases.one_cell(5000)
    d = every_way(dens, twin, xyz, counts, radius, 2501)
    assert int(d[0].shape[0]) == 0 and d[6][:2].tolist() == [2, 2500]
    assert int(every_way(dens, twin, xyz, counts, radius, 2500)[0].shape[0]) == 5000
    uni = np.random.default_rng(2).uniform(0.0, 1.0, (5000, 3)).astype(np.float32)          # ... and one cell that is one component
    assert every_way(dens, twin, uni, [5000], 1.0, 2)[6][:2].tolist() == [1, 5000]


@pytest.mark.parametrize("gap_at", [None, 1237])
def test_the_chain(dens, twin, gap_at):
    line, radius = cases.chain(2000, gap_at)
    perm = np.random.default_rng(3).permutation(2000)
    for xyz in (line[perm], line):
        for m in ((1999, 2000, 2001) if gap_at is None else (763, 764, 1237, 1238)):
            d = both(dens, twin, xyz, [700, 0, 1300], radius, m)
        assert d[6][0] == (1 if gap_at is None else 2) and d[6][1] == (2000 if gap_at is None else 1237)


def test_the_lattice_with_singletons_and_clumps(dens, twin):
    xyz, counts, radius, want = cases.lattice_with_clumps()
    for m in (2, 40, 41, 4096, 4097):
        d = every_way(dens, twin, xyz, counts, radius, m)
    assert np.array_equal(d[4].cpu().numpy(), want) and d[6][:2].tolist() == [241, 4096]


def test_the_small_cases_of_the_host_tier(dens, twin):
    from test_component_host import sheets_and_clumps
    just_over = np.nextafter(np.float32(0.5), np.float32(1.0))
    assert both(dens, twin, np.array([[0, 0, 0], [0.5, 0, 0]], np.float32), [2], 0.5, 2)[4].cpu().tolist() == [2, 2]      # the f32 boundary of the link
    assert both(dens, twin, np.array([[0, 0, 0], [just_over, 0, 0]], np.float32), [1, 1], 0.5, 2)[4].cpu().tolist() == [1, 1]
    one_cell = np.array([[0, 0, 0], [0.9, 0.9, 0.9], [0.05, 0, 0], [0.9, 0.9, 0.95]], np.float32)      # further apart than the radius inside one cell
    assert both(dens, twin, one_cell, [4], 1.0, 2)[5].cpu().tolist() == [0, 1, 0, 1]
    spot = np.tile(np.array([[1.5, -2.0, 0.25]], np.float32), (300, 1))
    assert both(dens, twin, spot, [100, 200], 1e-3, 300)[6][:2].tolist() == [1, 300]
    for d in np.stack(np.meshgrid([-1, 0, 1], [-1, 0, 1], [-1, 0, 1], indexing="ij"), -1).reshape(-1, 3):      # across a cell border, 26 directions
        if d.any():
            base = np.array([10.3, -4.2, 0.9])
            for off in (0.0, 0.5, 1.0):
                xyz = np.array([base - 3.0, base + off * d, base + d * 0.55 / np.linalg.norm(d) + off * d], np.float32)
                assert sorted(both(dens, twin, xyz, [1, 2], 1.0, 2)[4].cpu().tolist()) == [1, 2, 2], (d, off)
    xyz, counts, clump, radius = sheets_and_clumps()
    d = both(dens, twin, xyz, counts, radius, 31)
    assert np.array_equal(bits(d[0]), bits(xyz[~clump]))                   # every clump goes, the one-reference sheet stays


def direct(lib, ctx, dev, xyz, counts, radius, m, sizes, labels, with_summary):
    """lfd_component_filter[_host] through ctypes, the summary pointer null or not (the binding always hands one over): the kept rows, the
    offsets, size, label (None where not asked for) and the summary (None without one)"""
    import ctypes as C
    fn = lib.lfd_component_filter if dev.type == "cuda" else lib.lfd_component_filter_host
    n = xyz.shape[0]
    x = torch.from_numpy(xyz).to(dev)
    xo = torch.empty_like(x)
    size = torch.full((n,), -1, dtype=torch.int32, device=dev) if sizes else None
    label = torch.full((n,), -1, dtype=torch.int32, device=dev) if labels else None
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    offs_out = np.full_like(offs, -1)
    summ = np.full(66, -1, np.int64) if with_summary else None
    n_out = C.c_int64(-1)
    i64p = C.POINTER(C.c_int64)
    ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
    rc = fn(ctx, ptr(x), None, None, n, offs.ctypes.data_as(i64p), len(counts), C.c_float(radius), m, ptr(xo), None, None, offs_out.ctypes.data_as(i64p),
            ptr(size), ptr(label), summ.ctypes.data_as(i64p) if with_summary else None, C.byref(n_out))
    assert rc == 0, lib.lfd_last_error(ctx)
    u32 = lambda t: t.cpu().numpy().view(np.uint32) if t is not None else None      # noqa: E731
    return bits(xo[:n_out.value]), offs_out, u32(size), u32(label), summ


@pytest.mark.parametrize("sizes,labels", [(True, True), (False, False), (True, False), (False, True)])
def test_without_the_summary_every_other_output_is_the_same(dens, twin, sizes, labels):
    lib = hb.load_library()
    xyz, counts = cases.clustered(20011, 5, 13)                            # 79 workgroups, a ragged last one
    radius, m = 0.006, 20
    on = direct(lib, dens._ctx, DEV, xyz, counts, radius, m, sizes, labels, True)
    off = direct(lib, dens._ctx, DEV, xyz, counts, radius, m, sizes, labels, False)
    host_on = direct(lib, twin._ctx, torch.device("cpu"), xyz, counts, radius, m, sizes, labels, True)
    host_off = direct(lib, twin._ctx, torch.device("cpu"), xyz, counts, radius, m, sizes, labels, False)
    assert off[4] is None and host_off[4] is None and np.array_equal(on[4], host_on[4]) and on[4][0] > 1 and on[4][34:].sum() == 20011
    assert 0 < on[0].shape[0] < 20011 and on[1][-1] == on[0].shape[0]
    for other in (off, host_on, host_off):
        for a, b, name in zip(on[:4], other[:4], ("kept rows", "offsets", "size", "label")):
            assert (a is None) == (b is None) and (a is None or np.array_equal(a, b)), name
    assert (on[2] is None) == (not sizes) and (on[3] is None) == (not labels)


def test_non_finite_points_empty_references_and_no_points(dens, twin):
    xyz, _ = cases.clustered(2000, 2, 5)
    d = every_way(dens, twin, xyz, [0, 0, 500, 0, 1500, 0], 0.02, 3)
    assert 0 < int(d[0].shape[0]) < 2000 and not d[3][[0, 1, 3, 5]].any()
    bad = xyz.copy()
    at = np.random.default_rng(6).choice(2000, 90, replace=False)
    bad[at[:30], 0], bad[at[30:60], 2], bad[at[60:], 1] = np.nan, np.inf, -np.inf
    d = every_way(dens, twin, bad, [2000], 0.02, 2)
    assert (d[4].cpu().numpy()[at] == 1).all() and np.array_equal(d[5].cpu().numpy()[at], at)
    d = every_way(dens, twin, np.full((300, 3), np.nan, np.float32), [100, 200], 1.0, 2)
    assert int(d[0].shape[0]) == 0 and d[6][:3].tolist() == [300, 1, 300]
    z3 = np.zeros((0, 3), np.float32)
    d = both(dens, twin, z3, [0, 0, 0], 1.0, 2, True, True, z3, np.zeros((0,), np.float32))
    assert d[0].shape == (0, 3) and d[3].tolist() == [0, 0, 0] and not d[6].any()


@pytest.fixture(scope="module")
def big():
    """200 000 clustered points of 7 references; at radius 0.004 the grid has some 4e9 cells: four radix passes, 782 workgroups"""
    xyz, counts = cases.clustered(200000, 7, 7)
    return xyz, counts, 0.004


def test_a_clustered_cloud_of_many_workgroups_and_radix_passes(dens, twin, big):
    xyz, counts, radius = big
    rgb, err = travel(xyz.shape[0])
    d = both(dens, twin, xyz, counts, radius, 50, True, True, rgb, err)
    s = d[6]
    print(f"200 000 points: {s[0]} components, largest {s[1]}, {int(d[0].shape[0])} kept at 50")
    assert 0 < int(d[0].shape[0]) < 200000 and s[0] > 1000 and s[1] > 1000
    both(dens, twin, xyz, counts, radius, 2, False, False)


def test_two_launches_give_equal_bits_and_a_smaller_launch_reuses_the_workspace(dens, twin, big):
    xyz, counts, radius = big
    small, scounts = cases.clustered(700, 5, 10)
    a = both(dens, twin, xyz, counts, radius, 50)
    s = both(dens, twin, small, scounts, 0.02, 3)                                          # after a larger one: the workspace holds stale words behind it
    b = both(dens, twin, xyz, counts, radius, 50)
    for x, y in zip(a, b):
        assert np.array_equal(bits(x), bits(y))
    assert 0 < int(s[0].shape[0]) < 700


def test_both_contexts_refuse_each_other_s_entry_point(dens, twin):
    lib = hb.load_library()
    null = (None, None, None, 0, None, 1, 1.0, 2, None, None, None, None, None, None, None, None)
    assert lib.lfd_component_filter_host(dens._ctx, *null) == LFD_ERR_STATE and lib.lfd_last_error(dens._ctx)
    assert lib.lfd_component_filter(twin._ctx, *null) == LFD_ERR_STATE
    with pytest.raises(ValueError, match="on cuda"):
        dens.component_filter(torch.zeros(4, 3), None, None, [4], 1.0, 2)
    wide = torch.from_numpy((np.random.default_rng(0).uniform(-1, 1, (500, 3)) * 5000.0).astype(np.float32)).to(DEV)
    with pytest.raises(hb.ConsensusInputRefused, match="key range"):
        dens.component_filter(wide, None, None, [200, 300], 1e-4, 2)
    with pytest.raises(hb.HipBackendError, match="min_points") as e:
        dens.component_filter(wide, None, None, [200, 300], 1.0, 1)
    assert not isinstance(e.value, hb.ConsensusInputRefused)


def test_the_driver_on_the_device_writes_the_host_run_s_file(tmp_path_factory):
    """The tie-free, noise-free slab scene of tests/cycle_scene.py (see tests/test_gpu_cycle_gate.py for why): one run of the GUI entry point per
    backend with the filter on and normals; the files and the reports are compared byte for byte."""
    import cycle_scene
    from test_component_driver import ON
    from test_consensus_driver import gui_run
    root = str(tmp_path_factory.mktemp("component_gpu"))
    scene = cycle_scene.make_scene(root)
    kw = dict(occlusion_steps=True, out_of_range=0.3, noise_px=0.0, outlier_frac=0.0, cert_mode="tiefree")
    exp = {**ON, "estimate_normals": True}
    host_out, dev_out, off_out = (os.path.join(root, name) for name in ("host.ply", "dev.ply", "off.ply"))
    assert gui_run(scene, host_out, "sampled", exp, matcher_kw=kw) == (0, host_out)
    assert gui_run(scene, dev_out, "sampled", exp, backend="device", device=DEV, matcher_kw=kw) == (0, dev_out)
    assert gui_run(scene, off_out, "sampled", {"estimate_normals": True}, backend="device", device=DEV, matcher_kw=kw) == (0, off_out)
    host, dev, off = (open(p, "rb").read() for p in (host_out, dev_out, off_out))
    count = lambda raw: int(raw.split(b"element vertex ")[1].split(b"\n")[0])              # noqa: E731
    print(f"host {count(host)} points, device {count(dev)} (filter off: {count(off)})")
    assert 0 < count(dev) < count(off)
    assert dev == host
    assert open(dev_out + ".components.json", "rb").read() == open(host_out + ".components.json", "rb").read()
    assert not os.path.exists(off_out + ".components.json")
