"""The Gaussian-ready output on the device (lfd_knn_dist2 and lfd_pack_gaussians through HipDensifier) against the CPU twin,
both sides given the SAME arrays: dist2 EQUAL bit for bit and the statistics equal, on every cloud of the issue and under the forced cell sizes
that send a cloud through every ring and through the brute-force kernel; the packed records equal bit for bit in every column but the three
scales and the four rot values, which may differ by one f32 ulp (the number of values that differ at all is printed); the refusals; and one
end-to-end run of the driver on the device whose file is compared with the host backend's under the same column rule."""
import os

import numpy as np
import pytest
import torch

import knn_ref as kr
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
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def tensor(a, dev):
    return torch.from_numpy(np.array(a, dtype=np.float32, copy=True)).to(dev)


def both(dens, twin, xyz, h=0.0):
    x = tensor(xyz, DEV)
    keep = x.clone()
    d = dens.knn_dist2(x, h)
    w = twin.knn_dist2(tensor(xyz, "cpu"), h)
    assert np.array_equal(bits(x), bits(keep))                          # the input is read only
    assert d.is_cuda and d.dtype == torch.float32 and d.shape == w.shape
    diff = int((bits(d) != bits(w)).sum())
    assert diff == 0, (h, diff)
    assert dens.knn_stats == twin.knn_stats, (dens.knn_stats, twin.knn_stats)
    return d, dens.knn_stats


@pytest.mark.parametrize("name", kr.ALL)
def test_dist2_and_stats_equal_the_twin_for_every_cell_size(dens, twin, name):
    xyz = kr.cloud(name)
    for h in kr.cell_sizes(name):
        d, stats = both(dens, twin, xyz, h)
        assert np.array_equal(bits(d), bits(kr.reference(name)))        # ... and both are the brute-force reference
        print(name, "cell size", h, "stats", stats)
    if name.startswith("f"):
        both(dens, twin, xyz)
        assert dens.knn_stats[3] <= 0.01 * xyz.shape[0]
    if name.startswith("g"):
        both(dens, twin, xyz)
        assert dens.knn_stats[2] <= 64 and dens.knn_stats[3] <= 16


def test_the_workspace_is_shared_between_calls_of_different_sizes(dens, twin):
    first, _ = both(dens, twin, kr.cloud("b257"))
    first = first.clone()
    both(dens, twin, kr.cloud("g0"))
    again, _ = both(dens, twin, kr.cloud("b257"))
    assert np.array_equal(bits(first), bits(again))


def test_refusals_and_the_other_context_s_entry_points(dens, twin):
    d = dens.knn_dist2(torch.zeros((0, 3), dtype=torch.float32, device=DEV))
    assert d.shape == (0,) and dens.knn_stats == (0.0, 0, 0, 0)
    with pytest.raises(hb.KnnInputRefused, match="fewer than four points"):
        dens.knn_dist2(tensor(kr.cloud("a5")[:3], DEV))
    bad = np.array(kr.cloud("b65"), copy=True)
    bad[64, 2] = np.inf
    with pytest.raises(hb.KnnInputRefused, match="non-finite coordinate"):
        dens.knn_dist2(tensor(bad, DEV))
    with pytest.raises(hb.KnnInputRefused, match="key range"):
        dens.knn_dist2(tensor(kr.cloud("b65"), DEV), 1e-12)
    with pytest.raises(hb.KnnInputRefused, match="key range"):
        dens.knn_dist2(tensor(kr.cloud("b65"), DEV), 3e-8)
    both(dens, twin, kr.cloud("b65"))                                   # the context still works behind the refusals
    assert dens._lib.lfd_knn_dist2_host(dens._ctx, None, 0, 0.0, None, None) == LFD_ERR_STATE
    assert twin._lib.lfd_knn_dist2(twin._ctx, None, 0, 0.0, None, None) == LFD_ERR_STATE
    null = (None, None, None, None, 0, 0.0, 0.0, 0.0, None)
    assert dens._lib.lfd_pack_gaussians_host(dens._ctx, *null) == LFD_ERR_STATE
    assert twin._lib.lfd_pack_gaussians(twin._ctx, *null) == LFD_ERR_STATE


def compare_records(got: np.ndarray, want: np.ndarray, tag: str):
    """the column rule of the issue; returns how many of the seven loose values differ at all"""
    assert got.shape == want.shape
    strict = {col: int((np.ascontiguousarray(got[col]).view(np.uint32) != np.ascontiguousarray(want[col]).view(np.uint32)).sum())
              for col in ("xyz", "normal", "f_dc", "opacity")}
    print(f"{tag}: values that differ in the columns that must be equal: {strict}")
    for col in ("xyz", "normal", "f_dc", "opacity"):
        assert got[col].tobytes() == want[col].tobytes(), (tag, col)
    loose = 0
    for col in ("scale", "rot"):
        ok = np.isfinite(want[col])
        assert np.array_equal(np.isfinite(got[col]), ok), (tag, col)
        d = kr.ulp_distance(np.where(ok, got[col], 0), np.where(ok, want[col], 0))
        assert d.max(initial=0) <= 1, (tag, col, int(d.max()))
        loose += int((d != 0).sum())
    print(f"{tag}: {loose} of {7 * got.shape[0]} scale / rot values differ from the twin's (by one ulp)")
    return loose


def pack_inputs(seed, n):
    rs = np.random.RandomState(seed)
    xyz = rs.uniform(-2, 2, (n, 3)).astype(np.float32)
    nrm = rs.normal(size=(n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    nrm[:5] = [(0, 0, -1), (0, 0, 1), (0, 0, 0), (np.nan, 0, 1), (1, 0, 0)]
    nrm[5] = (np.float32(3e-4), 0, np.float32(-1.0) + np.float32(2.0 ** -24))
    nrm[6] = (np.float32(5e-4), 0, np.float32(-1.0) + np.float32(2.0 ** -23))
    rgb = rs.uniform(-0.1, 1.1, (n, 3)).astype(np.float32)
    rgb[7] = (np.nan, 0.5, np.float32(0.5 / 255.0))
    d2 = (rs.uniform(0, 1, n) ** 4).astype(np.float32)
    d2[:3] = (0.0, 1e-9, 1e-7)
    return xyz, nrm, rgb, d2


@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
@pytest.mark.parametrize("knobs", [dict(), dict(opacity=0.3, flatten=0.1, max_scale=0.05)])
def test_packed_records_against_the_twin(dens, twin, n, knobs):
    ins = pack_inputs(n, max(n, 8))
    ins = tuple(a[:n] for a in ins)
    got = dens.pack_gaussians(*(tensor(a, DEV) for a in ins), **knobs)
    want = twin.pack_gaussians(*(tensor(a, "cpu") for a in ins), **knobs)
    assert got.is_cuda and got.shape == (68 * n,)
    compare_records(np.frombuffer(got.cpu().numpy().tobytes(), kr.REC68), np.frombuffer(want.numpy().tobytes(), kr.REC68), f"n = {n}")


def test_the_records_of_a_cloud_and_its_own_distances(dens, twin):
    xyz = kr.cloud("g0")
    rs = np.random.RandomState(3)
    nrm = rs.normal(size=xyz.shape)
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    rgb = rs.uniform(0, 1, xyz.shape).astype(np.float32)
    d, _ = both(dens, twin, xyz)
    got = dens.pack_gaussians(tensor(xyz, DEV), tensor(nrm, DEV), tensor(rgb, DEV), d, flatten=0.25)
    want = twin.pack_gaussians(tensor(xyz, "cpu"), tensor(nrm, "cpu"), tensor(rgb, "cpu"), d.cpu(), flatten=0.25)
    compare_records(np.frombuffer(got.cpu().numpy().tobytes(), kr.REC68), np.frombuffer(want.numpy().tobytes(), kr.REC68), "cloud (g)")


@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_the_driver_on_the_device_writes_the_host_backend_s_file(tmp_path, mode):
    """dense_init with estimate_normals + gaussian_init, device backend against host backend: the same header, and the records under the column
    rule.  The scene keeps the comparison about this stage, as tests/test_gpu_cycle_gate.py's does: the same matcher fields in both runs (made on the
    host, moved to the device by the driver), tie-free certainties (the host sampling orders tied weights with an unstable argsort) and no noise
    (every two-view error far from its threshold, where the twin's IEEE division and the kernels' refined reciprocal cannot flip a survivor)."""
    import cycle_scene
    from lichtfeld_densification_plugin_amd import densify
    scene = cycle_scene.make_scene(str(tmp_path / "scene"), n_cams=4)

    def run(backend, name):
        args = densify.build_argparser().parse_args(["--scene_root", scene["root"], "--images_subdir", "images_4", "--num_refs", "0.75", "--nns_per_ref", "3",
                                                     "--matches_per_ref", "2500", "--seed", "3", "--pack_workers", "1", "--backend", backend,
                                                     "--triangulation_mode", mode, "--max_points", "5000", "--out_name", name, "--estimate_normals",
                                                     "--gaussian_init", "--gaussian_flatten", "0.2"])
        matcher = cycle_scene.matcher_for(scene, noise_px=0.0, outlier_frac=0.0, cert_mode="tiefree")
        kw = {"device": DEV} if backend == "device" else {}
        assert densify.dense_init(args, matcher=matcher, **kw) == 0
        head, body = open(os.path.join(scene["root"], "sparse", "0", name), "rb").read().split(b"end_header\n", 1)
        return head, np.frombuffer(body, kr.REC68)
    head_d, rec_d = run("device", f"gauss_device_{mode}.ply")
    head_h, rec_h = run("host", f"gauss_host_{mode}.ply")
    print(mode, "vertices:", rec_d.shape[0], rec_h.shape[0])
    assert head_d == head_h and rec_d.shape[0] > 1000
    compare_records(rec_d, rec_h, f"driver, {mode}")
