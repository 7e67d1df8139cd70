"""The per-image exposure gains on the device (lfd_gain_accumulate / lfd_gain_apply through HipDensifier) against the CPU twin
and the brute-force NumPy reference of tests/gain_ref.py - all sides are given the SAME input points, the device's own dense points.  Shapes:
two references of 20 x 24 cells (480 points each: the second workgroup straddles the two references), one of 6 x 8 (less than a wave), one of
40 x 48 (eight workgroups add to the same rows), a reference with no surviving point between two others, k = 3, 8 and 16 (the kernel's three
slot counts), 2- and 4-channel warps (its two strides), masks on and off.  The uint64 tables are equal element for element, a second launch
adds the same again, a sampled-mode result goes through the same call, the apply's bits are the twin's, both contexts refuse each other's
entry points, and through the driver - device_image_prep on and off - the PLY and the gains.json are the host backend's byte for byte."""
import dataclasses
import os

import numpy as np
import pytest
import torch

import colour_scene as cs
import gain_ref
from lichtfeld_densification_plugin_amd.core import gains
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LFD_ERR_STATE = 4
TAU = 1.6
MATCH = 96


@pytest.fixture(scope="module")
def dens():
    d = hb.HipDensifier(DEV)
    d.upload_cameras(cs.cameras())
    yield d
    d.close()


@pytest.fixture(scope="module")
def twin():
    d = hb.HostDensifier(16)
    d.upload_cameras(cs.cameras())
    yield d
    d.close()


_made = {}


def scenes_for(refs, k, H, W, channels, masks):
    """Gains between 0.8 and 1.35: part of the 1.35 view passes 0.95 (and clips), so samples of both kinds occur."""
    key = (refs, k, H, W, channels, masks)
    if key not in _made:
        g = [1.0] + [(0.8, 1.35, 1.0, 1.2)[j % 4] for j in range(k)]
        _made[key] = [cs.make(r, k, H, W, match=MATCH, channels=channels, masks=masks, noise_px=0.6, gains=g) for r in refs]
    return _made[key]


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def blank(ri):
    """The same reference with no observation anywhere (warps of NaN): no cell survives the triangulation."""
    return dataclasses.replace(ri, warp=[torch.full_like(w, float("nan")) for w in ri.warp])


@pytest.mark.parametrize("refs,k,H,W,channels,masks,empty", [
    ((5, 21), 3, 20, 24, 2, False, None), ((5, 21), 3, 20, 24, 4, True, None), ((5,), 3, 6, 8, 2, True, None), ((5,), 3, 40, 48, 2, False, None),
    ((5, 13, 21), 3, 20, 24, 2, True, 1), ((5, 21), 8, 20, 24, 4, True, None), ((5, 21), 16, 20, 24, 2, True, None), ((5,), 16, 6, 8, 4, False, None)])
def test_device_equals_twin_and_reference(dens, twin, refs, k, H, W, channels, masks, empty):
    scenes = scenes_for(refs, k, H, W, channels, masks)
    refs_h = [blank(s.inputs) if i == empty else s.inputs for i, s in enumerate(scenes)]
    batch_d = hb.PreparedBatch([cs.to_device(ri, DEV) for ri in refs_h], MATCH, MATCH)
    src = dens.triangulate_dense(batch_d, cs.params())
    n_live = len(refs) - (0 if empty is None else 1)
    assert src.count > 0.8 * n_live * H * W
    if empty is not None:
        assert src.ref_offsets[empty] == src.ref_offsets[empty + 1] and 0 < src.ref_offsets[empty] < src.count
    before = [cs.bits(getattr(src, n)).copy() for n in ("xyz", "rgb", "err", "cell", "slot")]
    table = dens.gain_accumulate(batch_d, src, TAU)
    dens.check_launches()
    got = u64(table).copy()
    src_h = cs.result_on_host(src)
    want_t = twin.gain_accumulate(hb.PreparedBatch(refs_h, MATCH, MATCH), src_h, TAU)
    assert got.shape == (len(refs) * k, 7) and np.array_equal(got, u64(want_t))
    want, part, counted = gain_ref.batch_reference(cs.cameras(), refs_h, [s.images for s in scenes], MATCH, MATCH, src_h, TAU, k)
    assert np.array_equal(got, want)
    assert counted.any() and (part & ~counted).any()
    if empty is not None:
        assert (got[empty * k:(empty + 1) * k] == 0).all() and (got[(empty + 1) * k:, 0] > 0).any() and (got[:empty * k, 0] > 0).any()
    for n, b in zip(("xyz", "rgb", "err", "cell", "slot"), before):             # reads only
        assert np.array_equal(cs.bits(getattr(src, n)), b)
    again = dens.gain_accumulate(batch_d, src, TAU, table=table)                # a second launch adds exactly the same again
    dens.check_launches()
    assert again is table and np.array_equal(u64(table), 2 * want)


def test_buffers_with_a_tail_and_a_collected_result_agree(dens):
    scenes = scenes_for((5, 21), 3, 20, 24, 2, False)
    batch_d = hb.PreparedBatch([cs.to_device(s.inputs, DEV) for s in scenes], MATCH, MATCH)
    cap = 2 * 20 * 24 + 300                                                   # (a whole workgroup beyond the last offset)
    src = hb.OutputBuffers(cap, 2, 3, DEV)
    with torch.cuda.stream(dens.stream):
        src._f.fill_(0.25)
    dens.launch_dense(batch_d, cs.params(), src)
    a = dens.gain_accumulate(batch_d, src, TAU)
    dens.check_launches()
    res = src.collect()
    assert res.count < cap - 256
    b = dens.gain_accumulate(batch_d, res, TAU)
    dens.check_launches()
    assert np.array_equal(u64(a), u64(b)) and int(a[:, 0].sum()) > 0


def test_a_sampled_result_goes_through_the_same_call(dens, twin):
    ri = cs.make(5, 3, 20, 24, match=MATCH, noise_px=0.6, gains=(1.0, 0.8, 1.35, 1.0)).inputs
    batch_d = hb.PreparedBatch([cs.to_device(ri, DEV)], MATCH, MATCH)
    dens.seed_rng(11)
    src = dens.triangulate_sampled(batch_d, cs.params(), 200)
    assert 50 < src.count <= 200 + 24 * 24
    got = dens.gain_accumulate(batch_d, src, TAU)
    dens.check_launches()
    want = twin.gain_accumulate(hb.PreparedBatch([ri], MATCH, MATCH), cs.result_on_host(src), TAU)
    assert np.array_equal(u64(got), u64(want)) and int(want[:, 0].sum()) > 50


def test_apply_bits_equal_the_twin(dens, twin):
    rng = np.random.default_rng(5)
    counts = np.array([300, 0, 77, 1, 5000], np.int64)                        # an empty reference; workgroups that straddle references
    n = int(counts.sum())
    rgb = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
    rgb[2, 1] = np.float32(0.9)
    rgb[7] = [np.nan, np.inf, -np.inf]
    rgb.view(np.uint32)[8, 0] = 0x7fc01234
    rgb[9, 2] = -0.25
    factors = np.array([[1.5, 1.5, 1.5], [9.0, 9.0, 9.0], [0.8, 1.0, 1.25], [0.25, 4.0, 1.0], [1.0 / 3.0, 1.1, 0.97]], np.float32)
    src = torch.from_numpy(rgb).to(DEV)
    got = dens.gain_apply(src, counts, factors)
    dens.check_launches()
    want = twin.gain_apply(torch.from_numpy(rgb), counts, factors)
    assert np.array_equal(cs.bits(got), cs.bits(want)) and np.array_equal(cs.bits(src), cs.bits(torch.from_numpy(rgb)))
    assert np.array_equal(cs.bits(want), gains.apply_rule(rgb, np.repeat(factors, counts, axis=0)).view(np.uint32))
    assert (want == 1.0).any() and cs.bits(got)[8, 0] == 0x7fc01234


def test_each_context_refuses_the_other_s_entry_points(dens, twin):
    scenes = scenes_for((5,), 3, 6, 8, 2, True)
    refs_h = [s.inputs for s in scenes]
    batch_d = hb.PreparedBatch([cs.to_device(ri, DEV) for ri in refs_h], MATCH, MATCH)
    batch_h = hb.PreparedBatch(refs_h, MATCH, MATCH)
    src = dens.triangulate_dense(batch_d, cs.params())
    rc, _t = hb._gain_accumulate_call(dens._lib.lfd_gain_accumulate_host, dens._ctx, batch_d, src, TAU, None, DEV)
    assert rc == LFD_ERR_STATE
    rc, _t = hb._gain_accumulate_call(twin._lib.lfd_gain_accumulate, twin._ctx, batch_h, cs.result_on_host(src), TAU, None, torch.device("cpu"))
    assert rc == LFD_ERR_STATE
    f = np.ones((1, 3), np.float32)
    rc, _o = hb._gain_apply_call(dens._lib.lfd_gain_apply_host, dens._ctx, src.rgb, [src.count], f, DEV)
    assert rc == LFD_ERR_STATE
    rc, _o = hb._gain_apply_call(twin._lib.lfd_gain_apply, twin._ctx, src.rgb.cpu(), [src.count], f, torch.device("cpu"))
    assert rc == LFD_ERR_STATE


class Node:
    """A camera node as the GUI hands it to dense_init_from_lfs."""

    def __init__(self, cam):
        self.has_camera, self.camera_uid = True, cam.uid
        self.camera_width, self.camera_height = cam.width, cam.height
        self.camera_focal_x, self.camera_focal_y = float(cam.K[0, 0]), float(cam.K[1, 1])
        self.camera_R, self.camera_T = cam.R, cam.t.reshape(3)
        self.image_path, self.has_mask, self.mask_path = cam.image_path, False, None


@pytest.mark.parametrize("gain_mode", ["luma", "rgb"])
def test_the_driver_on_the_device_gives_the_host_backend_s_files(tmp_path_factory, gain_mode):
    """Dense mode through dense_init_from_lfs on cuda:0, with device_image_prep on and off: the PLY and the gains.json are the host backend's
    byte for byte, and the knob changes colours only."""
    import cycle_scene
    import lichtfeld_densification_plugin_amd as lfd
    from lichtfeld_densification_plugin_amd import densify, synthetic
    scene = cycle_scene.make_scene(str(tmp_path_factory.mktemp("gain_gpu")), n_cams=4)
    out = tmp_path_factory.mktemp("gain_out")
    nodes = [Node(c) for c in scene["cams"]]
    recs = densify.extract_cameras_from_lfs(nodes)

    def run(name, backend, exp, **cfg_kw):
        on_gpu = backend == "device"
        matcher = synthetic.SyntheticMatcher(recs, setting="turbo", device=DEV if on_gpu else "cpu", channels=2, noise_px=0.3, outlier_frac=0.0,
                                             cert_mode="tiefree")
        cfg = lfd.DensePipelineConfig(output_path=str(out / name), num_refs=0.75, nns_per_ref=3, seed=3, viz_interval=0, pack_workers=1,
                                      backend=backend, triangulation_mode="dense", experimental=exp, **cfg_kw)
        rc, msg = densify.dense_init_from_lfs(nodes, cfg, matcher=matcher, **({"device": DEV} if on_gpu else {}))
        assert rc == 0, msg
        return str(out / name)

    exp = {"gain_compensation": gain_mode}
    host, host_off = run("host.ply", "host", exp), run("host_off.ply", "host", {})
    plain, prep = run("plain.ply", "device", exp), run("prep.ply", "device", exp, device_image_prep=True)
    dev_off = run("dev_off.ply", "device", {})
    want, want_json = open(host, "rb").read(), open(host + ".gains.json", "rb").read()
    assert len(want) > 500 * 15
    for path in (plain, prep):
        assert open(path, "rb").read() == want
        assert open(path + ".gains.json", "rb").read() == want_json
    assert open(dev_off, "rb").read() == open(host_off, "rb").read() and not os.path.exists(dev_off + ".gains.json")
    rec = np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)])
    on, off = (np.frombuffer(open(p, "rb").read().split(b"end_header\n", 1)[1], dtype=rec) for p in (host, host_off))
    assert on["xyz"].tobytes() == off["xyz"].tobytes() and on["rgb"].tobytes() != off["rgb"].tobytes()


@pytest.mark.parametrize("refs_per_launch,refuse_call", [(2, None), (2, 1), (1, 1)])
def test_sampled_schedules_keep_the_statistics_of_exactly_the_references_they_emit(tmp_path_factory, monkeypatch, refs_per_launch, refuse_call):
    """Sampled mode on the device goes through the asynchronous schedules, where a launch's table travels with its buffers.  Whatever the
    schedule does - also when one collection raises upstream's selection error (``refuse_call``: the index of the ``collect`` call that
    does) and the call is redone or its reference dropped - the run's rows are those of exactly the references whose points it emitted,
    each once, with ``min_support_views`` off.  Groups of two references (three collections) and one reference per launch."""
    import cycle_scene
    import lichtfeld_densification_plugin_amd as lfd
    from lichtfeld_densification_plugin_amd import densify, synthetic
    scene = cycle_scene.make_scene(str(tmp_path_factory.mktemp("gain_gpu_sampled")), n_cams=8)
    out = tmp_path_factory.mktemp("gain_sampled_out")
    nodes = [Node(c) for c in scene["cams"]]
    recs = densify.extract_cameras_from_lfs(nodes)
    seen = {}
    plain_step, plain_collect = densify._apply_gain_compensation, hb.OutputBuffers.collect
    calls = [0]

    def step(result, config, camera_records, refs_local, progress_callback=None):
        seen.update(rows=result.gain_rows, counts=np.asarray(result.points_per_reference).copy(),
                    uids=[int(camera_records[int(i)].uid) for i in refs_local])
        return plain_step(result, config, camera_records, refs_local, progress_callback)

    def collect(self, *a, **kw):
        calls[0] += 1
        res = plain_collect(self, *a, **kw)                                      # (waited for first: the refusal comes with the counts)
        if refuse_call is not None and calls[0] - 1 == refuse_call:
            raise ValueError("a must be non-empty")
        return res

    monkeypatch.setattr(densify, "_apply_gain_compensation", step)
    monkeypatch.setattr(hb.OutputBuffers, "collect", collect)
    matcher = synthetic.SyntheticMatcher(recs, setting="turbo", device=DEV, channels=2, noise_px=0.3, outlier_frac=0.0, cert_mode="tiefree")
    cfg = lfd.DensePipelineConfig(output_path=str(out / "sampled.ply"), num_refs=0.75, nns_per_ref=3, seed=3, viz_interval=0, pack_workers=1,
                                  matches_per_ref=2500, backend="device", triangulation_mode="sampled", refs_per_launch=refs_per_launch, experimental={"gain_compensation": "luma"})
    rc, msg = densify.dense_init_from_lfs(nodes, cfg, matcher=matcher, device=DEV)
    assert rc == 0, msg
    assert calls[0] >= 2 and os.path.exists(str(out / "sampled.ply.gains.json"))
    rows, counts, uids = seen["rows"], seen["counts"], seen["uids"]
    emitted = sorted(u for u, n in zip(uids, counts.tolist()) if n > 0)
    assert len(emitted) >= len(uids) - 1 and len(emitted) >= 4
    got, times = np.unique(rows.ref_uid, return_counts=True)
    assert got.tolist() == emitted, (got.tolist(), emitted)                      # the references that have points, no others
    assert (times == 3).all()                                                    # k rows each: no launch was committed twice
    assert (rows.table[:, 0] > 0).any()
