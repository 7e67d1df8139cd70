"""The multi-view colour on the device (lfd_colour_multiview through HipDensifier.colour_multiview) against the CPU twin and
the NumPy reference of tests/colour_ref.py - all sides are given the SAME input points, the device's own dense points.  Shapes: two references
of 20 x 24 cells (480 points each: the second workgroup straddles the two references) and of 6 x 8 cells, k = 3 and k = 16 (the kernel's
smallest and largest instantiation; k = 8 the middle one), 2- and 4-channel warps, masks on and off, both modes.  The colours equal the twin's
bit for bit, the statuses are equal, the counters are the recount, a second launch gives the same bits, in place equals out of place, a
sampled-mode result goes through the same call, both contexts refuse each other's entry point, and through the driver - with device_image_prep
on and off - the cloud is the host backend's and under device_image_prep no match-size image crosses to the device."""
import ctypes as C
import numpy as np
import pytest
import torch

import colour_ref
import colour_scene as cs
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LFD_ERR_STATE = 4
REFS = (5, 21)
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


def scenes_for(k, H, W, channels, masks):
    key = (k, H, W, channels, masks)
    if key not in _made:
        _made[key] = [cs.make(r, k, H, W, match=MATCH, channels=channels, masks=masks, noise_px=0.6,
                              gains=[1.0 + 0.03 * ((j * 7) % 5 - 2) for j in range(k + 1)]) for r in REFS]
    return _made[key]


@pytest.mark.parametrize("mode", ["mean", "median"])
@pytest.mark.parametrize("k,H,W,channels,masks", [(3, 20, 24, 2, False), (3, 20, 24, 4, True), (3, 6, 8, 2, True), (8, 20, 24, 2, True),
                                                  (16, 20, 24, 2, True), (16, 6, 8, 4, False)])
def test_device_equals_twin_and_reference(dens, twin, k, H, W, channels, masks, mode):
    scenes = scenes_for(k, H, W, channels, masks)
    refs_h = [s.inputs for s in scenes]
    batch_d = hb.PreparedBatch([cs.to_device(ri, DEV) for ri in refs_h], MATCH, MATCH)
    src = dens.triangulate_dense(batch_d, cs.params())
    assert src.count > 0.8 * 2 * H * W
    counters = torch.zeros(2, dtype=torch.int64, device=DEV)
    got, status = dens.colour_multiview(batch_d, src, TAU, mode, with_status=True, counters=counters)
    again, status2 = dens.colour_multiview(batch_d, src, TAU, mode, with_status=True)
    dens.check_launches()
    assert torch.equal(status, status2) and np.array_equal(cs.bits(got.rgb), cs.bits(again.rgb))
    for name in ("xyz", "err", "cell", "slot"):
        assert np.array_equal(cs.bits(getattr(got, name)), cs.bits(getattr(src, name)))
    st = status.cpu().numpy()
    assert counters.cpu().tolist() == [int((st > 0).sum()), int(st.astype(np.int64).sum())]
    src_h = cs.result_on_host(src)
    want, status_t = twin.colour_multiview(hb.PreparedBatch(refs_h, MATCH, MATCH), src_h, TAU, mode, with_status=True)
    assert np.array_equal(st, status_t.numpy())
    assert np.array_equal(cs.bits(got.rgb), cs.bits(want.rgb))
    ref, ref_status = colour_ref.batch_reference(cs.cameras(), refs_h, [s.images for s in scenes], MATCH, MATCH, src_h, TAU, mode)
    assert np.array_equal(st, ref_status) and np.array_equal(cs.bits(got.rgb), cs.bits(ref))
    assert not np.array_equal(cs.bits(got.rgb), cs.bits(src.rgb))             # (the stage does something here)


@pytest.mark.parametrize("mode", ["mean", "median"])
def test_in_place_equals_out_of_place_and_the_tail_stays(dens, mode):
    scenes = scenes_for(3, 20, 24, 2, False)
    batch_d = hb.PreparedBatch([cs.to_device(s.inputs, DEV) for s in scenes], MATCH, MATCH)
    cap = 2 * 20 * 24 + 300                                                   # (a whole workgroup beyond the last offset)
    src = hb.OutputBuffers(cap, 2, 3, DEV)
    with torch.cuda.stream(dens.stream):
        src._f.fill_(0.25)
    dens.launch_dense(batch_d, cs.params(), src)
    dens.check_launches()
    res = src.collect()
    n = res.count
    assert n < cap - 256
    apart, status = dens.colour_multiview(batch_d, res, TAU, mode, with_status=True)
    xyz = src.xyz.clone()
    same = dens.colour_multiview(batch_d, src, TAU, mode)
    dens.check_launches()
    assert same is src
    assert np.array_equal(cs.bits(src.rgb[:n]), cs.bits(apart.rgb)) and np.array_equal(cs.bits(src.xyz), cs.bits(xyz))
    assert (src.rgb[n:cap] == 0.25).all()
    # the status beyond the last offset, through the C entry point
    st = torch.full((cap,), 9, dtype=torch.uint8, device=DEV)
    out = torch.full((cap, 3), 7.0, device=DEV)
    torch.cuda.synchronize()
    rc = dens._lib.lfd_colour_multiview(dens._ctx, C.byref(batch_d.c), C.byref(src.c), src.ref_offsets.data_ptr(),
                                        C.cast(batch_d.nbr_images, C.c_void_p), C.c_float(TAU), hb.COLOUR_MODES[mode], out.data_ptr(), st.data_ptr(), None)
    dens.check_launches()
    assert rc == 0 and (st[n:] == 9).all() and (out[n:] == 7.0).all() and (st[:n] > 0).all()


def test_a_sampled_result_goes_through_the_same_call(dens, twin):
    scenes = [cs.make(5, 3, 20, 24, match=MATCH, noise_px=0.6)]
    ri = scenes[0].inputs
    batch_d = hb.PreparedBatch([cs.to_device(ri, DEV)], MATCH, MATCH)
    dens.seed_rng(11)
    src = dens.triangulate_sampled(batch_d, cs.params(), 200)
    assert 50 < src.count <= 200 + 24 * 24
    for mode in ("mean", "median"):
        got, status = dens.colour_multiview(batch_d, src, TAU, mode, with_status=True)
        dens.check_launches()
        want, status_t = twin.colour_multiview(hb.PreparedBatch([ri], MATCH, MATCH), cs.result_on_host(src), TAU, mode, with_status=True)
        assert np.array_equal(status.cpu().numpy(), status_t.numpy()) and np.array_equal(cs.bits(got.rgb), cs.bits(want.rgb))


def test_each_context_refuses_the_other_s_entry_point(dens, twin):
    scenes = scenes_for(3, 6, 8, 2, True)
    refs_h = [s.inputs for s in scenes]
    batch_d = hb.PreparedBatch([cs.to_device(ri, DEV) for ri in refs_h], MATCH, MATCH)
    batch_h = hb.PreparedBatch(refs_h, MATCH, MATCH)
    src = dens.triangulate_dense(batch_d, cs.params())
    rc, _r, _s = hb._colour_call(dens._lib.lfd_colour_multiview_host, dens._ctx, batch_d, src, TAU, "mean", False, None, DEV)
    assert rc == LFD_ERR_STATE
    rc, _r, _s = hb._colour_call(twin._lib.lfd_colour_multiview, twin._ctx, batch_h, cs.result_on_host(src), TAU, "mean", False, None, torch.device("cpu"))
    assert rc == LFD_ERR_STATE


def prep_match_size(scene):
    """(h_match, w_match) of the runs below: the analytic matcher's "turbo" preset; the scene's photographs are smaller (208 x 320)"""
    from lichtfeld_densification_plugin_amd import synthetic
    h, w = synthetic.ROMA_PRESETS["turbo"][:2]
    assert (h, w) != (scene["cams"][0].height, scene["cams"][0].width)
    return h, w


def test_the_driver_on_the_device_gives_the_host_backend_s_file(tmp_path_factory, monkeypatch):
    """Dense mode through run_dense_pipeline on cuda:0, with device_image_prep on and off: the cloud - and the file written from it - is the
    host backend's byte for byte, the knob changes colours only, and under device_image_prep every camera is prepared once and no match-size
    image is uploaded: the neighbours' images are the ones already resident."""
    import cycle_scene
    from lichtfeld_densification_plugin_amd import densify
    from lichtfeld_densification_plugin_amd.core import hotpath
    scene = cycle_scene.make_scene(str(tmp_path_factory.mktemp("colour_gpu")), n_cams=4)
    kw = dict(noise_px=0.3, outlier_frac=0.0, cert_mode="tiefree")
    exp = {"multiview_colour": "median"}
    uploads, prepared = [], []
    real_upload, real_prepare = hotpath._upload_u8, hb.HipDensifier.prepare_image

    def count_upload(a, dev):
        if getattr(a, "ndim", 0) == 3:
            uploads.append(tuple(a.shape))
        return real_upload(a, dev)

    def count_prepare(self, *a, **k):
        prepared.append(1)
        return real_prepare(self, *a, **k)

    monkeypatch.setattr(hotpath, "_upload_u8", count_upload)
    monkeypatch.setattr(hb.HipDensifier, "prepare_image", count_prepare)
    dev_run = lambda name, **cfg: cycle_scene.run(scene, cycle_scene.matcher_for(scene, device=DEV, **kw), name, backend="device", device=DEV,
                                                  triangulation_mode="dense", **cfg)
    host = cycle_scene.run(scene, cycle_scene.matcher_for(scene, **kw), "host.ply", triangulation_mode="dense", experimental=exp)
    host_off = cycle_scene.run(scene, cycle_scene.matcher_for(scene, **kw), "host_off.ply", triangulation_mode="dense")
    uploads.clear(), prepared.clear()
    prep_off = dev_run("prep_off.ply", device_image_prep=True)
    n_prep_off = len(prepared)
    uploads.clear(), prepared.clear()
    prep = dev_run("prep.ply", device_image_prep=True, experimental=exp)
    used = {int(r) for r in scene["refs"]} | {int(n) for r in scene["refs"] for n in list(scene["nn"][r])[:3]}
    assert len(prepared) == n_prep_off == len(used)                           # once per camera, knob on or off
    size = tuple(prep_match_size(scene))
    assert not [u for u in uploads if u[:2] == size]                          # no match-size image crosses: the neighbours' are resident
    uploads.clear()
    plain = dev_run("plain.ply", experimental=exp)
    assert len([u for u in uploads if u[:2] == size]) == 4 * len(scene["refs"])       # (without the preparation on the device they do: 1 + 3 per reference)
    assert host.xyz.shape[0] > 500
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)

    def same_file_columns(a, b):
        """positions, colours, counts and order - what the file holds.  (The reprojection error, which a PLY does not carry, differs in the
        last bit between the dense kernel and its twin on this scene with the knob off as well: 47 805 of 307 199 values, by 6e-8.)"""
        return (a.xyz.shape == b.xyz.shape and np.array_equal(bits(a.xyz), bits(b.xyz)) and np.array_equal(bits(a.rgb), bits(b.rgb))
                and np.array_equal(a.points_per_reference, b.points_per_reference))

    assert same_file_columns(prep, host) and same_file_columns(plain, host)
    assert same_file_columns(prep_off, host_off)
    assert np.array_equal(bits(host.xyz), bits(host_off.xyz)) and not np.array_equal(bits(host.rgb), bits(host_off.rgb))
    out = tmp_path_factory.mktemp("colour_out")
    files = {}
    for name, res in (("prep", prep), ("plain", plain)):
        files[name] = str(out / f"{name}.ply")
        assert densify._finish_on_device(res, files[name], 0, 0) == res.xyz.shape[0]
    densify._write_output(str(out / "host.ply"), host.xyz, host.rgb, host.err, None)
    want = open(str(out / "host.ply"), "rb").read()
    assert open(files["prep"], "rb").read() == want and open(files["plain"], "rb").read() == want
