"""The photo-consistency gate on the device (lfd_photo_gate through HipDensifier.photo_gate) against the CPU twin and the
brute-force reference of tests/photo_ref.py - all sides are given the SAME input points, the device's own dense points - on the shapes of
tests/test_photo_host.py at MATCH = 128: status, kept points, offsets, per-slot counts and every copied array are equal, ncc agrees within one
f32 ulp, the counters are added to, a second launch gives the same bits.  The kernel has ONE launch shape (a lane per point, 256 per
workgroup, no grid-stride path): point counts one below, at and one above a multiple of the workgroup size, a capacity with a whole workgroup
beyond the last offset whose tail stays untouched, an empty reference, a sampled-mode result, both contexts refusing each other's entry
point, and the driver on cuda:0 - with device_image_prep on and off - writing the host backend's file byte for byte."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import colour_scene as cs
import photo_ref
import photo_scene as ps
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LFD_ERR_STATE = 4
MATCH = ps.MATCH
BASE = [1, 10, 100, 1000, 10000]


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


def on_device(res):
    mv = lambda t: t.to(DEV)
    return dataclasses.replace(res, xyz=mv(res.xyz), rgb=mv(res.rgb), err=mv(res.err), cell=mv(res.cell), slot=mv(res.slot), _packed=None, normals=None)


def compare(dens, twin, refs_h, src_h, R, min_ncc=0.8, min_texture=2.0, reference=True):
    """Device against twin (and reference) over the host-side points ``src_h``; returns the device's status."""
    batch_d = hb.PreparedBatch([ps.to_device(ri, DEV) for ri in refs_h], MATCH, MATCH)
    batch_h = hb.PreparedBatch(refs_h, MATCH, MATCH)
    src_d = on_device(src_h)
    counters = torch.tensor(BASE, dtype=torch.int64, device=DEV)
    got, status, ncc = dens.photo_gate(batch_d, src_d, R, min_ncc, min_texture, with_status=True, with_ncc=True, counters=counters)
    again, status2, ncc2 = dens.photo_gate(batch_d, src_d, R, min_ncc, min_texture, with_status=True, with_ncc=True)
    dens.check_launches()
    want, status_t, ncc_t = twin.photo_gate(batch_h, src_h, R, min_ncc, min_texture, with_status=True, with_ncc=True)
    st = status.cpu().numpy()
    assert np.array_equal(st, status_t.numpy())
    assert torch.equal(status, status2) and np.array_equal(ps.bits(ncc), ps.bits(ncc2))
    assert ps.ulp_apart(ncc.cpu().numpy(), ncc_t.numpy()) <= 1
    assert (counters.cpu() - torch.tensor(BASE)).tolist() == np.bincount(st, minlength=5).tolist()             # added to, not overwritten
    assert got.count == want.count == again.count
    assert np.array_equal(got.ref_offsets, want.ref_offsets) and np.array_equal(got.seg_counts, want.seg_counts)
    for name in ("xyz", "rgb", "err", "cell", "slot"):
        assert np.array_equal(ps.bits(getattr(got, name)), ps.bits(getattr(want, name))), name
        assert np.array_equal(ps.bits(getattr(got, name)), ps.bits(getattr(again, name))), name
    if reference:
        ref_status, kept, ref_ncc = photo_ref.batch_reference(refs_h, MATCH, MATCH, src_h, R, min_ncc, min_texture)
        assert np.array_equal(st, ref_status) and ps.ulp_apart(ncc.cpu().numpy(), ref_ncc) <= 1
        cols, offs, seg = photo_ref.filtered(src_h, kept)
        assert np.array_equal(got.ref_offsets, offs) and np.array_equal(got.seg_counts, seg)
        for name, col in zip(("xyz", "rgb", "err", "cell", "slot"), cols):
            assert np.array_equal(ps.bits(getattr(got, name)), ps.bits(col)), name
    return st


@pytest.mark.parametrize("H,W,k,channels,masks,R", ps.SHAPES)
def test_device_equals_twin_and_reference(dens, twin, H, W, k, channels, masks, R):
    scenes = ps.case(H, W, k, channels, masks)
    refs_h = [s.inputs for s in scenes]
    src = dens.triangulate_dense(hb.PreparedBatch([ps.to_device(ri, DEV) for ri in refs_h], MATCH, MATCH), ps.params())
    assert src.count > 0.8 * 2 * H * W
    st = compare(dens, twin, refs_h, ps.result_on_host(src), R)
    if (H, W) == (20, 24) and not masks:
        assert {2, 3, 4} <= set(st.tolist())


@pytest.mark.parametrize("n", [255, 256, 257, 511, 512, 513])
def test_point_counts_around_a_multiple_of_the_workgroup(dens, twin, n):
    """One below, at and one above 256 and 512 points; the points straddle the two references inside a workgroup, and guarded points (a cell
    outside the grid, a slot the reference does not have) sit first and last."""
    scenes = ps.case(20, 24, 3, 2, False)
    refs_h = [s.inputs for s in scenes]
    full = twin.triangulate_dense(hb.PreparedBatch(refs_h, MATCH, MATCH), ps.params())
    n0 = int(full.ref_offsets[1])
    a = n // 3                                                                 # a points of reference 0, the rest of reference 1
    pick = np.concatenate([np.arange(n0 - a, n0), np.arange(n0, n0 + n - a)])
    assert n0 + n - a <= full.count
    take = lambda t: t[torch.from_numpy(pick)].clone()
    cell, slot = take(full.cell), take(full.slot)
    cell[0], slot[1], cell[n - 1], slot[n - 2] = -1, 3, 20 * 24, 255
    seg = np.zeros_like(full.seg_counts)
    src = dataclasses.replace(full, xyz=take(full.xyz), rgb=take(full.rgb), err=take(full.err), cell=cell, slot=slot,
                              ref_offsets=np.array([0, a, n], np.int64), seg_counts=seg, _packed=None, normals=None)
    st = compare(dens, twin, refs_h, src, 2)
    assert st.size == n and (st[[0, 1, n - 1, n - 2]] == 0).all()


@pytest.mark.parametrize("which", [0, 1])
def test_one_reference_empty(dens, twin, which):
    scenes = ps.case(20, 24, 3, 2, False)
    refs_h = [s.inputs for s in scenes]
    full = twin.triangulate_dense(hb.PreparedBatch(refs_h, MATCH, MATCH), ps.params())
    compare(dens, twin, refs_h, ps.one_reference_empty(full, which), 3)


def test_a_whole_workgroup_beyond_the_last_offset_stays_untouched(dens):
    scenes = ps.case(20, 24, 3, 2, False)
    batch_d = hb.PreparedBatch([ps.to_device(s.inputs, DEV) for s in scenes], MATCH, MATCH)
    cap = 2 * 20 * 24 + 300
    src, dst = hb.OutputBuffers(cap, 2, 3, DEV), hb.OutputBuffers(cap, 2, 3, DEV)
    with torch.cuda.stream(dens.stream):
        src._f.fill_(0.25)
        dst._f.fill_(0.5)
        dst.cell.fill_(-7)
        dst.slot.fill_(77)
    dens.launch_dense(batch_d, ps.params(), src)
    dens.check_launches()
    n = src.collect().count
    assert n < cap - 256
    before = [t.clone() for t in (src._f, src.cell, src.slot)]
    st = torch.full((cap,), 9, dtype=torch.uint8, device=DEV)
    ncc = torch.full((cap,), 7.0, device=DEV)
    torch.cuda.synchronize()
    rc = dens._lib.lfd_photo_gate(dens._ctx, C.byref(batch_d.c), C.byref(src.c), src.ref_offsets.data_ptr(), C.cast(batch_d.nbr_images, C.c_void_p),
                                  2, C.c_float(0.8), C.c_float(2.0), C.byref(dst.c), dst.ref_offsets.data_ptr(), dst.seg_counts.data_ptr(),
                                  st.data_ptr(), ncc.data_ptr(), None)
    dens.check_launches()
    assert rc == 0
    kept = int(dst.ref_offsets.cpu()[-1])
    assert 0 < kept < n and (st[:n] <= 4).all() and int((st[:n] != 4).sum()) == kept
    assert (st[n:] == 9).all() and (ncc[n:] == 7.0).all()                      # per input point: nothing beyond the last offset
    assert (dst.xyz[kept:] == 0.5).all() and (dst.rgb[kept:] == 0.5).all() and (dst.err[kept:cap] == 0.5).all()       # the output beyond the kept points
    assert (dst.cell[kept:] == -7).all() and (dst.slot[kept:] == 77).all()
    for t, b in zip((src._f, src.cell, src.slot), before):
        assert np.array_equal(ps.bits(t), ps.bits(b))                          # `in` is untouched


def test_a_sampled_result_goes_through_the_same_call(dens, twin):
    sc = ps.make(5, 3, 20, 24, match=MATCH, slide_rows=(8, 13), slide_px=3.0)
    batch_d = hb.PreparedBatch([ps.to_device(sc.inputs, DEV)], MATCH, MATCH)
    dens.seed_rng(11)
    src = dens.triangulate_sampled(batch_d, ps.params(), 200)
    assert 50 < src.count <= 200 + 24 * 24
    st = compare(dens, twin, [sc.inputs], ps.result_on_host(src), 2)
    assert (st == 4).any() and (st == 3).any()


def test_each_context_refuses_the_other_s_entry_point(dens, twin):
    scenes = ps.case(6, 8, 3, 4, True)
    refs_h = [s.inputs for s in scenes]
    batch_d = hb.PreparedBatch([ps.to_device(ri, DEV) for ri in refs_h], MATCH, MATCH)
    batch_h = hb.PreparedBatch(refs_h, MATCH, MATCH)
    src = dens.triangulate_dense(batch_d, ps.params())
    rc, *_ = hb._photo_gate_call(dens._lib.lfd_photo_gate_host, dens._ctx, batch_d, src, 2, 0.8, 2.0, False, False, None, None, DEV)
    assert rc == LFD_ERR_STATE
    rc, *_ = hb._photo_gate_call(twin._lib.lfd_photo_gate, twin._ctx, batch_h, ps.result_on_host(src), 2, 0.8, 2.0, False, False, None, None,
                                 torch.device("cpu"))
    assert rc == LFD_ERR_STATE


def test_the_driver_on_the_device_gives_the_host_backend_s_file(tmp_path_factory, monkeypatch):
    """Dense mode through run_dense_pipeline on cuda:0, with device_image_prep on and off: the cloud - and the file written from it - is the
    host backend's byte for byte, the gate drops points, and under device_image_prep no match-size image is uploaded: the neighbours' images
    are the ones already resident."""
    import cycle_scene
    from lichtfeld_densification_plugin_amd import densify, synthetic
    from lichtfeld_densification_plugin_amd.core import hotpath
    scene = cycle_scene.make_scene(str(tmp_path_factory.mktemp("photo_gpu")), n_cams=4)
    kw = dict(noise_px=0.3, outlier_frac=0.0, cert_mode="tiefree")
    exp = {"min_photo_ncc": 0.3, "photo_window_cells": 1}
    uploads = []
    real_upload = hotpath._upload_u8

    def count_upload(a, dev):
        if getattr(a, "ndim", 0) == 3:
            uploads.append(tuple(a.shape))
        return real_upload(a, dev)

    monkeypatch.setattr(hotpath, "_upload_u8", count_upload)
    dev_run = lambda name, **cfg: cycle_scene.run(scene, cycle_scene.matcher_for(scene, device=DEV, **kw), name, backend="device", device=DEV,
                                                  triangulation_mode="dense", **cfg)
    host = cycle_scene.run(scene, cycle_scene.matcher_for(scene, **kw), "host.ply", triangulation_mode="dense", experimental=exp)
    host_off = cycle_scene.run(scene, cycle_scene.matcher_for(scene, **kw), "host_off.ply", triangulation_mode="dense")
    uploads.clear()
    prep = dev_run("prep.ply", device_image_prep=True, experimental=exp)
    size = tuple(synthetic.ROMA_PRESETS["turbo"][:2])
    assert not [u for u in uploads if u[:2] == size]                          # no match-size image crosses: the neighbours' are resident
    uploads.clear()
    plain = dev_run("plain.ply", experimental=exp)
    assert len([u for u in uploads if u[:2] == size]) == 4 * len(scene["refs"])       # (without the preparation on the device they do: 1 + 3 per reference)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)

    def same_file_columns(a, b):
        return (a.xyz.shape == b.xyz.shape and np.array_equal(bits(a.xyz), bits(b.xyz)) and np.array_equal(bits(a.rgb), bits(b.rgb))
                and np.array_equal(a.points_per_reference, b.points_per_reference))

    assert same_file_columns(prep, host) and same_file_columns(plain, host)
    assert 500 < host.xyz.shape[0] < host_off.xyz.shape[0]                     # the gate drops points
    out = tmp_path_factory.mktemp("photo_out")
    files = {}
    for name, res in (("prep", prep), ("plain", plain)):
        files[name] = str(out / f"{name}.ply")
        assert densify._finish_on_device(res, files[name], 0, 0) == res.xyz.shape[0]
    densify._write_output(str(out / "host.ply"), host.xyz, host.rgb, host.err, None)
    want = open(str(out / "host.ply"), "rb").read()
    assert open(files["prep"], "rb").read() == want and open(files["plain"], "rb").read() == want


def test_the_stages_in_front_report_their_own_totals(tmp_path_factory, caplog):
    """Sampled mode on cuda:0 - the fused route, where one read-back of a result's integers feeds every stage's totals - behind the support
    filter and the depth-uncertainty gate: what those two log is what they log with the photo-consistency gate off, and the gate's five counts
    add up to what the depth gate kept."""
    import logging
    import cycle_scene
    scene = cycle_scene.make_scene(str(tmp_path_factory.mktemp("photo_totals")), n_cams=4)
    around = {"min_support_views": 1, "max_depth_sigma_rel": 0.02, "match_sigma_px": 0.5}
    lines = {}
    for name, exp in (("off", around), ("on", {**around, "min_photo_ncc": 0.3, "photo_window_cells": 1})):
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="lfd_densify"):
            res = cycle_scene.run(scene, cycle_scene.matcher_for(scene, device=DEV), f"{name}.ply", backend="device", device=DEV, experimental=exp)
        lines[name] = ([r.getMessage() for r in caplog.records if r.getMessage().startswith(("Multi-view support filter", "Depth-uncertainty gate"))],
                       [r.getMessage() for r in caplog.records if r.getMessage().startswith("Photo-consistency gate")], res.xyz.shape[0])
    assert len(lines["off"][0]) == 2 and lines["on"][0] == lines["off"][0] and not lines["off"][1] and len(lines["on"][1]) == 1
    kept_by_sigma = int(lines["on"][0][1].split(" points in, ")[1].split(" kept")[0])
    counts = [int(w) for w in lines["on"][1][0].split("grey levels: ")[1].replace(",", " ").split() if w.isdigit()]
    assert len(counts) == 5 and sum(counts) == kept_by_sigma == lines["off"][2]
    assert lines["on"][2] == kept_by_sigma - counts[4] and 0 < counts[4] < kept_by_sigma
