"""The multi-view re-triangulation on the device (lfd_refine_multiview through HipDensifier.refine_multiview) against the CPU twin and the f64
reference of tests/refine_ref.py - all sides are given the SAME input points, the device's own two-view points - over grids and neighbour counts
that take every path of the launch (one and several workgroups per reference, a reference boundary inside a workgroup, an empty reference, ragged
slots, masks, four-channel warps, k = 1, each of the three slot-count instantiations).  The candidate counts equal the twin's bit for bit; the
accepted bit may differ only on points the reference puts in band (the host divides where the device refines a reciprocal, so X' may move by an
ulp); where both accept the coordinates agree within the project's tolerances, where neither does the point is its input bit for bit.  Two launches
give the same bits, in place equals out of place, the counters are the recount of the status bytes, the input may come from the dense kernel or
from the chained sampled call, both contexts refuse each other's entry point, and the driver with backend="device" emits the (cell, slot) sets of
the host-backend run."""
import dataclasses

import numpy as np
import pytest
import torch

import cycle_scene
import refine_ref as rr
import support_scene as sc
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LFD_ERR_STATE = 4
TAU, THR = 1.6, 0.8
XYZ_RTOL, XYZ_ATOL, ERR_ATOL = 1e-5, 1e-6, 1e-3


@pytest.fixture(scope="module")
def dens():
    d = hb.HipDensifier(DEV)
    d.upload_cameras(sc.cameras())
    yield d
    d.close()


@pytest.fixture(scope="module")
def twin():
    d = hb.HostDensifier(16)
    d.upload_cameras(sc.cameras())
    yield d
    d.close()


def to_device(ri):
    dev = lambda t: t.to(DEV) if t is not None else None
    return hb.ReferenceInputs(ref_cam=ri.ref_cam, nbr_cams=list(ri.nbr_cams), cert=[dev(c) for c in ri.cert], warp=[dev(w) for w in ri.warp],
                              image=dev(ri.image), mask_a=dev(ri.mask_a), mask_b=[dev(m) for m in ri.mask_b] if ri.mask_b is not None else None)


def refs_for(spec, H, W, channels=2):
    """spec: (reference, k, masks, dead) per reference; ``dead``: the reference's own mask blanks it - the dense kernel has no candidate there.
    Returns the ReferenceInputs on the host (made there: the same fields whatever the device) and their copies on the device."""
    host = []
    for ref, k, masks, dead in spec:
        _s, ri = sc.reference_inputs(ref, k, H, W, channels=channels, masks=masks)
        if dead:
            ri.mask_a = torch.zeros((sc.MATCH, sc.MATCH), dtype=torch.uint8)
        host.append(ri)
    return host, [to_device(ri) for ri in host]


def owned(res):
    """A collected result whose arrays are its own (collect hands out views of the buffers, which an in-place launch overwrites)."""
    return dataclasses.replace(res, xyz=res.xyz.clone(), rgb=res.rgb.clone(), err=res.err.clone(), cell=res.cell.clone(), slot=res.slot.clone(), _packed=None)


def compare(dens, twin, refs_h, refs_d, src, buffers=None):
    """The device's launch on ``src`` (collected, owning its arrays; ``buffers``: the launch's OutputBuffers, refined in place as well) against
    the twin's on the same points and against the f64 reference.  Returns (status, accepted, fallen back)."""
    batch = hb.PreparedBatch(refs_d, sc.MATCH, sc.MATCH)
    counters = torch.zeros(2, dtype=torch.int64, device=DEV)
    got, status = dens.refine_multiview(batch, src, TAU, THR, with_status=True, counters=counters)
    again, status2 = dens.refine_multiview(batch, src, TAU, THR, with_status=True)
    dens.check_launches()
    st = status.cpu().numpy()
    assert torch.equal(status, status2) and np.array_equal(rr.bits(got.xyz), rr.bits(again.xyz)) and np.array_equal(rr.bits(got.err), rr.bits(again.err))
    for name in ("rgb", "cell", "slot"):
        assert np.array_equal(rr.bits(getattr(got, name)), rr.bits(getattr(src, name)))
    assert np.array_equal(got.ref_offsets, src.ref_offsets)
    acc = (st & 0x80) != 0
    fall = ((st & 0x7f) != 0) & ~acc
    assert counters.cpu().tolist() == [int(acc.sum()), int(fall.sum())]
    if buffers is not None:
        same, st_in = dens.refine_multiview(batch, buffers, TAU, THR, with_status=True)
        with torch.cuda.stream(dens.stream):
            inplace = same.collect(indexed=True)
        assert same is buffers and torch.equal(st_in[:src.count], status)
        assert np.array_equal(rr.bits(inplace.xyz), rr.bits(got.xyz)) and np.array_equal(rr.bits(inplace.err), rr.bits(got.err))
        assert np.array_equal(rr.bits(inplace.rgb), rr.bits(src.rgb)) and torch.equal(inplace.cell, src.cell) and torch.equal(inplace.slot, src.slot)
    # the f64 reference: the cap on the band, the reference's status outside it, fallbacks bit-identical, tolerances where accepted
    ref = rr.over_references(sc.cameras(), refs_h, src, TAU, THR, sc.MATCH, sc.MATCH)
    n_has, n_band, _a, _f = rr.check_against_reference(ref, src, got.xyz, got.err, status, THR, sc.BAND_CAP, XYZ_RTOL, XYZ_ATOL, ERR_ATOL)
    # the twin on the same points
    src_h = sc.result_on_host(src)
    want, status_h = twin.refine_multiview(hb.PreparedBatch(refs_h, sc.MATCH, sc.MATCH), src_h, TAU, THR, with_status=True)
    sh = status_h.numpy()
    assert np.array_equal(st & 0x7f, sh & 0x7f)
    acc_h = (sh & 0x80) != 0
    differ = acc != acc_h
    assert not (differ & ~ref["band"]).any()
    both, neither = acc & acc_h, ~acc & ~acc_h
    gx, ge, wx, we = got.xyz.cpu().numpy(), got.err.cpu().numpy(), want.xyz.numpy(), want.err.numpy()
    np.testing.assert_allclose(gx[both], wx[both], rtol=XYZ_RTOL, atol=XYZ_ATOL)
    np.testing.assert_allclose(ge[both], we[both], rtol=0, atol=ERR_ATOL)
    assert np.array_equal(rr.bits(gx)[neither], rr.bits(src.xyz)[neither]) and np.array_equal(rr.bits(ge)[neither], rr.bits(src.err)[neither])
    same_bits = float((rr.bits(gx)[both] == rr.bits(wx)[both]).all(axis=1).mean()) if both.any() else 1.0
    print(f"{src.count} points, {n_has} with a candidate, {int(acc.sum())} refined, {int(fall.sum())} fallen back, {n_band} in band, accepted bit "
          f"differs from the twin's on {int(differ.sum())}, coordinates bit-identical to the twin's on {100.0 * same_bits:.2f} % of the refined")
    return st, int(acc.sum()), int(fall.sum())


CASES = {
    "64x48_k3": (48, 64, 2, [(10, 3, False, False)]),
    "37x29_k8_c4": (29, 37, 4, [(10, 8, False, False)]),
    "k1": (48, 64, 2, [(10, 1, False, False)]),
    "k12": (29, 37, 2, [(10, 12, False, False)]),
    "ragged_3_refs": (48, 64, 2, [(10, 3, False, False), (20, 1, False, False), (30, 2, False, False)]),
    "masks": (48, 64, 2, [(10, 3, True, False), (11, 3, True, False)]),
    "empty_reference": (48, 64, 2, [(10, 3, False, False), (20, 3, False, True), (30, 3, False, False)]),
    "128x128_two_refs": (128, 128, 2, [(10, 3, False, False), (25, 4, False, False)]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_against_the_twin_and_the_reference(dens, twin, name):
    H, W, channels, spec = CASES[name]
    refs_h, refs_d = refs_for(spec, H, W, channels)
    batch = hb.PreparedBatch(refs_d, sc.MATCH, sc.MATCH)
    out = hb.OutputBuffers(len(spec) * H * W, len(spec), batch.k, DEV)
    dens.launch_dense(batch, sc.params(reproj_thresh=THR), out)
    dens.check_launches()
    with torch.cuda.stream(dens.stream):
        src = owned(out.collect())
    off = np.asarray(src.ref_offsets)
    st, n_acc, n_fall = compare(dens, twin, refs_h, refs_d, src, buffers=out)
    if name == "k1":
        assert src.count > 1000 and n_acc == 0 and n_fall == 0 and int(st.max()) == 0
    else:
        assert n_acc > 100 and n_fall > 20                                 # it refines some points and falls back on some
    if name == "ragged_3_refs":
        assert int(st[off[1]:off[2]].max()) == 0 and int((st[off[2]:] & 0x7f).max()) == 1
    if name == "empty_reference":
        assert off[1] == off[2] and off[1] > 0 and off[3] > off[2]
    if name == "128x128_two_refs":
        assert off[1] > 256 * 4 and off[1] % 256 != 0 and src.count - off[1] > 256 * 4      # several workgroups each, the boundary inside one


def test_input_from_the_chained_sampled_call(dens, twin):
    """The buffers lfd_triangulate_sampled_chain wrote are refined as they are, in place (asynchronously, nothing read back in between)."""
    refs_h, refs_d = refs_for([(10, 3, False, False), (20, 3, False, False), (30, 2, False, False)], 96, 96)
    batch = hb.PreparedBatch(refs_d, sc.MATCH, sc.MATCH)
    M = 1500
    out = hb.OutputBuffers(3 * (M + 24 * 24 + 64), 3, batch.k, DEV)
    dens.seed_rng(5)
    dens.launch_sampled_chain(batch, sc.params(matches_per_ref=M, reproj_thresh=THR), M, out)
    with torch.cuda.stream(dens.stream):
        src = owned(out.collect(indexed=True, check_selection=True))
    assert src.count > 2000
    _st, n_acc, n_fall = compare(dens, twin, refs_h, refs_d, src, buffers=out)
    assert n_acc > 1000 and n_fall > 20


def test_each_context_refuses_the_other_s_entry_point(dens, twin):
    lib = hb.load_library()
    assert lib.lfd_refine_multiview_host(dens._ctx, None, None, None, 1.0, 1.0, None, None, None, None) == LFD_ERR_STATE
    assert lib.lfd_refine_multiview(twin._ctx, None, None, None, 1.0, 1.0, None, None, None, None) == LFD_ERR_STATE
    _refs_h, refs_d = refs_for([(10, 3, False, False)], 29, 37)
    batch = hb.PreparedBatch(refs_d, sc.MATCH, sc.MATCH)
    src = dens.triangulate_dense(batch, sc.params())
    with pytest.raises(ValueError, match="lives on|live on"):
        dens.refine_multiview(batch, sc.result_on_host(src), TAU, THR)
    with pytest.raises(ValueError, match="counters"):
        dens.refine_multiview(batch, src, TAU, THR, counters=torch.zeros(2, dtype=torch.int64))


@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_the_driver_on_the_device_emits_the_host_run_s_cells(tmp_path_factory, mode):
    """The tie-free, noise-free slab scene of tests/cycle_scene.py (for the reason tests/test_gpu_cycle_gate.py gives: only decisions far from
    every threshold are the same on both backends by construction), with the support filter in front: the re-triangulation moves points and never
    changes which (cell, slot) a run emits."""
    scene = cycle_scene.make_scene(str(tmp_path_factory.mktemp("refine_gpu")))
    kw = dict(occlusion_steps=True, out_of_range=0.3, noise_px=0.0, outlier_frac=0.05, cert_mode="tiefree")
    exp = {"min_support_views": 2, "multiview_refine": True}
    with cycle_scene.recorded_cells() as host_cells:
        host = cycle_scene.run(scene, cycle_scene.matcher_for(scene, **kw), "host.ply", triangulation_mode=mode, experimental=exp)
    with cycle_scene.recorded_cells() as dev_cells:
        dev = cycle_scene.run(scene, cycle_scene.matcher_for(scene, **kw), "dev.ply", backend="device", device=DEV, triangulation_mode=mode,
                              experimental=exp)
    with cycle_scene.recorded_cells() as off_cells:
        off = cycle_scene.run(scene, cycle_scene.matcher_for(scene, **kw), "off.ply", backend="device", device=DEV, triangulation_mode=mode,
                              experimental={"min_support_views": 2})
    n = len(scene["refs"])
    # the host backend collects a reference's points and then the filter's result (they alternate); the device routes collect once, behind the
    # filter and the re-triangulation
    assert len(host_cells) == 2 * n and len(dev_cells) == n and len(off_cells) == n and host.xyz.shape[0] > 500
    assert dev_cells == host_cells[1::2] and dev_cells == off_cells
    assert dev.xyz.shape[0] == host.xyz.shape[0] == off.xyz.shape[0] and np.array_equal(dev.points_per_reference, host.points_per_reference)
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    assert np.array_equal(bits(dev.rgb), bits(off.rgb))
    moved = (bits(dev.xyz) != bits(off.xyz)).any(axis=1)
    print(f"{mode}: {dev.xyz.shape[0]} points, {int(moved.sum())} moved by the re-triangulation on the device")
    assert moved.mean() > 0.5
