"""The precision-weighted re-triangulation on the device (lfd_refine_multiview_weighted through HipDensifier.refine_multiview(precision=True))
against the CPU twin and the f64 reference of tests/wrefine_ref.py - all sides are given the SAME input points, the device's own two-view points -
over the smallest grids and neighbour counts that take every path of the launch (one and several workgroups per reference, a reference boundary
inside a workgroup, an empty reference, ragged slots, masks, four-channel warps, k = 1, each of the three slot-count instantiations, a plane with
an invalid patch).  Candidate counts and the weights-used bit equal the twin's bit for bit; the accepted bit may differ only on points the
reference puts in band; where both accept the coordinates agree within the project's tolerances, where neither does the point is its input bit
for bit.  With all-NaN planes the output is the device's own lfd_refine_multiview's bit for bit.  Two launches give the same bits, in place
equals out of place, the three counters are the recount of the status bytes, the input may come from the dense kernel or from the chained sampled
call, and both contexts refuse each other's entry point."""
import dataclasses

import numpy as np
import pytest
import torch

import refine_ref as rr
import support_scene as sc
import wrefine_ref as wr
import wrefine_scene as ws
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LFD_ERR_STATE = 4
THR = ws.THR
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


def refs_for(spec, H, W, channels=2, patch=False):
    """spec: (reference, k, masks, dead) per reference; ``dead``: the reference's own mask blanks it.  ``patch``: slot 1 of the first reference
    gets a block of indefinite cells and a NaN.  Returns the ReferenceInputs on the host and their copies on the device."""
    host = []
    for ref, k, masks, dead in spec:
        ri = ws.reference_inputs(ref, k, H, W, channels=channels, masks=masks)
        if dead:
            ri.mask_a = torch.zeros((sc.MATCH, sc.MATCH), dtype=torch.uint8)
        host.append(ri)
    if patch:
        q = host[0].precision[1]
        q[H // 4:3 * H // 4, W // 4:3 * W // 4] = torch.tensor([1.0, 5.0, 1.0])
        q[H // 4 + 1, W // 4 + 1] = float("nan")
    return host, [ws.to_device(ri, DEV) for ri in host]


def owned(res):
    """A collected result whose arrays are its own (collect hands out views of the buffers, which an in-place launch overwrites)."""
    return dataclasses.replace(res, xyz=res.xyz.clone(), rgb=res.rgb.clone(), err=res.err.clone(), cell=res.cell.clone(), slot=res.slot.clone(), _packed=None)


def same(a, b):
    return np.array_equal(rr.bits(a.xyz), rr.bits(b.xyz)) and np.array_equal(rr.bits(a.err), rr.bits(b.err))


def compare(dens, twin, refs_h, refs_d, src, tau, buffers=None):
    """The device's weighted launch on ``src`` (collected, owning its arrays; ``buffers``: the launch's OutputBuffers, refined in place as well)
    against the twin's on the same points and against the f64 reference.  Returns (status, accepted, fallen back, solved with weights)."""
    batch = hb.PreparedBatch(refs_d, sc.MATCH, sc.MATCH)
    counters = torch.zeros(3, dtype=torch.int64, device=DEV)
    got, status = dens.refine_multiview(batch, src, tau, THR, with_status=True, counters=counters, precision=True)
    again, status2 = dens.refine_multiview(batch, src, tau, THR, with_status=True, precision=True)
    # all-NaN planes: the device's own unweighted launch, bit for bit
    nan_batch = hb.PreparedBatch([ws.filled(r, (float("nan"),) * 3) for r in refs_d], sc.MATCH, sc.MATCH)
    nan_res, nan_st = dens.refine_multiview(nan_batch, src, tau, THR, with_status=True, precision=True)
    unw, unw_st = dens.refine_multiview(batch, src, tau, THR, with_status=True)
    dens.check_launches()
    assert torch.equal(nan_st, unw_st) and same(nan_res, unw)
    st = status.cpu().numpy()
    assert torch.equal(status, status2) and same(got, again)
    for name in ("rgb", "cell", "slot"):
        assert np.array_equal(rr.bits(getattr(got, name)), rr.bits(getattr(src, name)))
    assert np.array_equal(got.ref_offsets, src.ref_offsets)
    acc = (st & 0x80) != 0
    fall = ((st & 0x3f) != 0) & ~acc
    wtd = (st & 0x40) != 0
    assert counters.cpu().tolist() == [int(acc.sum()), int(fall.sum()), int(wtd.sum())]
    assert np.array_equal(st & 0x3f, unw_st.cpu().numpy() & 0x7f)
    if buffers is not None:
        inb, st_in = dens.refine_multiview(batch, buffers, tau, THR, with_status=True, precision=True)
        with torch.cuda.stream(dens.stream):
            inplace = inb.collect(indexed=True)
        assert inb is buffers and torch.equal(st_in[:src.count], status)
        assert same(inplace, got)
        assert np.array_equal(rr.bits(inplace.rgb), rr.bits(src.rgb)) and torch.equal(inplace.cell, src.cell) and torch.equal(inplace.slot, src.slot)
    # the f64 reference: the cap on the band, the reference's status outside it, fallbacks bit-identical, tolerances where accepted
    ref = wr.over_references(sc.cameras(), refs_h, src, tau, THR, sc.MATCH, sc.MATCH)
    n_has, n_band, _a, _f, _w = wr.check_against_reference(ref, src, got.xyz, got.err, status, THR, sc.BAND_CAP, XYZ_RTOL, XYZ_ATOL, ERR_ATOL)
    # the twin on the same points
    src_h = sc.result_on_host(src)
    want, status_h = twin.refine_multiview(hb.PreparedBatch(refs_h, sc.MATCH, sc.MATCH), src_h, tau, THR, with_status=True, precision=True)
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
    print(f"{src.count} points, {n_has} with a candidate, {int(acc.sum())} refined, {int(fall.sum())} fallen back, {int(wtd.sum())} weighted, "
          f"{n_band} in band, accepted bit differs from the twin's on {int(differ.sum())}, coordinates bit-identical to the twin's on "
          f"{100.0 * same_bits:.2f} % of the refined")
    return st, int(acc.sum()), int(fall.sum()), int((wtd & acc).sum())


# (tau 3.0 at k = 8 and k = 12: with that many candidate tests per point the f64 reference alone puts 1 % of the points in band at 1.6)
CASES = {
    "64x48_k3": (48, 64, 2, 1.6, False, [(10, 3, False, False)]),
    "37x29_k8_c4": (29, 37, 4, 3.0, False, [(10, 8, False, False)]),
    "k1": (48, 64, 2, 1.6, False, [(10, 1, False, False)]),
    "k12": (29, 37, 2, 3.0, False, [(10, 12, False, False)]),
    "ragged_3_refs_empty_middle": (48, 64, 2, 1.6, False, [(10, 3, False, False), (20, 2, False, True), (30, 2, False, False)]),
    "masks": (48, 64, 2, 1.6, False, [(10, 3, True, False), (11, 3, True, False)]),
    "128x128_two_refs": (128, 128, 2, 1.6, False, [(10, 3, False, False), (25, 4, False, False)]),
    "invalid_patch": (48, 64, 2, 1.6, True, [(10, 3, False, False)]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_against_the_twin_and_the_reference(dens, twin, name):
    H, W, channels, tau, patch, spec = CASES[name]
    refs_h, refs_d = refs_for(spec, H, W, channels, patch)
    batch = hb.PreparedBatch(refs_d, sc.MATCH, sc.MATCH)
    out = hb.OutputBuffers(len(spec) * H * W, len(spec), batch.k, DEV)
    dens.launch_dense(batch, sc.params(reproj_thresh=THR), out)
    dens.check_launches()
    with torch.cuda.stream(dens.stream):
        src = owned(out.collect())
    off = np.asarray(src.ref_offsets)
    st, n_acc, n_fall, n_wacc = compare(dens, twin, refs_h, refs_d, src, tau, buffers=out)
    if name == "k1":
        assert src.count > 1000 and n_acc == 0 and n_fall == 0 and int(st.max()) == 0
    else:
        assert n_wacc > 100 and n_fall > 20                                # it refines some points with weights and falls back on some
    if name == "ragged_3_refs_empty_middle":
        assert off[1] > 0 and off[1] == off[2] and off[3] > off[2] and int((st[off[2]:] & 0x3f).max()) == 1
    if name == "128x128_two_refs":
        assert off[1] > 256 * 4 and off[1] % 256 != 0 and src.count - off[1] > 256 * 4      # several workgroups each, the boundary inside one
    if name == "invalid_patch":
        has = (st & 0x3f) != 0
        assert (has & ((st & 0x40) == 0)).sum() > 100 and (has & ((st & 0x40) != 0)).sum() > 100


def test_input_from_the_chained_sampled_call(dens, twin):
    """The buffers lfd_triangulate_sampled_chain wrote are refined as they are, in place (asynchronously, nothing read back in between)."""
    refs_h, refs_d = refs_for([(10, 3, False, False), (20, 3, False, False), (30, 2, False, False)], 64, 64)
    batch = hb.PreparedBatch(refs_d, sc.MATCH, sc.MATCH)
    M = 1000
    out = hb.OutputBuffers(3 * (M + 24 * 24 + 64), 3, batch.k, DEV)
    dens.seed_rng(5)
    dens.launch_sampled_chain(batch, sc.params(matches_per_ref=M, reproj_thresh=THR), M, out)
    with torch.cuda.stream(dens.stream):
        src = owned(out.collect(indexed=True, check_selection=True))
    assert src.count > 1000
    _st, n_acc, n_fall, n_wacc = compare(dens, twin, refs_h, refs_d, src, 1.6, buffers=out)
    assert n_wacc > 300 and n_fall > 20


def test_each_context_refuses_the_other_s_entry_point(dens, twin):
    lib = hb.load_library()
    null = (None, None, None, 1.0, 1.0, None, None, None, None, None)
    assert lib.lfd_refine_multiview_weighted_host(dens._ctx, *null) == LFD_ERR_STATE
    assert lib.lfd_refine_multiview_weighted(twin._ctx, *null) == LFD_ERR_STATE
    _refs_h, refs_d = refs_for([(10, 3, False, False)], 29, 37)
    batch = hb.PreparedBatch(refs_d, sc.MATCH, sc.MATCH)
    src = dens.triangulate_dense(batch, sc.params())
    with pytest.raises(ValueError, match="lives on|live on"):
        dens.refine_multiview(batch, sc.result_on_host(src), 1.6, THR, precision=True)
    with pytest.raises(ValueError, match="counters"):
        dens.refine_multiview(batch, src, 1.6, THR, counters=torch.zeros(3, dtype=torch.int64), precision=True)
    # a null plane in a valid slot is refused before anything is launched
    import ctypes as C
    holes = (C.c_void_p * 3)(batch.precision[0], None, batch.precision[2])
    buf = hb.OutputBuffers(29 * 37, 1, 3, DEV)
    dens.launch_dense(batch, sc.params(), buf)
    rc = lib.lfd_refine_multiview_weighted(dens._ctx, C.byref(batch.c), C.byref(buf.c), buf.ref_offsets.data_ptr(), 1.6, THR, buf.c.xyz, buf.c.err,
                                           None, None, C.cast(holes, C.c_void_p))
    assert rc == 1 and b"precision" in lib.lfd_last_error(dens._ctx)
    dens.check_launches()


@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_the_driver_on_the_device_emits_the_host_run_s_cells(tmp_path_factory, mode):
    """The tie-free, noise-free slab scene of tests/cycle_scene.py (only decisions far from every threshold are the same on both backends by
    construction), with the support filter in front: the weighted re-triangulation moves points and never changes which (cell, slot) a run
    emits, on either backend."""
    import cycle_scene
    scene = cycle_scene.make_scene(str(tmp_path_factory.mktemp("wrefine_gpu")))
    kw = dict(occlusion_steps=True, out_of_range=0.3, noise_px=0.0, outlier_frac=0.05, cert_mode="tiefree")
    exp = {"min_support_views": 2, "multiview_refine": True, "precision_weighted_refine": True}
    with cycle_scene.recorded_cells() as host_cells:
        host = cycle_scene.run(scene, cycle_scene.matcher_for(scene, **kw), "host.ply", triangulation_mode=mode, experimental=exp)
    with cycle_scene.recorded_cells() as dev_cells:
        dev = cycle_scene.run(scene, cycle_scene.matcher_for(scene, **kw), "dev.ply", backend="device", device=DEV, triangulation_mode=mode,
                              experimental=exp)
    n = len(scene["refs"])
    # the host backend collects a reference's points and then the filter's result (they alternate); the device routes collect once
    assert len(host_cells) == 2 * n and len(dev_cells) == n and host.xyz.shape[0] > 500
    assert dev_cells == host_cells[1::2]
    assert dev.xyz.shape[0] == host.xyz.shape[0] and np.array_equal(dev.points_per_reference, host.points_per_reference)
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    assert np.array_equal(bits(dev.rgb), bits(host.rgb))
