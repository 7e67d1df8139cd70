"""The depth-uncertainty gate on the device (lfd_depth_sigma_filter through HipDensifier.depth_sigma_filter) against the CPU twin - both sides are
given the SAME input points, the device's own - over the smallest grids and neighbour counts that take every path of the launch (one and several
workgroups per reference, a reference boundary inside a workgroup, an empty reference, ragged slots, masks, four-channel warps, k = 1, each of the
three slot-count instantiations, a plane with an invalid patch), each winner-only, with the device's own refine status and in the isotropic form.
Both sides evaluate the same f64 expressions and differ only in lfd_recip_refined / lfd_sqrt_rare, far below half an f32 ulp: finite sigma_rel
agrees within 1 ulp, +inf occurs at the same points, and with a threshold placed midway between two sorted twin sigmas more than 4 ulp apart the
compacted arrays, offsets, per-slot counts and sigma_rel_out are the twin's bit for bit.  Two launches give the same bits, the input may come from
the dense kernel or from the chained sampled call, and both contexts refuse each other's entry point."""
import dataclasses

import numpy as np
import pytest
import torch

import refine_ref as rr
import support_scene as sc
import wrefine_scene as ws
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LFD_ERR_STATE = 4
THR = ws.THR
ISO = 0.5


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


def ulps(a, b):
    """Distance in f32 ulps between two arrays of positive finite floats."""
    return np.abs(rr.bits(a).astype(np.int64) - rr.bits(b).astype(np.int64))


def gap_threshold(sigma, q=0.5):
    """A threshold midway between two sorted sigmas that are more than 4 ulp apart, near the q-quantile of the finite ones: no point sits within
    rounding of it."""
    s = np.sort(sigma[np.isfinite(sigma)])
    i0 = int(q * (s.size - 1))
    for i in list(range(i0, s.size - 1)) + list(range(i0 - 1, -1, -1)):
        if int(ulps(s[i:i + 1], s[i + 1:i + 2])[0]) > 4:
            mid = np.float32(0.5 * (np.float64(s[i]) + np.float64(s[i + 1])))
            if s[i] < mid < s[i + 1]:
                return float(mid)
    raise AssertionError("no gap of more than 4 ulp between two sorted sigmas")


def compare(dens, twin, refs_h, refs_d, src, tau, form):
    """One form of the gate on the device's points ``src`` (collected, owning its arrays) against the twin on the same points.  form: "winner"
    (planes, no status), "status" (planes, the device's own refine status over its own refined points) or "iso" (isotropic, with that status).
    Returns (points in, points kept, points with +inf)."""
    batch_d, batch_h = hb.PreparedBatch(refs_d, sc.MATCH, sc.MATCH), hb.PreparedBatch(refs_h, sc.MATCH, sc.MATCH)
    status = None
    if form != "winner":
        src, status = dens.refine_multiview(batch_d, src, tau, THR, with_status=True, precision=True)
    iso = ISO if form == "iso" else 0.0
    kw = dict(iso_sigma_px=iso, refine_status=status, support_thresh_px=tau if status is not None else 0.0, with_sigma=True)
    kw_h = dict(kw, refine_status=status.cpu() if status is not None else None)
    src_h = sc.result_on_host(src)
    res0, sigma, sigma_out0 = dens.depth_sigma_filter(batch_d, src, 0.0, **kw)
    dens.check_launches()
    ref0, sigma_h, _so = twin.depth_sigma_filter(batch_h, src_h, 0.0, **kw_h)
    sg, sh = sigma.cpu().numpy(), sigma_h.numpy()
    fin = np.isfinite(sh)
    assert not np.isnan(sg).any() and np.array_equal(np.isposinf(sg), np.isposinf(sh))
    worst = int(ulps(sg[fin], sh[fin]).max()) if fin.any() else 0
    n_diff = int((rr.bits(sg)[fin] != rr.bits(sh)[fin]).sum())
    assert worst <= 1, f"finite sigma_rel differs from the twin's by up to {worst} ulp"
    assert sc.same_points(res0, src) and np.array_equal(rr.bits(sigma_out0), rr.bits(sigma))          # annotate only: everything is copied
    mx = gap_threshold(sh)
    res, sigma2, sigma_out = dens.depth_sigma_filter(batch_d, src, mx, **kw)
    again, sigma3, sigma_out3 = dens.depth_sigma_filter(batch_d, src, mx, **kw)
    dens.check_launches()
    want, _s, want_out = twin.depth_sigma_filter(batch_h, src_h, mx, **kw_h)
    assert np.array_equal(rr.bits(sigma2), rr.bits(sigma)) and np.array_equal(rr.bits(sigma3), rr.bits(sigma))
    assert sc.same_points(res, again) and np.array_equal(rr.bits(sigma_out), rr.bits(sigma_out3))
    assert sc.same_points(sc.result_on_host(res), want), "the compacted arrays, offsets or per-slot counts differ from the twin's"
    assert np.array_equal(rr.bits(sigma_out), rr.bits(want_out))
    keep = sg <= np.float32(mx)
    sc.check_is_stable_subset(src, res, torch.from_numpy(keep.astype(np.uint8)), 1, batch_d.k)
    assert res.sigma_in == src.count and 0 < res.count < src.count                                    # keeps some, drops some
    print(f"{form}: {src.count} points, {int((~fin).sum())} +inf, {n_diff} finite sigmas differ from the twin's (at most {worst} ulp), threshold "
          f"{mx:.6g} keeps {res.count}")
    return src.count, res.count, int((~fin).sum())


# (tau 3.0 at k = 8 and k = 12, as in tests/test_gpu_wrefine.py)
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
def test_device_against_the_twin(dens, twin, name):
    H, W, channels, tau, patch, spec = CASES[name]
    refs_h, refs_d = refs_for(spec, H, W, channels, patch)
    batch = hb.PreparedBatch(refs_d, sc.MATCH, sc.MATCH)
    out = hb.OutputBuffers(len(spec) * H * W, len(spec), batch.k, DEV)
    dens.launch_dense(batch, sc.params(reproj_thresh=THR), out)
    dens.check_launches()
    with torch.cuda.stream(dens.stream):
        src = owned(out.collect())
    off = np.asarray(src.ref_offsets)
    n_inf = {}
    for form in ("winner", "status", "iso"):
        _n, _kept, n_inf[form] = compare(dens, twin, refs_h, refs_d, src, tau, form)
    if name == "ragged_3_refs_empty_middle":
        assert off[1] > 0 and off[1] == off[2] and off[3] > off[2]
    if name == "128x128_two_refs":
        assert off[1] > 256 * 4 and off[1] % 256 != 0 and src.count - off[1] > 256 * 4      # several workgroups each, the boundary inside one
    if name == "invalid_patch":
        assert n_inf["winner"] > 100 and n_inf["iso"] == 0                                  # the patch's own winners have no valid view
    # the buffers form: the launch's own buffers through the gate, asynchronously, into new ones
    _r0, sigma, _o = dens.depth_sigma_filter(batch, src, 0.0, with_sigma=True)
    mx = gap_threshold(sigma.cpu().numpy())
    got = dens.depth_sigma_filter(batch, out, mx)
    assert isinstance(got, hb.OutputBuffers) and got is not out and got.sigma_filtered
    dens.check_launches()
    with torch.cuda.stream(dens.stream):
        res = got.collect()
    want = dens.depth_sigma_filter(batch, src, mx)
    assert sc.same_points(res, want) and res.sigma_in == src.count and res.support_in is None


def test_input_from_the_chained_sampled_call(dens, twin):
    """The buffers lfd_triangulate_sampled_chain wrote are gated as they are (asynchronously, nothing read back in between)."""
    refs_h, refs_d = refs_for([(10, 3, False, False), (20, 3, False, False), (30, 2, False, False)], 64, 64)
    batch = hb.PreparedBatch(refs_d, sc.MATCH, sc.MATCH)
    M = 1000
    out = hb.OutputBuffers(3 * (M + 24 * 24 + 64), 3, batch.k, DEV)
    dens.seed_rng(5)
    dens.launch_sampled_chain(batch, sc.params(matches_per_ref=M, reproj_thresh=THR), M, out)
    with torch.cuda.stream(dens.stream):
        src = owned(out.collect(indexed=True, check_selection=True))
    assert src.count > 1000
    for form in ("winner", "status", "iso"):
        compare(dens, twin, refs_h, refs_d, src, 1.6, form)
    _r0, sigma, _o = dens.depth_sigma_filter(batch, src, 0.0, with_sigma=True)
    mx = gap_threshold(sigma.cpu().numpy())
    got = dens.depth_sigma_filter(batch, out, mx)
    dens.check_launches()
    with torch.cuda.stream(dens.stream):
        res = got.collect(indexed=True)
    want = dens.depth_sigma_filter(batch, src, mx)
    assert sc.same_points(res, want) and res.sigma_in == src.count and np.array_equal(res.sel_status, src.sel_status)


def test_each_context_refuses_the_other_s_entry_point(dens, twin):
    lib = hb.load_library()
    null = (None, None, None, None, 0.5, None, 0.0, 0.0, None, None, None, None, None)
    assert lib.lfd_depth_sigma_filter_host(dens._ctx, *null) == LFD_ERR_STATE
    assert lib.lfd_depth_sigma_filter(twin._ctx, *null) == LFD_ERR_STATE
    _refs_h, refs_d = refs_for([(10, 3, False, False)], 29, 37)
    batch = hb.PreparedBatch(refs_d, sc.MATCH, sc.MATCH)
    src = dens.triangulate_dense(batch, sc.params())
    with pytest.raises(ValueError, match="lives on|live on"):
        dens.depth_sigma_filter(batch, sc.result_on_host(src), 0.05)
    with pytest.raises(ValueError, match="refine_status"):
        dens.depth_sigma_filter(batch, src, 0.05, refine_status=torch.zeros(src.count, dtype=torch.uint8), support_thresh_px=1.6)
    # a null plane in a valid slot is refused before anything is launched
    import ctypes as C
    holes = (C.c_void_p * 3)(batch.precision[0], None, batch.precision[2])
    buf, dst = hb.OutputBuffers(29 * 37, 1, 3, DEV), hb.OutputBuffers(29 * 37, 1, 3, DEV)
    dens.launch_dense(batch, sc.params(), buf)
    rc = lib.lfd_depth_sigma_filter(dens._ctx, C.byref(batch.c), C.byref(buf.c), buf.ref_offsets.data_ptr(), C.cast(holes, C.c_void_p), 0.0, None, 0.0,
                                    0.05, C.byref(dst.c), dst.ref_offsets.data_ptr(), None, None, None)
    assert rc == 1 and b"precision" in lib.lfd_last_error(dens._ctx)
    dens.check_launches()


@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_the_driver_on_the_device_emits_the_host_run_s_cells(tmp_path_factory, mode):
    """The tie-free, noise-free slab scene of tests/cycle_scene.py with the support filter in front of the gate: the threshold sits in a gap of
    the host run's sigmas (found with a run whose gate keeps every finite one), so both backends take the same decisions."""
    import cycle_scene
    from test_depth_sigma_driver import joined, recorded_gates
    scene = cycle_scene.make_scene(str(tmp_path_factory.mktemp("sigma_gpu")))
    kw = dict(occlusion_steps=True, out_of_range=0.3, noise_px=0.0, outlier_frac=0.05, cert_mode="tiefree")
    exp = {"min_support_views": 2, "match_sigma_px": ISO}
    with recorded_gates() as (seen, _order):
        cycle_scene.run(scene, cycle_scene.matcher_for(scene, **kw), "probe.ply", triangulation_mode=mode, experimental={**exp, "max_depth_sigma_rel": 1e30})
    exp["max_depth_sigma_rel"] = gap_threshold(joined(seen, "sigma"))
    with cycle_scene.recorded_cells() as host_cells:
        host = cycle_scene.run(scene, cycle_scene.matcher_for(scene, **kw), "host.ply", triangulation_mode=mode, experimental=exp)
    with cycle_scene.recorded_cells() as dev_cells:
        dev = cycle_scene.run(scene, cycle_scene.matcher_for(scene, **kw), "dev.ply", backend="device", device=DEV, triangulation_mode=mode,
                              experimental=exp)
    n = len(scene["refs"])
    # the host backend collects a reference's points, the filter's result and the gate's (in turn); the device routes collect once
    assert len(host_cells) == 3 * n and len(dev_cells) == n and 300 < host.xyz.shape[0]
    assert dev_cells == host_cells[2::3] and sum(len(c) for c in host_cells[1::3]) > host.xyz.shape[0]
    assert dev.xyz.shape[0] == host.xyz.shape[0] and np.array_equal(dev.points_per_reference, host.points_per_reference)
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    assert np.array_equal(bits(dev.rgb), bits(host.rgb))
