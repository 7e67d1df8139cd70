"""The multi-view support filter on the device (lfd_support_filter through HipDensifier.support_filter): the compacted arrays, the offsets, the
per-slot counts and the support counts equal the CPU twin's bit for bit - both sides are given the SAME input points, the device's own - over
grids and neighbour counts that take every path of the launch (one and several workgroups per reference, a reference boundary inside a
workgroup, an empty reference, ragged slots, masks, four-channel warps, k = 1, each of the three slot-count instantiations); two launches give
the same bits; the input may come from the dense kernel or from the chained sampled call; both contexts refuse each other's entry point; and the
driver with backend="device" emits the (cell, slot) sets of the host-backend run."""
import numpy as np
import pytest
import torch

import cycle_scene
import support_scene as sc
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LFD_ERR_STATE = 4
TAU = 1.6


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


def refs_for(spec, H, W, channels=2):
    """spec: (reference, k, masks, dead) per reference; ``dead``: the reference's own mask blanks it - the dense kernel has no candidate there."""
    out = []
    for ref, k, masks, dead in spec:
        _s, ri = sc.reference_inputs(ref, k, H, W, channels=channels, masks=masks, device=DEV)
        if dead:
            ri.mask_a = torch.zeros((sc.MATCH, sc.MATCH), dtype=torch.uint8, device=DEV)
        out.append(ri)
    return out


def compare(dens, twin, refs, src, min_support, src_buffers=None):
    """The device's filter on ``src`` (collected; ``src_buffers``: the launch's OutputBuffers instead) against the twin's on the same points."""
    batch = hb.PreparedBatch(refs, sc.MATCH, sc.MATCH)
    if src_buffers is not None:
        dst, sup = dens.support_filter(batch, src_buffers, min_support, TAU, with_support=True)
        with torch.cuda.stream(dens.stream):
            got = dst.collect(indexed=True)
        sup = sup[:src.count]
    else:
        got, sup = dens.support_filter(batch, src, min_support, TAU, with_support=True)
    dens.check_launches()
    refs_h = sc.on_host(refs)
    want, sup_h = twin.support_filter(hb.PreparedBatch(refs_h, sc.MATCH, sc.MATCH), sc.result_on_host(src), min_support, TAU, with_support=True)
    assert sc.same_points(got, want), (got.ref_offsets, want.ref_offsets, got.seg_counts, want.seg_counts)
    assert np.array_equal(sup.cpu().numpy(), sup_h.numpy())
    sc.check_is_stable_subset(src, got, sup, min_support, batch.k)
    return got, sup


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
def test_device_equals_the_twin_bit_for_bit(dens, twin, name):
    H, W, channels, spec = CASES[name]
    refs = refs_for(spec, H, W, channels)
    src = dens.triangulate_dense(hb.PreparedBatch(refs, sc.MATCH, sc.MATCH), sc.params())
    off = np.asarray(src.ref_offsets)
    k_min = min(len(r.cert) for r in refs)
    got, sup = compare(dens, twin, refs, src, 1)
    if name == "k1":
        assert src.count > 1000 and got.count == 0 and int(sup.max()) == 0
    else:
        assert 0 < got.count < src.count                                   # the filter bites and does not empty the cloud
    if name == "empty_reference":
        assert off[1] == off[2] and off[1] > 0 and off[3] > off[2]
    if name == "128x128_two_refs":
        assert off[1] > 256 * 4 and off[1] % 256 != 0 and src.count - off[1] > 256 * 4      # several workgroups each, the boundary inside one
    if k_min > 2:
        got2, _ = compare(dens, twin, refs, src, k_min - 1)
        assert got2.count <= got.count


def test_two_launches_give_the_same_bits(dens):
    refs = refs_for([(10, 3, True, False), (25, 3, False, False)], 128, 128)
    batch = hb.PreparedBatch(refs, sc.MATCH, sc.MATCH)
    src = dens.triangulate_dense(batch, sc.params())
    a, sa = dens.support_filter(batch, src, 1, TAU, with_support=True)
    b, sb = dens.support_filter(batch, src, 1, TAU, with_support=True)
    assert sc.same_points(a, b) and torch.equal(sa, sb) and 0 < a.count < src.count


def test_input_from_the_chained_sampled_call(dens, twin):
    """The buffers lfd_triangulate_sampled_chain wrote go through the filter as they are (asynchronously, nothing read back in between); the
    first-appearance slot groups keep their order, and the selection status travels with the points."""
    refs = refs_for([(10, 3, False, False), (20, 3, False, False), (30, 2, False, False)], 96, 96)
    batch = hb.PreparedBatch(refs, sc.MATCH, sc.MATCH)
    M = 1500
    out = hb.OutputBuffers(3 * (M + 24 * 24 + 64), 3, batch.k, DEV)
    dens.seed_rng(5)
    dens.launch_sampled_chain(batch, sc.params(matches_per_ref=M), M, out)
    with torch.cuda.stream(dens.stream):
        src = out.collect(indexed=True, check_selection=True)
    assert src.count > 2000
    got, _sup = compare(dens, twin, refs, src, 1, src_buffers=out)
    assert np.array_equal(got.sel_status, src.sel_status) and got.n_selected == src.n_selected and 0 < got.count < src.count


def test_each_context_refuses_the_other_s_entry_point(dens, twin):
    lib = hb.load_library()
    assert lib.lfd_support_filter_host(dens._ctx, None, None, None, 1, 1.0, None, None, None, None) == LFD_ERR_STATE
    assert lib.lfd_support_filter(twin._ctx, None, None, None, 1, 1.0, None, None, None, None) == LFD_ERR_STATE
    refs = refs_for([(10, 3, False, False)], 29, 37)
    src = dens.triangulate_dense(hb.PreparedBatch(refs, sc.MATCH, sc.MATCH), sc.params())
    with pytest.raises(ValueError, match="lives on|live on"):
        dens.support_filter(hb.PreparedBatch(refs, sc.MATCH, sc.MATCH), sc.result_on_host(src), 1, TAU)


@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_the_driver_on_the_device_emits_the_host_run_s_cells(tmp_path_factory, mode):
    """The tie-free, noise-free slab scene of tests/cycle_scene.py, for the reason tests/test_gpu_cycle_gate.py gives: the host sampling stage
    orders tied weights differently, and the twin divides in IEEE where the kernels use the 1-ulp reciprocal, so only decisions far from every
    threshold are the same on both backends by construction.  Noise-free fields put the residual of a correct neighbour near 0; the 5 % outliers
    (a random coordinate: hundreds of pixels off) are what the filter finds, with both other neighbours required."""
    scene = cycle_scene.make_scene(str(tmp_path_factory.mktemp("support_gpu")))
    kw = dict(occlusion_steps=True, out_of_range=0.3, noise_px=0.0, outlier_frac=0.05, cert_mode="tiefree")
    exp = {"min_support_views": 2}
    with cycle_scene.recorded_cells() as host_cells:
        host = cycle_scene.run(scene, cycle_scene.matcher_for(scene, **kw), "host.ply", triangulation_mode=mode, experimental=exp)
    with cycle_scene.recorded_cells() as dev_cells:
        dev = cycle_scene.run(scene, cycle_scene.matcher_for(scene, **kw), "dev.ply", backend="device", device=DEV, triangulation_mode=mode,
                              experimental=exp)
    with cycle_scene.recorded_cells() as off_cells:
        off = cycle_scene.run(scene, cycle_scene.matcher_for(scene, **kw), "off.ply", backend="device", device=DEV, triangulation_mode=mode)
    n = len(scene["refs"])
    # the recorder sees every buffer a run collects.  The host backend collects a reference's points and then the filter's result (one reference
    # per call: they alternate); the device routes launch the filter behind the triangulation and collect its result alone.
    assert len(host_cells) == 2 * n and len(dev_cells) == n and len(off_cells) == n and host.xyz.shape[0] > 500
    unfiltered, filtered = host_cells[0::2], host_cells[1::2]
    print(f"{mode}: filter off {off.xyz.shape[0]} points, on: host {host.xyz.shape[0]}, device {dev.xyz.shape[0]}; per reference |host|, |device|, "
          f"|symmetric difference|: {[(len(a), len(b), len(a ^ b)) for a, b in zip(filtered, dev_cells)]}")
    assert all(f <= u for f, u in zip(filtered, unfiltered))
    assert dev_cells == filtered
    assert dev.xyz.shape[0] == host.xyz.shape[0] and np.array_equal(dev.points_per_reference, host.points_per_reference)
    assert dev.xyz.shape[0] < off.xyz.shape[0] and off_cells != dev_cells        # the filter changed what the device run emits
