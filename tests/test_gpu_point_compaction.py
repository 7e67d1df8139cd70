"""The compaction tail the three gates behind triangulation share (lfd_compact_launch: the support filter, the depth-uncertainty gate and the
photo-consistency gate hand it a keep byte per point) and the one workspace they carve for it.

  one workspace, changing sizes   the gates run one after the other on ONE context and stream, nothing read back in between, on inputs of
                                  alternating size - so every call finds the keep bytes, the workgroup counts and the f32 plane of the call
                                  before it, at other offsets - and every output equals what the same call gives on a fresh context; the keep
                                  decisions are the twin's
  nothing to do                   offsets that are all zero over a capacity that is not, and a capacity of zero: the scan alone runs, writes
                                  zero offsets, and nothing else is written

The scan's loop over more than 1024 workgroups is reached by tests/test_gpu_stage_scale.py (four references of 288 x 288, 1296 workgroups, through
the support filter and the depth-uncertainty gate) and is not repeated here."""
import ctypes as C

import numpy as np
import pytest
import torch

import support_scene as sc
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from test_gpu_depth_sigma import gap_threshold
from test_gpu_support_filter import refs_for

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TAU = 1.6
ISO = 0.5                      # the gate's isotropic form: the scenes of support_scene carry no precision planes
RADIUS, MIN_NCC, MIN_TEXTURE = 2, 0.8, 2.0
SMALL = (29, 37, 4, [(10, 8, False, False)])                                    # tests/test_gpu_support_filter.py: "37x29_k8_c4"
LARGE = (128, 128, 2, [(10, 3, False, False), (25, 4, False, False)])           # ... "128x128_two_refs"


def fresh_context():
    d = hb.HipDensifier(DEV)
    d.upload_cameras(sc.cameras())
    return d


@pytest.fixture(scope="module")
def dens():
    d = fresh_context()
    yield d
    d.close()


@pytest.fixture(scope="module")
def twin():
    d = hb.HostDensifier(16)
    d.upload_cameras(sc.cameras())
    yield d
    d.close()


def scene(dens, case):
    """(device batch, host batch, the dense kernel's points in their launch buffers, the same points collected)."""
    H, W, channels, spec = case
    refs = [sc.with_neighbour_images(ri, DEV) for ri in refs_for(spec, H, W, channels)]
    batch = hb.PreparedBatch(refs, sc.MATCH, sc.MATCH)
    buf = hb.OutputBuffers(len(refs) * H * W, len(refs), batch.k, DEV)
    dens.launch_dense(batch, sc.params(), buf)
    with torch.cuda.stream(dens.stream):
        src = buf.collect(indexed=True)
    dens.check_launches()
    return batch, hb.PreparedBatch(sc.on_host(refs), sc.MATCH, sc.MATCH), buf, src


def run_gate(d, gate, batch, buf, mx):
    """One gate over the launch buffers ``buf``, asynchronously: (result buffers, its tensors per INPUT point, its tensors per KEPT point)."""
    if gate == "sigma":
        dst, sigma, sigma_out = d.depth_sigma_filter(batch, buf, mx, iso_sigma_px=ISO, with_sigma=True)
        return dst, [sigma], [sigma_out]
    if gate == "support":
        dst, support = d.support_filter(batch, buf, 1, TAU, with_support=True)
        return dst, [support], []
    dst, status, ncc = d.photo_gate(batch, buf, RADIUS, MIN_NCC, MIN_TEXTURE, with_status=True, with_ncc=True)
    return dst, [status, ncc], []


def read(d, n_in, dst, per_input, per_kept):
    """The collected result and the bit patterns of the gate's own tensors, trimmed to the points they describe."""
    with torch.cuda.stream(d.stream):
        res = dst.collect(indexed=True)
    d.check_launches()
    return res, [sc.bits(t[:n_in]).copy() for t in per_input] + [sc.bits(t[:res.count]).copy() for t in per_kept]


def test_one_workspace_serves_gates_of_changing_sizes(dens, twin):
    small, large = scene(dens, SMALL), scene(dens, LARGE)
    assert large[3].count > 8 * small[3].count > 0
    # thresholds of the two sigma calls: midway between two of the twin's sigmas more than 4 ulp apart, so that no decision hangs on a rounding
    mx = {}
    for name, (_bd, bh, _buf, src) in (("small", small), ("large", large)):
        _r, sig, _so = twin.depth_sigma_filter(bh, sc.result_on_host(src), 0.0, iso_sigma_px=ISO, with_sigma=True)
        mx[name] = gap_threshold(sig.numpy())
    calls = [("sigma", "small", small), ("support", "large", large), ("photo", "small", small), ("sigma", "large", large)]
    # the sequence: nothing is read back between the calls
    pending = [run_gate(dens, gate, sc_[0], sc_[2], mx[name]) for gate, name, sc_ in calls]
    got = [read(dens, c[2][3].count, *out) for c, out in zip(calls, pending)]
    for (gate, name, (batch_d, batch_h, buf, src)), (res, planes) in zip(calls, got):
        assert 0 < res.count < src.count, (gate, name, res.count, src.count)                # the gate keeps some and drops some
        # ... what the same call gives on a context that has run nothing else
        alone = fresh_context()
        try:
            res1, planes1 = read(alone, src.count, *run_gate(alone, gate, batch_d, buf, mx[name]))
            assert sc.same_points(res, res1), (gate, name, res.ref_offsets, res1.ref_offsets)
            assert len(planes) == len(planes1) and all(np.array_equal(a, b) for a, b in zip(planes, planes1)), (gate, name)
        finally:
            alone.close()
        # ... and the twin's decisions on the same points
        src_h = sc.result_on_host(src)
        if gate == "sigma":
            want, _s, want_out = twin.depth_sigma_filter(batch_h, src_h, mx[name], iso_sigma_px=ISO, with_sigma=True)
            assert np.array_equal(planes[1], sc.bits(want_out))
        elif gate == "support":
            want, sup = twin.support_filter(batch_h, src_h, 1, TAU, with_support=True)
            assert np.array_equal(planes[0], sup.numpy())
        else:
            want, status, _ncc = twin.photo_gate(batch_h, src_h, RADIUS, MIN_NCC, MIN_TEXTURE, with_status=True, with_ncc=True)
            assert np.array_equal(planes[0], status.numpy())
        assert sc.same_points(sc.result_on_host(res), want), (gate, name, res.ref_offsets, want.ref_offsets)
        print(f"{gate} on {name}: {src.count} points in, {res.count} kept")


def call_gate(dens, gate, batch, src, dst, sigma_out):
    """The library's entry point itself (the wrappers of hip_backend copy the source's offsets into the destination before the call, which would
    hide whether the scan wrote them)."""
    lib, off, seg = dens._lib, dst.ref_offsets.data_ptr(), dst.seg_counts.data_ptr()
    with torch.cuda.stream(dens.stream):
        if gate == "support":
            rc = lib.lfd_support_filter(dens._ctx, C.byref(batch.c), C.byref(src.c), src.ref_offsets.data_ptr(), 1, C.c_float(TAU), C.byref(dst.c),
                                        off, seg, None)
        elif gate == "sigma":
            rc = lib.lfd_depth_sigma_filter(dens._ctx, C.byref(batch.c), C.byref(src.c), src.ref_offsets.data_ptr(), None, C.c_float(ISO), None,
                                            C.c_float(0.0), C.c_float(0.05), C.byref(dst.c), off, seg, None, sigma_out.data_ptr())
        else:
            rc = lib.lfd_photo_gate(dens._ctx, C.byref(batch.c), C.byref(src.c), src.ref_offsets.data_ptr(), C.cast(batch.nbr_images, C.c_void_p),
                                    RADIUS, C.c_float(MIN_NCC), C.c_float(MIN_TEXTURE), C.byref(dst.c), off, seg, None, None, None)
    dens._check(rc, gate)


@pytest.mark.parametrize("capacity", [600, 0])
@pytest.mark.parametrize("gate", ["support", "sigma", "photo"])
def test_nothing_to_do(dens, gate, capacity):
    """All offsets zero - over a capacity of 600 (three workgroups that retire at once) and over a capacity of zero (no workgroup: the scan
    alone is launched)."""
    refs = [sc.with_neighbour_images(ri, DEV) for ri in refs_for([(10, 3, False, False), (20, 2, False, False)], 29, 37)]
    batch = hb.PreparedBatch(refs, sc.MATCH, sc.MATCH)
    src, dst = hb.OutputBuffers(capacity, 2, batch.k, DEV), hb.OutputBuffers(capacity, 2, batch.k, DEV)
    sigma_out = torch.full((max(capacity, 1),), 0.25, dtype=torch.float32, device=DEV)
    with torch.cuda.stream(dens.stream):
        src._f.fill_(0.125)
        src.cell.fill_(3)
        src.slot.fill_(1)
        dst._f.fill_(0.5)
        dst.cell.fill_(-7)
        dst.slot.fill_(77)
        dst.ref_offsets.fill_(7)
        dst.seg_counts.fill_(7)
    assert int(src.ref_offsets.abs().sum()) == 0
    call_gate(dens, gate, batch, src, dst, sigma_out)
    dens.check_launches()
    torch.cuda.synchronize()
    assert dst.ref_offsets.tolist() == [0, 0, 0]
    assert int(dst.seg_counts.abs().sum()) == 0
    assert bool((dst._f == 0.5).all()) and bool((dst.cell == -7).all()) and bool((dst.slot == 77).all()) and bool((sigma_out == 0.25).all())
