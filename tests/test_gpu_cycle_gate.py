"""The forward-backward gate on the device (lfd_cycle_gate through HipDensifier.cycle_gate): cert_out and the counters equal the CPU twin's bit
for bit at the grids of the five RoMa presets with 1, 3 and 8 pairs per launch, two runs give the same output, the device meets the f64
reference of tests/cycle_ref.py under the rule of tests/test_cycle_gate_host.py, both contexts refuse each other's entry point, and the driver
with backend="device" emits the (cell, slot) sets of the host-backend run in both modes."""
import ctypes as C

import numpy as np
import pytest
import torch

import cycle_ref
import cycle_scene
from lichtfeld_densification_plugin_amd import synthetic as syn
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LFD_ERR_STATE = 4
BAND_CAP = 0.005


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


@pytest.fixture(scope="module")
def cams():
    return syn.ring_cameras(185)


def bits(t):
    return t.contiguous().view(torch.int32)


def inputs(cams, side, k, channels=2, ref=10, **kw):
    """the probe's fields, made on the device (f64 torch arithmetic: the same values as on the host up to the library's own rounding - both
    sides of every comparison below read the SAME tensors)"""
    kw = {"occlusion_steps": True, "out_of_range": 0.3, **kw}
    return cycle_ref.probe_inputs(cams, ref, syn.ring_neighbours(185, ref, k), side, side, min(side, 800), min(side, 800), device=DEV,
                                  channels=channels, **kw)


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("side", [320, 512, 960, 1280])
def test_device_equals_the_twin_bit_for_bit(dens, twin, cams, side, k):
    cert, wab, wba = inputs(cams, side, k, channels=4 if (side == 512 and k == 3) else 2)
    wm = min(side, 800)
    rej = torch.tensor([3] * k, dtype=torch.int32, device=DEV)
    outs, errs = dens.cycle_gate(cert, wab, wba, wm, wm, 0.2, 1.0, with_err=True, rejected=rej)
    again, _ = dens.cycle_gate(cert, wab, wba, wm, wm, 0.2, 1.0, rejected=rej)
    torch.cuda.synchronize()
    rej_h = torch.tensor([3] * k, dtype=torch.int32)
    h = lambda ts: [t.cpu() for t in ts]
    outs_h, errs_h = twin.cycle_gate(h(cert), h(wab), h(wba), wm, wm, 0.2, 1.0, with_err=True, rejected=rej_h)
    for j in range(k):
        assert torch.equal(bits(outs[j]).cpu(), bits(outs_h[j])), (side, k, j)
        assert torch.equal(bits(again[j]), bits(outs[j]))                                  # two runs, the same bits
        e_d, e_h = errs[j].cpu().double(), errs_h[j].double()
        fin = torch.isfinite(e_h)
        assert torch.equal(torch.isfinite(e_d), fin) and torch.equal(e_d[~fin], e_h[~fin])
        assert bool(((e_d[fin] - e_h[fin]).abs() <= 2.0 ** -22 * e_h[fin]).all())          # the square root: 1 ulp on the device
    zeros = [int((o == 0).sum()) for o in outs_h]
    assert rej_h.tolist() == [3 + z for z in zeros]
    assert rej.cpu().tolist() == [3 + 2 * z for z in zeros]                                # added to, twice
    assert 0.02 < sum(zeros) / (k * side * side) < 0.98


def test_in_place_and_unaligned_layouts(dens, twin, cams):
    cert, wab, wba = inputs(cams, 320, 3)
    outs, _ = dens.cycle_gate(cert, wab, wba, 320, 320, 0.2, 1.0)
    mine = [c.clone() for c in cert]
    dens.cycle_gate(mine, wab, wba, 320, 320, 0.2, 1.0, inplace=True)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(outs, mine))
    # a width that is no multiple of four, and planes that start 4 bytes off a 16-byte boundary: the general kernel, the same bits as the twin
    H, W = 37, 50
    rs = np.random.RandomState(7)
    c = torch.from_numpy(rs.uniform(0, 1, (H, W)).astype(np.float32))
    w = torch.from_numpy(rs.uniform(-1.05, 1.05, (H, W, 2)).astype(np.float32))
    b = torch.from_numpy(rs.uniform(-1, 1, (23, 31, 2)).astype(np.float32))
    want, _ = twin.cycle_gate([c], [w], [b], 64, 48, 0.2, 8.0)
    got, _ = dens.cycle_gate([c.to(DEV)], [w.to(DEV)], [b.to(DEV)], 64, 48, 0.2, 8.0)
    assert torch.equal(bits(got[0]).cpu(), bits(want[0])) and 0 < int((want[0] == 0).sum()) < H * W
    H, W = 16, 32
    c, w = torch.from_numpy(rs.uniform(0, 1, (H, W)).astype(np.float32)), torch.from_numpy(rs.uniform(-1, 1, (H, W, 2)).astype(np.float32))
    want, _ = twin.cycle_gate([c], [w], [b], 64, 48, 0.2, 8.0)
    shifted = torch.empty(H * W + 1, dtype=torch.float32, device=DEV)
    shifted[1:] = c.reshape(-1).to(DEV)
    off = shifted[1:].view(H, W)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    got, _ = dens.cycle_gate([off], [w.to(DEV)], [b.to(DEV)], 64, 48, 0.2, 8.0)
    assert torch.equal(bits(got[0]).cpu(), bits(want[0]))


@pytest.mark.parametrize("side,occlusion", [(320, False), (512, True)])
def test_device_against_the_reference(dens, cams, side, occlusion):
    cert, wab, wba = inputs(cams, side, 3, occlusion_steps=occlusion)
    for tau in (0.5, 1.0, 2.0):
        outs, errs = dens.cycle_gate(cert, wab, wba, side, side, 0.2, tau, with_err=True)
        in_band = cells = 0
        for j in range(3):
            ref = cycle_ref.reference(cert[j].cpu().numpy(), wab[j].cpu().numpy(), wba[j].cpu().numpy(), side, side, 0.2, tau)
            wrong, neither, bad_err, _share = cycle_ref.check_against_reference(ref, outs[j].cpu().numpy(), errs[j].cpu().numpy())
            assert (wrong, neither, bad_err) == (0, 0, 0), (side, tau, j, wrong, neither, bad_err)
            in_band += int(ref["band"].sum())
            cells += ref["band"].size
        print(f"{side}^2 occlusion={occlusion} tau={tau}: in band {100.0 * in_band / cells:.4f} % of {cells} cells")
        assert in_band / cells <= BAND_CAP


def test_non_finite_coordinates_form_no_address(dens):
    H = W = 64
    cert = torch.full((H, W), 0.7, device=DEV)
    wab = torch.zeros((H, W, 2), device=DEV)
    bad = torch.tensor([float("nan"), float("inf"), float("-inf"), 3.0e38, -3.0e38, 1.0000001, 1e20, -7.0], device=DEV)
    wab[0, :8, 0] = bad
    wab[1, :8, 1] = bad
    wba = torch.zeros((H, W, 2), device=DEV)
    outs, errs = dens.cycle_gate([cert], [wab], [wba], 64, 64, 0.2, 1e9, with_err=True)
    torch.cuda.synchronize()
    assert bool((outs[0][:2, :8] == 0).all()) and bool(torch.isinf(errs[0][:2, :8]).all()) and bool((errs[0][:2, :8] > 0).all())
    assert bool((outs[0][2:] == np.float32(0.7)).all())


def test_device_context_is_refused_by_the_twin_s_entry_point(dens):
    lib = hb.load_library()
    assert lib.lfd_cycle_gate_host(dens._ctx, 1, None, None, None, 1, 1, 2, 1, 1, None, None, 1, 1, 0.2, 1.0, None, None, None) == LFD_ERR_STATE
    with pytest.raises(ValueError, match="lives on"):
        dens.cycle_gate([torch.zeros(4, 4)], [torch.zeros(4, 4, 2)], [torch.zeros(4, 4, 2)], 4, 4, 0.2, 1.0)


@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_the_driver_on_the_device_emits_the_host_run_s_cells(tmp_path_factory, mode):
    """The scene keeps the comparison about the gate.  Two things legitimately differ between the CPU twin and the device without it and are kept
    out by construction: (1) the host sampling stage orders tied weights with NumPy's unstable argsort (core/sampling.py), so the certainties
    are tie-free (``cert_mode="tiefree"``) - on the smooth field, where the floor and the cap tie thousands of cells, the two backends' coverage
    picks differ with the filter OFF already (measured on this scene: 96 / 118 / 74 / 1 / 0 / 1 cells per reference of ~1 250); (2) the twin
    divides in IEEE where the kernels use the 1-ulp reciprocal (include/lfd_densify.h), so a survivor within rounding of a geometric threshold
    may flip - the fields are noise-free, which puts every reprojection and Sampson error near 0, far from its threshold.  Depth steps and
    out-of-range columns remain: the gate rejects a large share of the cells."""
    scene = cycle_scene.make_scene(str(tmp_path_factory.mktemp("cycle_gpu")))
    kw = dict(occlusion_steps=True, out_of_range=0.3, noise_px=0.0, outlier_frac=0.0, cert_mode="tiefree")
    exp = {"cycle_thresh_px": 1.0}
    with cycle_scene.recorded_cells() as host_cells:
        host = cycle_scene.run(scene, cycle_scene.matcher_for(scene, **kw), "host.ply", triangulation_mode=mode, experimental=exp)
    # (the same matcher fields in every run - made on the host, moved to the device by the driver - so that the runs differ in the backend alone)
    with cycle_scene.recorded_cells() as dev_cells:
        dev = cycle_scene.run(scene, cycle_scene.matcher_for(scene, **kw), "dev.ply", backend="device", device=DEV, triangulation_mode=mode,
                              experimental=exp)
    with cycle_scene.recorded_cells() as off_cells:
        off = cycle_scene.run(scene, cycle_scene.matcher_for(scene, **kw), "off.ply", backend="device", device=DEV, triangulation_mode=mode)
    assert len(host_cells) == len(dev_cells) == len(scene["refs"]) and host.xyz.shape[0] > 500
    print(f"{mode}: per reference |host|, |device|, |symmetric difference|: {[(len(a), len(b), len(a ^ b)) for a, b in zip(host_cells, dev_cells)]}; "
          f"filter off: {off.xyz.shape[0]} points, at 1 px: {dev.xyz.shape[0]}")
    assert dev_cells == host_cells
    assert dev.xyz.shape[0] == host.xyz.shape[0]
    assert off_cells != dev_cells                                                          # the filter changed what the device run emits
