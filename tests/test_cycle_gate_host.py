"""CPU tier of the forward-backward gate: the twin (lfd_cycle_gate_host) against the f64 reference of tests/cycle_ref.py under its derived
bound, and the contract of the entry point (exact zeros, +inf, border clamping, layouts, aliasing, the floor, the counters, argument errors).

Measured on the probe scenes (512^2, ring of 185 cameras, reference 10, three neighbours, 0.5 px noise, 5 % outliers, out_of_range 0.3), share of the
786 432 cells inside the band / decisions that differ from the reference's outside it:
    smooth surface   tau 0.5: 0.0337 % / 0    tau 1: 0.0067 % / 0    tau 2: 0.0037 % / 0
    depth steps      tau 0.5: 0.0306 % / 0    tau 1: 0.0065 % / 0    tau 2: 0.0036 % / 0
The cap is 0.5 %.  Largest |e_f32 - e_ref| / bound over all cells with a finite error: 0.194 (smooth), 0.183 (steps)."""
import ctypes as C

import numpy as np
import pytest
import torch

import cycle_ref
from lichtfeld_densification_plugin_amd import synthetic as syn
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

LFD_ERR_INVALID = 1
BAND_CAP = 0.005
_cache = {}


@pytest.fixture(scope="module")
def twin():
    d = hb.HostDensifier(4)
    yield d
    d.close()


def probe(occlusion: bool, channels: int = 2):
    key = (occlusion, channels)
    if key not in _cache:
        cams = syn.ring_cameras(185)
        _cache[key] = cycle_ref.probe_inputs(cams, 10, syn.ring_neighbours(185, 10, 3), 512, 512, 512, 512, channels=channels,
                                             occlusion_steps=occlusion, out_of_range=0.3)
    return _cache[key]


@pytest.mark.parametrize("tau", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("occlusion", [False, True])
def test_twin_takes_the_reference_decision_outside_the_band(twin, occlusion, tau):
    cert, wab, wba = probe(occlusion)
    rejected = torch.zeros(3, dtype=torch.int32)
    outs, errs = twin.cycle_gate(cert, wab, wba, 512, 512, 0.2, tau, with_err=True, rejected=rejected)
    in_band = cells = 0
    worst = 0.0
    for j in range(3):
        ref = cycle_ref.reference(cert[j].numpy(), wab[j].numpy(), wba[j].numpy(), 512, 512, 0.2, tau)
        wrong, neither, bad_err, share = cycle_ref.check_against_reference(ref, outs[j].numpy(), errs[j].numpy())
        fin = np.isfinite(ref["e"]) & (ref["bound"] > 0)
        worst = max(worst, float((np.abs(errs[j].numpy().astype(np.float64) - ref["e"])[fin] / ref["bound"][fin]).max()))
        in_band += int(ref["band"].sum())
        cells += ref["band"].size
        assert wrong == 0, f"pair {j}: {wrong} decisions outside the band differ from the reference's"
        assert neither == 0 and bad_err == 0, f"pair {j}: {neither} in-band outputs are neither c nor 0, {bad_err} errors outside the bound"
        # the counter is the number of zeros the gate wrote (every kept cell carries the floor 0.2 > 0)
        assert int(rejected[j]) == int((outs[j] == 0).sum())
        kept = float(ref["keep"].mean())
        assert 0.1 < kept < 0.95, f"the filter must bite and must not empty the pair: kept {kept:.3f}"
    print(f"occlusion={occlusion} tau={tau}: in band {100.0 * in_band / cells:.4f} % of {cells} cells, worst |e - e_ref| / bound {worst:.3f}")
    assert in_band / cells <= BAND_CAP


def test_depth_steps_are_what_the_filter_rejects():
    """The slabs of ``occlusion_steps`` exist in the reference's image only: the neighbour's own field does not come back across them."""
    kept = []
    for occlusion in (False, True):
        cert, wab, wba = probe(occlusion)
        kept.append(np.mean([cycle_ref.reference(cert[j].numpy(), wab[j].numpy(), wba[j].numpy(), 512, 512, 0.2, 1.0)["keep"].mean() for j in range(3)]))
    assert kept[1] < kept[0] - 0.05


def small_case(H=12, W=16, Hb=12, Wb=16, C_=2, seed=0):
    rng = np.random.RandomState(seed)
    cert = torch.from_numpy(rng.uniform(0.0, 1.0, (H, W)).astype(np.float32))
    wab = torch.from_numpy(rng.uniform(-1.0, 1.0, (H, W, C_)).astype(np.float32))
    # a backward field that is nearly the inverse of nothing in particular: smooth + noise, in [-1, 1]
    wba = torch.from_numpy(rng.uniform(-1.0, 1.0, (Hb, Wb, 2)).astype(np.float32))
    return cert, wab, wba


def test_outside_nan_and_inf_coordinates_give_exact_zero_and_plus_inf(twin):
    cert, wab, wba = small_case()
    cert[:] = 0.7
    bad = [float("nan"), float("inf"), float("-inf"), 1.0000001, -1.0000001, 3.0e38, -2.5]
    for i, v in enumerate(bad):
        wab[0, i, 0] = v                      # x outside
        wab[1, i, 1] = v                      # y outside
    wab[2, 0] = torch.tensor([1.0, -1.0])     # the closed border is inside
    wab[2, 1] = torch.tensor([-1.0, 1.0])
    outs, errs = twin.cycle_gate([cert], [wab], [wba], 16, 12, 0.2, 1e9, with_err=True)
    o, e = outs[0], errs[0]
    for i in range(len(bad)):
        for row in (0, 1):
            assert o[row, i].item() == 0.0 and np.signbit(o[row, i].item()) == False  # noqa: E712
            assert e[row, i].item() == float("inf")
    assert o[2, 0].item() == np.float32(0.7) and o[2, 1].item() == np.float32(0.7) and torch.isfinite(e[2, :2]).all()
    ref = cycle_ref.reference(cert.numpy(), wab.numpy(), wba.numpy(), 16, 12, 0.2, 1e9)
    assert cycle_ref.check_against_reference(ref, o.numpy(), e.numpy())[:3] == (0, 0, 0)


def test_a_nan_in_the_backward_warp_rejects_and_a_nan_certainty_stays(twin):
    cert, wab, wba = small_case(seed=1)
    wba[3, 4, 0] = float("nan")
    cert[5, 5] = float("nan")
    wab[5, 5] = torch.tensor([0.9, 0.9])      # far from the poisoned texel
    outs, errs = twin.cycle_gate([cert], [wab], [wba], 16, 12, 0.2, 1e9, with_err=True)
    ref = cycle_ref.reference(cert.numpy(), wab.numpy(), wba.numpy(), 16, 12, 0.2, 1e9)
    hit = np.isnan(ref["e"])
    assert hit.any() and (outs[0].numpy()[hit] == 0).all() and np.isnan(errs[0].numpy()[hit]).all()
    assert np.isnan(outs[0][5, 5].item())
    assert cycle_ref.check_against_reference(ref, outs[0].numpy(), errs[0].numpy())[:3] == (0, 0, 0)


def test_taps_are_clamped_at_the_border(twin):
    """Within half a texel of the edge both taps of an axis are the edge texel: the blend is that texel's value (padding_mode='border')."""
    Hb, Wb = 5, 7
    wba = torch.zeros((Hb, Wb, 2))
    wba[..., 0] = torch.linspace(-0.9, 0.9, Wb).view(1, Wb)
    wba[..., 1] = torch.linspace(-0.8, 0.8, Hb).view(Hb, 1)
    wab = torch.tensor([[[-1.0, -1.0], [1.0, 1.0], [-1.0 + 0.5 / Wb, 1.0 - 0.5 / Hb], [0.0, -1.0]]])        # (1, 4, 2)
    cert = torch.full((1, 4), 0.5)
    ax, ay = torch.zeros(4), torch.zeros(1)                                                               # xa = ya = 0: the error is |A'| in px
    _outs, errs = twin.cycle_gate([cert], [wab], [wba], 3, 3, 0.2, 1e9, axes=(ax, ay), with_err=True)     # 0.5 (3 - 1) = 1 px per unit
    e = errs[0][0].numpy().astype(np.float64)
    want = [np.hypot(0.9, 0.8), np.hypot(0.9, 0.8), np.hypot(0.9, 0.8), np.hypot(0.0, 0.8)]
    assert np.allclose(e, want, rtol=0, atol=1e-6), (e, want)


@pytest.mark.parametrize("channels", [2, 4])
@pytest.mark.parametrize("grid_b", [(64, 64), (40, 56)])
def test_layouts_two_and_four_channels_and_a_backward_grid_of_another_size(twin, channels, grid_b):
    cams = syn.ring_cameras(185)
    nbrs = syn.ring_neighbours(185, 20, 2)
    cert, wab, wba = cycle_ref.probe_inputs(cams, 20, nbrs, 64, 64, 512, 512, channels=channels, occlusion_steps=True)
    if grid_b != (64, 64):      # the neighbour's field on a coarser grid of its own
        wba = [cycle_ref.probe_inputs(cams, n, [20], grid_b[0], grid_b[1], 512, 512)[1][0] for n in nbrs]
    outs, errs = twin.cycle_gate(cert, wab, wba, 512, 512, 0.2, 1.0, with_err=True)
    for j in range(2):
        ref = cycle_ref.reference(cert[j].numpy(), wab[j].numpy(), wba[j].numpy(), 512, 512, 0.2, 1.0)
        assert cycle_ref.check_against_reference(ref, outs[j].numpy(), errs[j].numpy())[:3] == (0, 0, 0)
        assert 0.05 < ref["keep"].mean() < 0.98
    if channels == 4:           # the same cells with the A-coordinates taken from the axes: the same bits
        two = [w[..., 2:].contiguous() for w in wab]
        outs2, _ = twin.cycle_gate(cert, two, wba, 512, 512, 0.2, 1.0)
        assert all(torch.equal(a, b) for a, b in zip(outs, outs2))
        ax, ay = torch.from_numpy(hb.identity_axis(64)), torch.from_numpy(hb.identity_axis(64))
        outs3, _ = twin.cycle_gate(cert, two, wba, 512, 512, 0.2, 1.0, axes=(ax, ay))
        assert all(torch.equal(a, b) for a, b in zip(outs, outs3))


def test_reference_axis_is_the_library_s():
    for n in (1, 2, 7, 64, 512, 1280):
        assert np.array_equal(cycle_ref.identity_axis(n), hb.identity_axis(n))


def test_a_width_that_is_no_multiple_of_four(twin):
    cert, wab, wba = small_case(H=9, W=13, Hb=6, Wb=5, seed=3)
    outs, errs = twin.cycle_gate([cert], [wab], [wba], 40, 30, 0.2, 6.0, with_err=True)
    ref = cycle_ref.reference(cert.numpy(), wab.numpy(), wba.numpy(), 40, 30, 0.2, 6.0)
    assert cycle_ref.check_against_reference(ref, outs[0].numpy(), errs[0].numpy())[:3] == (0, 0, 0)
    assert 0 < ref["keep"].sum() < ref["keep"].size


def test_in_place_equals_out_of_place(twin):
    cert, wab, wba = probe(True)
    outs, _ = twin.cycle_gate(cert, wab, wba, 512, 512, 0.2, 1.0)
    mine = [c.clone() for c in cert]
    same, _ = twin.cycle_gate(mine, wab, wba, 512, 512, 0.2, 1.0, inplace=True)
    assert all(s is m for s, m in zip(same, mine))
    assert all(torch.equal(a, b) for a, b in zip(outs, mine))
    assert not torch.equal(mine[0], cert[0])


def test_kept_cells_carry_the_floor_and_the_kernels_floor_of_zero_leaves_them_alone(twin):
    cert, wab, wba = probe(False)
    cert = [(c * 0.3).contiguous() for c in cert]          # (the probe's low certainties all sit on cells that leave the neighbour's image)
    outs, _ = twin.cycle_gate(cert, wab, wba, 512, 512, 0.2, 1.0)
    o, c = outs[0], cert[0]
    kept = o != 0
    assert (c < 0.2).any() and float(o[kept].min()) == np.float32(0.2)
    assert torch.equal(o[kept], torch.where(c < 0.2, torch.tensor(np.float32(0.2)), c)[kept])
    # a threshold of 0 floors nothing that is not negative; a negative one lets raw values through
    raw, _ = twin.cycle_gate(cert, wab, wba, 512, 512, -1.0, 1.0)
    assert torch.equal(raw[0][kept], c[kept]) and torch.equal(raw[0] == 0, ~kept | (c == 0))
    # gating a gated plane again with the floor min(thresh, 0) changes nothing: what the hot path relies on
    again, _ = twin.cycle_gate(outs, wab, wba, 512, 512, 0.0, 1.0)
    assert all(torch.equal(a, b) for a, b in zip(again, outs))


def test_counters_are_added_to(twin):
    cert, wab, wba = probe(True)
    rejected = torch.tensor([5, 0, 7, 11], dtype=torch.int32)
    outs, _ = twin.cycle_gate(cert, wab, wba, 512, 512, 0.2, 1.0, rejected=rejected)
    zeros = [int((o == 0).sum()) for o in outs]
    assert rejected.tolist() == [5 + zeros[0], zeros[1], 7 + zeros[2], 11]
    twin.cycle_gate(cert, wab, wba, 512, 512, 0.2, 1.0, rejected=rejected)
    assert rejected.tolist() == [5 + 2 * zeros[0], 2 * zeros[1], 7 + 2 * zeros[2], 11]


def test_sixteen_pairs_in_one_call_and_seventeen_refused(twin):
    cert, wab, wba = small_case(seed=4)
    one, _ = twin.cycle_gate([cert], [wab], [wba], 16, 12, 0.2, 2.0)
    outs, _ = twin.cycle_gate([cert] * 16, [wab] * 16, [wba] * 16, 16, 12, 0.2, 2.0)
    assert len(outs) == 16 and all(torch.equal(o, one[0]) for o in outs)
    with pytest.raises(hb.HipBackendError, match="n_pairs"):
        twin.cycle_gate([cert] * 17, [wab] * 17, [wba] * 17, 16, 12, 0.2, 2.0)


def test_every_argument_error_is_lfd_err_invalid():
    lib = hb.load_library()
    ctx = C.c_void_p()
    assert lib.lfd_create_host(1, C.byref(ctx)) == 0
    cert, wab, wba = small_case()
    out = torch.empty_like(cert)
    tab = lambda t: (C.c_void_p * 1)(t.data_ptr())
    null1 = (C.c_void_p * 1)(None)
    good = dict(n=1, cert=tab(cert), wab=tab(wab), wba=tab(wba), H=12, W=16, C_=2, Hb=12, Wb=16, ax=None, ay=None, wm=16, hm=12, th=0.2, tau=1.0,
                out=tab(out), err=None, rej=None)

    def call(**kw):
        a = {**good, **kw}
        return lib.lfd_cycle_gate_host(ctx, a["n"], a["cert"], a["wab"], a["wba"], a["H"], a["W"], a["C_"], a["Hb"], a["Wb"], a["ax"], a["ay"], a["wm"],
                                       a["hm"], a["th"], a["tau"], a["out"], a["err"], a["rej"])
    try:
        assert call() == 0
        axis = torch.zeros(16)
        bad = [dict(n=0), dict(n=17), dict(n=-1), dict(cert=None), dict(wab=None), dict(wba=None), dict(out=None), dict(cert=null1), dict(wab=null1),
               dict(wba=null1), dict(out=null1), dict(err=null1), dict(H=0), dict(W=0), dict(Hb=0), dict(Wb=0), dict(H=32769), dict(W=32769),
               dict(Hb=32769), dict(Wb=40000), dict(C_=1), dict(C_=3), dict(C_=8), dict(tau=0.0), dict(tau=-1.0), dict(tau=float("inf")),
               dict(tau=float("nan")), dict(wm=0), dict(hm=0), dict(ax=axis.data_ptr()), dict(ay=axis.data_ptr())]
        for kw in bad:
            assert call(**kw) == LFD_ERR_INVALID, kw
            assert b"lfd_cycle_gate_host" in lib.lfd_last_error(ctx)
        assert call() == 0
        assert lib.lfd_cycle_gate_host(None, 1, None, None, None, 1, 1, 2, 1, 1, None, None, 1, 1, 0.2, 1.0, None, None, None) == LFD_ERR_INVALID
    finally:
        lib.lfd_destroy(ctx)


def test_binding_refuses_what_the_library_would_read_wrongly(twin):
    cert, wab, wba = small_case()
    with pytest.raises(ValueError, match="contiguous float32"):
        twin.cycle_gate([cert.double()], [wab], [wba], 16, 12, 0.2, 1.0)
    with pytest.raises(ValueError, match="contiguous float32"):
        twin.cycle_gate([cert.t()], [wab], [wba], 16, 12, 0.2, 1.0)
    with pytest.raises(ValueError, match="of one size"):
        twin.cycle_gate([cert], [wab[:5]], [wba], 16, 12, 0.2, 1.0)
    with pytest.raises(ValueError, match="rejected"):
        twin.cycle_gate([cert], [wab], [wba], 16, 12, 0.2, 1.0, rejected=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match="at least one pair"):
        twin.cycle_gate([], [], [], 16, 12, 0.2, 1.0)
