"""The fused refiner-head kernel on the device (lfd_refiner_head through HipDensifier.refiner_head and the model-facing shim):
against the CPU twin on every shape and variant - ``warp`` and ``conf[..., 0]`` bit for bit, ``conf[..., 1:4]``, which pass through the device's
own exp and log1p, within the derived device-to-twin distance of tests/refiner_head_ref.py, the number of differing values printed -, inside the
derived bound around the f64 reference, the exact cases, context reuse, stream ordering, the shim against torch's own tail on the device, and
the refusals through a device context."""

import numpy as np
import pytest
import torch

import refiner_head_ref as R
import test_refiner_head_shim as S
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from lichtfeld_densification_plugin_amd.core.refiner_head import FusedRefinerHead
from test_refiner_head_abi import LFD_ERR_INVALID, LFD_ERR_STATE, invalid_calls
from test_refiner_head_host import EXACT, check_exact, exact_call

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
# the 4-pixel lanes (2^18 pixels and more), vector and - with H W = 2 mod 4 - the 2-pixel fallback of a large call; the 256-thread workgroups
WIDE = [(R.WIDE_SHAPE, False, 4, True), (R.WIDE_SHAPE, True, 1, False), ((1, 2, 514, 511), False, 0, False), (R.LARGE_SHAPE, False, 4, True),
        ((2, 1, 1023, 513), True, 1, False)]


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


def bits(t):
    return t.contiguous().view(torch.int32).cpu()


def against_the_twin(got, want, ref, prev_dim, what):
    """warp and conf[..., 0]: the same bits.  conf[..., 1:4]: within the derived distance; the number of differing values is printed."""
    (gw, gc), (ww, wc) = got, want
    assert gw.device == DEV and gc.device == DEV and gw.dtype == gc.dtype == torch.float32 and gw.is_contiguous() and gc.is_contiguous()
    assert torch.equal(bits(gw), bits(ww)), what
    assert torch.equal(bits(gc[..., 0]), bits(wc[..., 0])), what
    _, _, rc, _, rd = ref
    tol = R.twin_bound(rc, rd, prev_dim)
    err = np.abs(R.to_numpy(gc).astype(np.float64) - wc.numpy().astype(np.float64))
    differing = int((bits(gc) != bits(wc)).sum())
    outside = int((~(err <= tol)).sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = float(np.nanmax(np.where(tol > 0, err / tol, 0.0)))
    print(f"{what}: {differing} of {gc.numel()} confidence values differ from the twin, worst distance / derived bound = {worst:.4f} ({outside} outside)")
    assert outside == 0, what


@pytest.mark.parametrize("variant", R.VARIANTS + WIDE, ids=R.variant_id)
def test_device_against_the_twin_and_inside_the_bound(dens, twin, variant):
    shape, f32, prev_dim, planar = variant
    d = R.case(shape, prev_dim)
    got = dens.refiner_head(*R.tensors(d, f32, planar, DEV))
    B, _, H, W = shape
    assert tuple(got[0].shape) == (B, H, W, 2) and tuple(got[1].shape) == (B, H, W, 4)
    want = twin.refiner_head(*R.tensors(d, f32, planar))
    ref = d["ref32" if f32 else "ref"]
    against_the_twin(got, want, ref, prev_dim, R.variant_id(variant))
    rw, bw, rc, bc, _ = ref
    (bad_w, worst_w), (bad_c, worst_c) = R.violations(R.to_numpy(got[0]), rw, bw), R.violations(R.to_numpy(got[1]), rc, bc)
    print(f"{R.variant_id(variant)}: worst |out - ref| / bound: warp {worst_w:.4f} ({bad_w} outside), conf {worst_c:.4f} ({bad_c} outside)")
    assert bad_w == 0 and bad_c == 0


@pytest.mark.parametrize("prev_dim", [0, 1, 4])
def test_exact_cases_as_on_the_twin(dens, twin, prev_dim):
    warp, conf = exact_call(dens, EXACT, prev_dim, device=DEV)
    check_exact(warp, conf, EXACT, prev_dim)                                        # threshold sides, +-inf, NaN in exactly the pixels that read it
    tw, tc = exact_call(twin, EXACT, prev_dim)
    assert np.array_equal(warp.view(np.uint32), tw.view(np.uint32)) and np.array_equal(conf[:, 0].view(np.uint32), tc[:, 0].view(np.uint32))
    for i, value in enumerate(EXACT):
        if np.isnan(value):
            continue
        exact = value > 20.0 or np.isinf(value)                                    # softplus is the identity there: no library call
        for k in (1, 2, 3):
            a, b = float(conf[i, k]), float(tc[i, k])
            assert a == b or (not exact and abs(a - b) <= 2.0 ** -21 * abs(b)), (value, k, a, b)
    for pd, prev_value, bias in ((0, 0.0, -0.0), (1, 0.0, -0.0), (4, -0.0, -0.0), (1, -0.0, -0.0)):        # signed zero
        got, want = exact_call(dens, [-0.0], pd, prev_value, device=DEV, bias=bias), exact_call(twin, [-0.0], pd, prev_value, bias=bias)
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1][:, [0, 2]].view(np.uint32), want[1][:, [0, 2]].view(np.uint32))


def test_a_small_call_after_a_larger_one_on_the_same_context(dens, twin):
    """nothing of the larger launch (its grid, its lane width) leaks into the next one"""
    for shape, f32, pd, planar in ((R.WIDE_SHAPE, False, 4, True), ((1, 3, 4, 5), False, 1, True), ((1, 32, 17, 64), True, 4, False), ((1, 1, 1, 1), False, 0, False)):
        d = R.case(shape, pd)
        got, want = dens.refiner_head(*R.tensors(d, f32, planar, DEV)), twin.refiner_head(*R.tensors(d, f32, planar))
        against_the_twin(got, want, d["ref32" if f32 else "ref"], pd, f"{shape} after the previous call")


def test_a_call_on_a_side_stream_is_ordered_with_torch_work_around_it(twin):
    """the shim points its context at torch's current stream: z is produced on that stream right before the call and the outputs are consumed on
    it right after, with no synchronisation in between"""
    d = R.case((1, 32, 17, 64), 4)
    z, hw_, hb_, pw, pc = R.tensors(d, True, True, DEV)
    ctx = hb.HipDensifier(DEV)
    side = torch.cuda.Stream(device=DEV)
    try:
        torch.cuda.synchronize(DEV)
        with torch.cuda.stream(side):
            half = z * 0.5                                   # torch work before ...
            doubled = half + half                            # ... (exact: the input again)
            ctx.set_stream(torch.cuda.current_stream(DEV))
            warp, conf = ctx.refiner_head(doubled, hw_, hb_, pw, pc)
            after = warp * 2.0                               # ... and after
        side.synchronize()
        assert int(ctx.stream.cuda_stream) == int(side.cuda_stream)
        want = twin.refiner_head(*R.tensors(d, True, True))
        against_the_twin((warp, conf), want, d["ref32"], 4, "side stream")
        assert torch.equal(after.cpu(), want[0] * 2.0)
    finally:
        ctx.close()


@pytest.mark.parametrize("prev_dim", [1, 4])
def test_the_shim_on_device_tensors_against_torchs_own_tail(monkeypatch, prev_dim):
    monkeypatch.setattr(S, "DEVICE", DEV)
    refiner = S.make_refiner().to(DEV)
    kw = {k: (None if v is None else v.to(DEV)) for k, v in S.inputs(prev_dim, B=2, H=9, W=14).items()}
    assert not kw["prev_warp"].is_contiguous()                                      # the planar view survives the move
    shim = FusedRefinerHead()
    taps = S.Taps(refiner)
    side = torch.cuda.Stream(device=DEV)
    try:
        with torch.no_grad():
            plain = refiner(**kw)
            with shim.installed(S.model_with(refiner)):
                fused = refiner(**kw)
                torch.cuda.synchronize(DEV)
                with torch.cuda.stream(side):                                       # ... and it follows torch's current stream
                    again = refiner(**kw)
                side.synchronize()
            assert int(shim._ctx[DEV].stream.cuda_stream) == int(side.cuda_stream) and "forward" not in refiner.__dict__
        assert torch.equal(taps.d[0], taps.d[1]) and torch.equal(taps.z[0], taps.z[1]) and taps.z[1].dtype == torch.bfloat16
        bad, worst = S.inside_the_bound(refiner, taps.z[1], kw, fused)
        theirs = S.inside_the_bound(refiner, taps.z[0], kw, plain)[1]
        print(f"prev_dim {prev_dim}: fused tail worst |out - ref| / bound = {worst:.4f} ({bad} outside); torch's own tail on the device: {theirs:.4f}")
        assert bad == 0 and fused["warp"].device == DEV
        assert torch.equal(bits(again["warp"]), bits(fused["warp"])) and torch.equal(bits(again["confidence"]), bits(fused["confidence"]))
    finally:
        taps.remove()
        shim.close()


def test_the_refusals_through_a_device_context(dens):
    lib = dens._lib
    keep, good, call, cases = invalid_calls()
    for what, args, piece in cases:                          # every one is refused before anything is launched: the pointers are never read
        assert lib.lfd_refiner_head(dens._ctx, *args) == LFD_ERR_INVALID, what
        msg = lib.lfd_last_error(dens._ctx).decode()
        assert msg.startswith("lfd_refiner_head: ") and piece in msg, (what, msg)
    assert lib.lfd_refiner_head_host(dens._ctx, *cases[0][1]) == LFD_ERR_STATE       # the twin's call on a device context
    # ... and through the binding and the shim
    d = R.case((1, 3, 4, 5), 4)
    z, hw_, hb_, pw, pc = R.tensors(d, False, False, DEV)
    with pytest.raises(hb.HipBackendError, match="prev_dim must be 0, 1 or 4"):
        dens.refiner_head(z, hw_, hb_, pw, pc[..., :2])
    with pytest.raises(hb.HipBackendError, match="refine_init must be finite and > 0"):
        dens.refiner_head(z, hw_, hb_, pw, pc, refine_init=float("nan"))
    with pytest.raises(ValueError, match="lives on"):
        dens.refiner_head(z.cpu(), hw_, hb_, pw, pc)
    with pytest.raises(ValueError, match="lives on"):
        dens.refiner_head(z, hw_, hb_, pw, pc.cpu())
    assert dens.refiner_head(z, hw_, hb_, pw, pc)[1].shape == (1, 4, 5, 4)          # the context still works
