"""The fused refiner-block kernels on the device (lfd_refiner_block through HipDensifier.refiner_block and the model-facing shim, DESIGN.md
4.18): bit for bit the CPU twin on every shape and variant, inside the derived bound of tests/refiner_block_ref.py (valid while nothing
under- or overflows in bf16: the inputs are O(1)), context reuse, stream ordering, the shim against torch's own operators on the device -
whose distance to the f64 reference is printed for information, only the fused one is gated - and the refusals through a device context."""

import pytest
import torch

import refiner_block_ref as R
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from lichtfeld_densification_plugin_amd.core.refiner_blocks import FusedRefinerBlocks
from test_refiner_block_abi import LFD_ERR_INVALID, LFD_ERR_STATE, invalid_calls

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


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
    return t.contiguous().view(torch.int16).cpu()


@pytest.mark.parametrize("variant", R.VARIANTS, ids=R.variant_id)
def test_device_equals_the_twin_bit_for_bit_and_is_inside_the_bound(dens, twin, variant):
    shape, f32, pw = variant
    d = R.case(shape, pw)
    out = dens.refiner_block(*R.tensors(d, f32, pw, DEV))
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == shape and out.device == DEV and out.is_contiguous()
    host = twin.refiner_block(*R.tensors(d, f32, pw))
    differing = int((bits(out) != bits(host)).sum())
    bad, worst = R.violations(R.to_numpy(out), d["ref"], d["bound"])
    print(f"{R.variant_id(variant)}: {differing} of {out.numel()} elements differ from the twin; worst |out - ref| / bound = {worst:.4f} ({bad} outside)")
    assert differing == 0
    assert bad == 0, (variant, bad, worst)


def test_nan_and_signed_zero_as_on_the_twin(dens, twin):
    d = R.case((2, 32, 7, 9), True)
    for pw in (False, True):
        x, *rest = R.tensors(d, True, pw)
        x[1, 5, 3, 4] = float("nan")
        x[0, 0, 0, 0] = -0.0
        want = twin.refiner_block(x, *rest)
        got = dens.refiner_block(x.to(DEV), *[None if t is None else t.to(DEV) for t in rest])
        assert torch.equal(bits(got), bits(want))
        assert int(torch.isnan(got.float()).sum()) == (25 * 32 if pw else 25)


def test_a_small_call_after_a_larger_one_on_the_same_context(dens, twin):
    """nothing of the larger launch (grid, staged tiles) leaks into the next one"""
    big, small = R.case((1, 32, 35, 131), True), R.case((1, 3, 4, 5), False)
    first = dens.refiner_block(*R.tensors(big, False, True, DEV))
    second = dens.refiner_block(*R.tensors(small, False, False, DEV))
    third = dens.refiner_block(*R.tensors(big, True, False, DEV))
    assert torch.equal(bits(first), bits(twin.refiner_block(*R.tensors(big, False, True))))
    assert torch.equal(bits(second), bits(twin.refiner_block(*R.tensors(small, False, False))))
    assert torch.equal(bits(third), bits(twin.refiner_block(*R.tensors(big, True, False))))


def test_a_call_on_a_side_stream_is_ordered_with_torch_work_around_it(twin):
    """the shim points its context at torch's current stream: the input is produced on that stream right before the call and the output is
    consumed on it right after, with no synchronisation in between"""
    d = R.case((1, 32, 35, 131), True)
    x, *rest = R.tensors(d, True, True, DEV)
    blk = R.stand_in_block(d, device=DEV)
    shim = FusedRefinerBlocks()
    side = torch.cuda.Stream(device=DEV)
    try:
        torch.cuda.synchronize(DEV)
        with torch.cuda.stream(side):
            half = x * 0.5                                   # torch work before ...
            doubled = half + half                            # ... (exact: the input again)
            out = shim.forward(blk, doubled)
            after = out.float() * 2.0                        # ... and after
        side.synchronize()
        assert int(shim._ctx[DEV].stream.cuda_stream) == int(side.cuda_stream)
        want = twin.refiner_block(*R.tensors(d, True, True))
        assert torch.equal(bits(out), bits(want))
        assert torch.equal(after.cpu(), want.float() * 2.0)
        out2 = shim.forward(blk, x)                          # back on the default stream
        torch.cuda.synchronize(DEV)
        assert torch.equal(bits(out2), bits(want))
    finally:
        shim.close()


@pytest.mark.parametrize("shape", [(1, 32, 35, 131), (1, 128, 20, 70), (1, 33, 9, 9)], ids=lambda s: "x".join(map(str, s)))
def test_the_shim_on_device_tensors_against_torchs_own_operators(shape):
    C_ch = shape[1]
    d = R.case(shape, C_ch == 32)
    blk = R.stand_in_block(d, device=DEV)
    x = torch.from_numpy(d["x"].copy()).to(DEV)
    shim = FusedRefinerBlocks()
    seen = []
    hook = blk.conv_pointwise.register_forward_hook(lambda m, inp, out: seen.append(inp[0]))
    try:
        with torch.no_grad():
            plain = blk(x)
            n_plain = len(seen)
            with _installed_on(shim, blk):
                fused = blk(x)
            assert "forward" not in blk.__dict__
        assert fused.dtype == torch.bfloat16 and fused.shape == plain.shape and fused.device == DEV
        if C_ch == 32:
            assert len(seen) == n_plain                      # one launch: the block's own 1x1 convolution did not run
            bad, worst = R.violations(R.to_numpy(fused), d["ref"], d["bound"])
            theirs = R.violations(R.to_numpy(plain), d["ref"], d["bound"])[1]
            print(f"{shape}: fused block worst |out - ref| / bound = {worst:.4f} ({bad} outside); torch's operators on the device: {theirs:.2f}")
            assert bad == 0
        else:
            assert len(seen) == n_plain + 1                  # the general launch, then the block's own conv_pointwise on the hidden value
            hidden = seen[-1]
            bad, worst = R.violations(R.to_numpy(hidden), d["ref"], d["bound"])
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                theirs_h = blk.relu(blk.norm(blk.conv_depthwise(x)))
            theirs = R.violations(R.to_numpy(theirs_h), d["ref"], d["bound"])[1]
            print(f"{shape}: fused hidden value worst |out - ref| / bound = {worst:.4f} ({bad} outside); torch's operators on the device: {theirs:.2f}; "
                  f"max |fused block - torch's block| = {float((fused.float() - plain.float()).abs().max()):.4f}")
            assert bad == 0 and hidden.dtype == torch.bfloat16
    finally:
        hook.remove()
        shim.close()


def _installed_on(shim, blk):
    """``installed`` wants a model with ``refiners``"""
    model = torch.nn.Module()
    model.refiners = torch.nn.ModuleDict({"1": torch.nn.Sequential(blk)})
    return shim.installed(model)


def test_the_refusals_through_a_device_context(dens):
    lib = dens._lib
    keep, cases = invalid_calls()
    for what, args, piece in cases:
        assert lib.lfd_refiner_block(dens._ctx, *args) == LFD_ERR_INVALID, what
        msg = lib.lfd_last_error(dens._ctx).decode()
        assert msg.startswith("lfd_refiner_block: ") and piece in msg, (what, msg)
    assert lib.lfd_refiner_block_host(dens._ctx, *cases[0][1]) == LFD_ERR_STATE      # the twin's call on a device context
    # ... and through the binding and the shim
    d = R.case((1, 3, 4, 5), False)
    x, w, s, t, _, _ = R.tensors(d, False, False, DEV)
    with pytest.raises(hb.HipBackendError, match="pointwise fusion implements C == 32 only"):
        dens.refiner_block(x, w, s, t, torch.zeros(3, 3, device=DEV), torch.zeros(3, device=DEV))
    with pytest.raises(ValueError, match="lives on"):
        dens.refiner_block(x.cpu(), w, s, t)
    shim = FusedRefinerBlocks()
    try:
        with pytest.raises(NotImplementedError, match="float16"):
            shim.forward(R.stand_in_block(d, device=DEV), x.half())
    finally:
        shim.close()
    assert dens.refiner_block(x, w, s, t).shape == x.shape                          # the context still works
