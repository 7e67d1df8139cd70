"""The CPU twin of the fused refiner block (lfd_refiner_block_host through HostDensifier.refiner_block) against the f64
yardstick of tests/refiner_block_ref.py under the derived bound - the bound holds while nothing under- or overflows in bf16, and these inputs
are O(1) -, the sanity case that the bound is tight enough to tell a one-pixel shift, NaN and signed-zero handling, and independence of the
thread count.  torch's own bf16 autocast sequence is printed beside the fused result for information; only the fused one is gated."""
import numpy as np
import pytest
import torch

import refiner_block_ref as R
from lichtfeld_densification_plugin_amd.core import hip_backend as hb


@pytest.fixture(scope="module")
def twin():
    d = hb.HostDensifier(8)
    yield d
    d.close()


def fallback_ratio(d, pointwise):
    """worst |torch's autocast sequence - ref| / bound on a case, on the CPU"""
    blk = R.stand_in_block(d)
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
        h = blk.relu(blk.norm(blk.conv_depthwise(torch.from_numpy(d["xb"].copy()).to(torch.bfloat16))))
        out = blk.conv_pointwise(h) if pointwise else h
    return R.violations(R.to_numpy(out), d["ref"], d["bound"])[1]


@pytest.mark.parametrize("variant", R.VARIANTS, ids=R.variant_id)
def test_the_twin_is_inside_the_bound(twin, variant):
    shape, f32, pw = variant
    d = R.case(shape, pw)
    out = twin.refiner_block(*R.tensors(d, f32, pw))
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == shape and out.is_contiguous()
    bad, worst = R.violations(R.to_numpy(out), d["ref"], d["bound"])
    print(f"{R.variant_id(variant)}: fused worst |out - ref| / bound = {worst:.4f} ({bad} outside); torch's autocast sequence: "
          f"{fallback_ratio(d, pw):.2f}")
    assert bad == 0, (variant, bad, worst)


def test_an_f32_input_is_rounded_on_load(twin):
    """... to the very bf16 values: the two input forms give the same bits"""
    d = R.case((1, 32, 17, 67), True)
    a = twin.refiner_block(*R.tensors(d, False, True))
    b = twin.refiner_block(*R.tensors(d, True, True))
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_a_non_contiguous_input_is_copied_first(twin):
    d = R.case((2, 32, 7, 9), False)
    x, *rest = R.tensors(d, True, False)
    want = twin.refiner_block(x, *rest)
    strided = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)          # channels last: same values, other strides
    assert not strided.is_contiguous()
    assert torch.equal(twin.refiner_block(strided, *rest).view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("pointwise", [False, True], ids=["dw", "pw"])
def test_the_input_shifted_by_one_pixel_is_outside_the_bound(twin, pointwise):
    """the bound is no blanket: the block of the same input moved by one pixel along x misses it by a wide margin"""
    d = R.case((1, 32, 35, 131), pointwise)
    x, *rest = R.tensors(d, False, pointwise)
    out = twin.refiner_block(torch.roll(x, 1, dims=3), *rest)
    bad, worst = R.violations(R.to_numpy(out), d["ref"], d["bound"])
    print(f"shifted by one pixel, pointwise {pointwise}: {bad} of {out.numel()} outside, worst ratio {worst:.0f}")
    assert bad > out.numel() // 2 and worst > 100.0


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
def test_a_nan_appears_exactly_where_its_window_reaches(twin, f32):
    shape = (2, 32, 7, 9)
    d = R.case(shape, False)
    b, c, y, x0 = 1, 5, 3, 7
    for pointwise in (False, True):
        x, *rest = R.tensors(R.case(shape, pointwise), f32, pointwise)
        x[b, c, y, x0] = float("nan")
        out = R.to_numpy(twin.refiner_block(x, *rest))
        want = np.zeros(shape, bool)
        rows, cols = slice(max(0, y - 2), y + 3), slice(max(0, x0 - 2), x0 + 3)
        if pointwise:
            want[b, :, rows, cols] = True                    # every output channel of the pixels whose window holds it
        else:
            want[b, c, rows, cols] = True
        assert np.array_equal(np.isnan(out), want)
        bits = R.bf16_bits(out[np.isnan(out)])
        assert ((bits & 0x7FC0) == 0x7FC0).all()             # quiet NaNs
    assert d["dw_w"].reshape(32, 25)[c].all()                # (no zero weight hides a tap)


def test_negative_zero_becomes_positive_zero(twin):
    """g = fmaf(s, a, t) = -0 (s = -1, t = -0 on an all-zero window) comes out as +0, and so does any negative g"""
    C = 3
    x = torch.zeros(1, C, 4, 5, dtype=torch.bfloat16)
    x[0, 2] = 1.0
    w = torch.ones(C, 25)
    s = torch.tensor([-1.0, 1.0, -1.0])
    t = torch.tensor([-0.0, -0.0, 0.5])
    out = twin.refiner_block(x, w, s, t)
    assert (out.view(torch.int16) == 0).all()                # the bits of +0 everywhere: -0, +0 + -0, and negative values under the ReLU


def test_the_result_does_not_depend_on_the_thread_count():
    one, eight = hb.HostDensifier(1), hb.HostDensifier(8)
    try:
        assert one.n_threads == 1 and eight.n_threads == 8
        for shape, f32, pw in [((1, 32, 35, 131), False, True), ((1, 128, 20, 70), True, False), ((2, 32, 7, 9), False, False)]:
            args = R.tensors(R.case(shape, pw), f32, pw)
            assert torch.equal(one.refiner_block(*args).view(torch.int16), eight.refiner_block(*args).view(torch.int16))
    finally:
        one.close()
        eight.close()


def test_the_numpy_rounding_is_torchs():
    """the yardstick's integer bf16 rounding against torch's conversion, ties and NaN included"""
    rng = np.random.RandomState(0)
    v = np.concatenate([rng.standard_normal(4096).astype(np.float32) * 10.0 ** rng.randint(-20, 20, 4096),
                        np.array([1.00390625, 1.01171875, -1.00390625, 0.0, -0.0, np.inf, -np.inf, 3.3895314e38], np.float32)])
    assert np.array_equal(R.bf16_round(v).view(np.uint32), torch.from_numpy(v).to(torch.bfloat16).float().numpy().view(np.uint32))
    assert np.isnan(R.bf16_round(np.array([np.nan], np.float32))).all()
