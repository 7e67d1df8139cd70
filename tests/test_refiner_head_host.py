"""CPU tier of the fused refiner head (lfd_refiner_head_host): the twin against the f64 yardstick and its derived bound
(tests/refiner_head_ref.py) on every shape, input type, previous-state variant and layout - torch's own tail printed beside it -, proof that
the bound can tell a wrong result from a rounded one, the exact cases (softplus threshold, +-inf, NaN, signed zero) and bit equality across
thread counts."""
import numpy as np
import pytest
import torch

import refiner_head_ref as R
from lichtfeld_densification_plugin_amd.core import hip_backend as hb


@pytest.fixture(scope="module")
def host():
    ctx = hb.HostDensifier(2)
    yield ctx
    ctx.close()


def run(ctx, d, f32, planar=False):
    warp, conf = ctx.refiner_head(*R.tensors(d, f32, planar), refine_init=R.REFINE_INIT)
    assert warp.dtype == conf.dtype == torch.float32 and warp.is_contiguous() and conf.is_contiguous()
    B, _, H, W = d["z"].shape
    assert tuple(warp.shape) == (B, H, W, 2) and tuple(conf.shape) == (B, H, W, 4)
    return warp.numpy(), conf.numpy()


@pytest.mark.parametrize("variant", R.VARIANTS, ids=R.variant_id)
def test_the_twin_is_inside_the_bound(host, variant):
    shape, f32, prev_dim, planar = variant
    d = R.case(shape, prev_dim)
    warp, conf = run(host, d, f32, planar)
    rw, bw, rc, bc, _ = d["ref32" if f32 else "ref"]
    (bad_w, worst_w), (bad_c, worst_c) = R.violations(warp, rw, bw), R.violations(conf, rc, bc)
    wh, ch = R.stand_in_heads(d)
    z, _, _, pw, pc = R.tensors(d, f32, planar)
    tw, tc = R.torch_tail(z, wh, ch, pw, pc)
    print(f"{R.variant_id(variant)}: twin worst |out - ref| / bound: warp {worst_w:.4f}, conf {worst_c:.4f}; torch's own tail: "
          f"warp {R.violations(R.to_numpy(tw), rw, bw)[1]:.4f}, conf {R.violations(R.to_numpy(tc), rc, bc)[1]:.4f}")
    assert bad_w == 0 and bad_c == 0


def test_the_bound_tells_a_wrong_result_from_a_rounded_one(host):
    shape = (2, 32, 7, 9)
    d = R.case(shape, 4)
    rw, bw, rc, bc, _ = d["ref"]
    z, hw_, hb_, pw, pc = R.tensors(d, False)
    # the same inputs with z shifted by one pixel
    warp, conf = host.refiner_head(torch.roll(z, 1, dims=3), hw_, hb_, pw, pc)
    fw, fc = R.violations(warp.numpy(), rw, bw)[1], R.violations(conf.numpy(), rc, bc)[1]
    print(f"z shifted by one pixel: warp {fw:.3g} x the bound, conf {fc:.3g} x")
    assert fw > 1e3 and fc > 1e3
    # head rows 3 and 5 swapped: l00 and l11 trade places - the warp and conf[0] do not notice, conf[1..3] do
    swapped = hw_.clone()
    swapped[[3, 5]] = hw_[[5, 3]]
    warp, conf = host.refiner_head(z, swapped, hb_, pw, pc)
    fw, fc = R.violations(warp.numpy(), rw, bw)[1], R.violations(conf.numpy(), rc, bc)[1]
    print(f"head rows 3 and 5 swapped: warp {fw:.3g} x the bound, conf {fc:.3g} x")
    assert fw <= 1.0 and fc > 1e3
    # prev_dim 1 treated as channel 3
    d1 = R.case(shape, 1)
    rw, bw, rc, bc, dd = d1["ref"]
    wrong = dd.copy()
    wrong[..., 3] += d1["prev_conf"][..., 0]
    fc = R.violations(wrong, rc, bc)[1]
    warp, conf = run(host, d1, False)
    print(f"prev_dim 1 added to channel 3 instead of 0: conf {fc:.3g} x the bound; the twin {R.violations(conf, rc, bc)[1]:.4f} x")
    assert fc > 1e3 and R.violations(conf, rc, bc)[0] == 0


EXACT = [-200.0, -100.0, 0.0, 19.999, 20.0, 20.0001, 80.0, float("inf"), float("-inf"), float("nan")]


def exact_call(ctx, values, prev_dim, prev_value=0.0, device="cpu", bias=0.0):
    """C = 1, all six weights 1, bias 0 (-0 where the sign of a zero is to survive fmaf(1, -0, bias)): a[o] = z for every output.  One row of
    len(values) pixels; (warp, conf) as NumPy."""
    n = len(values)
    z = torch.tensor(values, dtype=torch.float32, device=device).reshape(1, 1, 1, n)
    head_w, head_b = torch.ones(6, 1, device=device), torch.full((6,), bias, device=device)
    pw = torch.zeros(1, 1, n, 2, device=device)
    pc = None if prev_dim == 0 else torch.full((1, 1, n, prev_dim), prev_value, device=device)
    warp, conf = ctx.refiner_head(z, head_w, head_b, pw, pc)
    return warp.cpu().numpy()[0, 0], conf.cpu().numpy()[0, 0]


def exact_expected(values):
    """(warp.x, l00 = l11, per value) from the f64 reference, rounded where the specification rounds."""
    v = np.asarray(values, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        sp = R.softplus64(v).astype(np.float32)
        l = (sp + np.float32(1e-6)).astype(np.float32)
    return v, l


def check_exact(warp, conf, values, prev_dim):
    v, l = exact_expected(values)
    n = len(values)
    with np.errstate(invalid="ignore", over="ignore"):
        want_conf = np.stack([v, (l * l).astype(np.float32), (l * v).astype(np.float32), ((v * v).astype(np.float32) + (l * l).astype(np.float32))], -1)
        want_warp = np.stack([v / np.float32(4.0 * n), v / np.float32(4.0)], -1).astype(np.float32)
    with np.errstate(invalid="ignore"):
        want_warp = (np.float32(0.0) + want_warp).astype(np.float32)
        if prev_dim:
            want_conf = (np.float32(0.0) + want_conf).astype(np.float32)
    for i, value in enumerate(values):
        nan = np.isnan(value)
        assert np.isnan(warp[i]).all() == nan and np.isnan(conf[i]).all() == nan, (value, warp[i], conf[i])      # a NaN in exactly the pixels that read it
        if nan:
            continue
        # conf[1..3] pass through the library's exp and log1p: one f32 ulp of l (tests/refiner_head_ref.py), exact where softplus is the identity
        assert np.array_equal(warp[i], want_warp[i]) and conf[i, 0] == want_conf[i, 0], (value, warp[i], conf[i])
        tol = 0.0 if (value > 20.0 or np.isinf(value)) else 2.0 ** -21
        for k in (1, 2, 3):
            a, b = float(conf[i, k]), float(want_conf[i, k])
            assert a == b or abs(a - b) <= tol * abs(b), (value, k, a, b)
    return want_conf


@pytest.mark.parametrize("prev_dim", [0, 1, 4])
def test_exact_cases(host, prev_dim):
    warp, conf = exact_call(host, EXACT, prev_dim)
    check_exact(warp, conf, EXACT, prev_dim)
    by = dict(zip(EXACT, conf))
    # the threshold side is exact: 20.0 is NOT above the threshold and goes through log1p(exp(.)), 20.0001 is and passes as it is
    l_at = np.float32(np.float32(np.log1p(np.exp(20.0))) + np.float32(1e-6))
    l_above = np.float32(np.float32(20.0001) + np.float32(1e-6))
    assert by[20.0][1] == np.float32(l_at * l_at) and by[20.0001][1] == np.float32(l_above * l_above)
    assert by[80.0][1] == np.float32(np.float32(80.0 + 1e-6) ** 2) and by[float("inf")][1] == np.inf
    assert by[float("-inf")][1] == np.float32(np.float32(1e-6) * np.float32(1e-6)) and by[float("-inf")][0] == -np.inf
    assert by[-200.0][1] == by[float("-inf")][1]                                  # exp(-200) is below half an ulp of 1e-6


def test_signed_zero(host):
    """prev_dim 0 leaves the bits of d untouched: a[2] = -0 stays -0.  With a previous confidence the zero padding is ADDED: -0 + +0 = +0."""
    for prev_dim, prev_value, negative in ((0, 0.0, True), (1, 0.0, False), (4, 0.0, False), (4, -0.0, True), (1, -0.0, True)):
        warp, conf = exact_call(host, [-0.0], prev_dim, prev_value, bias=-0.0)
        assert conf[0, 0] == 0.0 and bool(np.signbit(conf[0, 0])) == negative, (prev_dim, prev_value, conf[0])
        assert warp[0, 0] == 0.0 and not np.signbit(warp[0, 0])                    # prev_warp is +0: +0 + -0 = +0
    # channels 1..3 with prev_dim 1 are padded with +0 whatever the sign of the channel-0 value: l00 l10 = l00 * -0 = -0, then +0 + -0 = +0
    for prev_dim, negative in ((0, True), (1, False)):
        _, conf = exact_call(host, [-0.0], prev_dim, -0.0, bias=-0.0)
        assert conf[0, 2] == 0.0 and bool(np.signbit(conf[0, 2])) == negative, (prev_dim, conf[0])


def test_the_bits_do_not_depend_on_the_thread_count():
    outs = []
    for threads in (1, 8):
        ctx = hb.HostDensifier(threads)
        try:
            for shape, f32, pd, planar in (((2, 32, 7, 9), False, 4, True), ((1, 33, 9, 9), True, 1, False), ((1, 32, 3, 131), False, 0, False)):
                w, c = run(ctx, R.case(shape, pd), f32, planar)
                outs.append((threads, w.copy(), c.copy()))
        finally:
            ctx.close()
    half = len(outs) // 2
    for (_, w1, c1), (_, w8, c8) in zip(outs[:half], outs[half:]):
        assert np.array_equal(w1.view(np.uint32), w8.view(np.uint32)) and np.array_equal(c1.view(np.uint32), c8.view(np.uint32))


def test_python_side_checks(host):
    d = R.case((1, 3, 4, 5), 4)
    z, hw_, hb_, pw, pc = R.tensors(d, False)
    with pytest.raises(ValueError, match="bfloat16 or float32"):
        host.refiner_head(z.to(torch.float16), hw_, hb_, pw, pc)
    with pytest.raises(ValueError, match="head_w"):
        host.refiner_head(z, hw_[:, :2], hb_, pw, pc)
    with pytest.raises(ValueError, match="head_b"):
        host.refiner_head(z, hw_, hb_.double(), pw, pc)
    with pytest.raises(ValueError, match="prev_warp"):
        host.refiner_head(z, hw_, hb_, pw.double(), pc)
    with pytest.raises(ValueError, match="prev_conf"):
        host.refiner_head(z, hw_, hb_, pw, pc[:, :2])
    with pytest.raises(hb.HipBackendError, match="prev_dim must be 0, 1 or 4"):
        host.refiner_head(z, hw_, hb_, pw, pc[..., :2])
    with pytest.raises(hb.HipBackendError, match="refine_init must be finite and > 0"):
        host.refiner_head(z, hw_, hb_, pw, pc, refine_init=0.0)
    # a z that is not contiguous NCHW is refused, not copied: the call exists to read z once
    zt = z.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert not zt.is_contiguous()
    with pytest.raises(ValueError, match="z must be contiguous NCHW"):
        host.refiner_head(zt, hw_, hb_, pw, pc)
    with pytest.raises(ValueError, match="z must be contiguous NCHW"):
        host.refiner_head(z.to(memory_format=torch.channels_last), hw_, hb_, pw, pc)
