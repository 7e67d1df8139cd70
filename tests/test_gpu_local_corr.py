"""The local-correlation kernel on the device (lfd_local_corr through HipDensifier.local_corr and the model-facing shim) against the f64
yardstick of tests/local_corr_ref.py under the derived bound, against the CPU twin, and for determinism, layout independence, safety with
non-finite coordinates and memory use."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from local_corr_ref import model_case, reference_numpy, reference_torch, violations
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from lichtfeld_densification_plugin_amd.core.local_corr import LocalCorr
from test_local_corr_fixture import wrapper_tensors
from test_local_corr_host import CASES as SMALL_CASES

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
# (B, C, h, w, r): the refiners' shapes at `fast` (patch 4, patch 2), a batch of three at `base`, and a non-square one
REAL_CASES = [(1, 192, 128, 128, 3), (1, 48, 256, 256, 1), (3, 192, 160, 160, 3), (1, 192, 96, 72, 3)]


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


def on_device(*arrays):
    return tuple(torch.as_tensor(a).to(DEV) for a in arrays)


def bits(t):
    return t.contiguous().view(torch.int32)


def test_the_torch_yardstick_is_the_numpy_one(dens):
    """reference_torch (used below where NumPy on one core would take minutes) against reference_numpy, the definition."""
    for case in SMALL_CASES[2:8]:
        B, C, h, w, r, H1, W1 = case
        A, Bf, warp = model_case(B, C, h, w, r, seed=5, H1=H1, W1=W1)
        ref_n, bound_n = reference_numpy(A, Bf, warp)
        ref_t, bound_t = reference_torch(*on_device(A, Bf, warp))
        assert np.allclose(ref_t.cpu().numpy(), ref_n, rtol=1e-12, atol=1e-13)
        assert np.allclose(bound_t.cpu().numpy(), bound_n, rtol=1e-12, atol=0.0)
        assert np.array_equal(bound_t.cpu().numpy() == 0, bound_n == 0)


@pytest.mark.parametrize("case", REAL_CASES, ids=lambda c: "B%d_C%d_h%d_w%d_r%d" % c)
def test_device_is_under_the_bound_at_the_real_shapes(dens, case):
    B, C, h, w, r = case
    A, Bf, warp = on_device(*model_case(B, C, h, w, r, seed=C + h))
    out = dens.local_corr(A, Bf, warp)
    assert out.shape == (B, h * w, (2 * r + 1) ** 2) and out.dtype == torch.float32 and out.device == DEV
    ref, bound = reference_torch(A, Bf, warp)
    bad, worst = violations(out.double(), ref, bound)
    zeros = int((bound == 0).sum())
    print(f"{case}: {out.numel()} elements, {zeros} with bound 0, worst |out - ref| / bound = {worst:.4f}, outside the bound: {bad}")
    assert bad == 0, (case, bad, worst)
    assert 0 < zeros < out.numel()                       # N(0, 0.3) puts a share of the samples outside the map


@pytest.mark.parametrize("case", SMALL_CASES, ids=lambda c: "B%d_C%d_h%d_w%d_r%d_H%s_W%s" % c)
def test_device_is_under_the_bound_and_agrees_with_the_twin_on_the_small_odd_cases(dens, twin, case):
    B, C, h, w, r, H1, W1 = case
    A, Bf, warp = model_case(B, C, h, w, r, seed=C * 100 + r, H1=H1, W1=W1)
    out = dens.local_corr(*on_device(A, Bf, warp)).cpu().numpy()
    ref, bound = reference_numpy(A, Bf, warp)
    bad, worst = violations(out.astype(np.float64), ref, bound)
    print(f"{case}: worst |out - ref| / bound = {worst:.4f}, outside the bound: {bad}")
    assert bad == 0, (case, bad, worst)
    host = twin.local_corr(torch.as_tensor(A), torch.as_tensor(Bf), torch.as_tensor(warp)).numpy()
    assert (np.abs(out.astype(np.float64) - host.astype(np.float64)) <= 2.0 * bound).all()
    assert np.array_equal(out == 0, host == 0)


@pytest.mark.parametrize("case", [(1, 192, 32, 32, 3), (2, 48, 64, 48, 1)], ids=lambda c: "B%d_C%d_h%d_w%d_r%d" % c)
def test_device_against_the_twin_at_model_like_shapes(dens, twin, case):
    B, C, h, w, r = case
    A, Bf, warp = model_case(B, C, h, w, r, seed=77)
    out = dens.local_corr(*on_device(A, Bf, warp)).cpu().numpy()
    host = twin.local_corr(torch.as_tensor(A), torch.as_tensor(Bf), torch.as_tensor(warp)).numpy()
    _ref, bound = reference_numpy(A, Bf, warp)
    assert (np.abs(out.astype(np.float64) - host.astype(np.float64)) <= 2.0 * bound).all()
    assert np.array_equal(out == 0, host == 0) and (out == 0).any() and (out != 0).any()


@pytest.mark.parametrize("case", [(1, 192, 64, 64, 3), (2, 48, 96, 80, 1)], ids=lambda c: "B%d_C%d_h%d_w%d_r%d" % c)
def test_the_lattice_form_gives_the_bits_of_the_general_loop(dens, case):
    """Where a pixel's K samples are a lattice of texels the vector kernel multiplies each shared texel once (csrc/lfd_corr.hip).  With the
    samples handed over in reverse order the test for that fails and every pixel takes the general loop: the same values in reverse, bit for
    bit - which form a pixel takes never shows."""
    B, C, h, w, r = case
    A, Bf, warp = model_case(B, C, h, w, r, seed=31, sigma=0.1)
    ref, bound = reference_numpy(A, Bf, warp)
    forward = dens.local_corr(*on_device(A, Bf, warp)).cpu().numpy()
    backward = np.ascontiguousarray(dens.local_corr(*on_device(A, Bf, np.ascontiguousarray(warp[:, :, ::-1]))).cpu().numpy()[:, :, ::-1])
    assert violations(forward.astype(np.float64), ref, bound)[0] == 0
    assert np.array_equal(forward.view(np.uint32), backward.view(np.uint32))


@pytest.mark.parametrize("C", [48, 192, 7])
def test_two_launches_give_the_same_bits_and_a_strided_input_those_of_its_contiguous_copy(dens, C):
    A, Bf, warp = on_device(*model_case(2, C, 40, 36, 1 if C == 48 else 3, seed=C))
    first = dens.local_corr(A, Bf, warp)
    assert torch.equal(bits(first), bits(dens.local_corr(A, Bf, warp)))
    a_view = A.permute(0, 2, 1).contiguous().permute(0, 2, 1)               # (B, N, C) over channel-first memory, as the model hands it over
    bf_view = Bf.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
    assert not a_view.is_contiguous() and not bf_view.is_contiguous()
    assert torch.equal(bits(first), bits(dens.local_corr(a_view, bf_view, warp)))
    assert torch.equal(bits(first), bits(dens.local_corr(A, bf_view, warp)))
    sliced = torch.cat([Bf, Bf], dim=3)[..., :C]                            # channels adjacent, rows twice as far apart
    assert not sliced.is_contiguous()
    assert torch.equal(bits(first), bits(dens.local_corr(A, sliced, warp)))


def test_non_finite_and_huge_coordinates_contribute_zero_and_leave_the_rest_alone(dens):
    """Run once.  No address is formed from an unclamped coordinate (csrc/lfd_corr.hpp: lfd_corr_taps)."""
    for C in (192, 7):                                                     # the vector kernel and the general one
        A, Bf, warp = model_case(2, C, 24, 20, 1, seed=9, sigma=0.05)
        clean = dens.local_corr(*on_device(A, Bf, warp)).cpu().numpy()
        dirty = warp.copy()
        flat = dirty.reshape(-1, 2)
        specials = [np.inf, -np.inf, np.nan, 1e30, -1e30, 3.4e38]
        hit = np.arange(0, flat.shape[0], 7)
        for j, s in enumerate(hit):
            flat[s, j % 2] = specials[j % len(specials)]
        out = dens.local_corr(*on_device(A, Bf, dirty)).cpu().numpy()
        mask = np.zeros(flat.shape[0], bool)
        mask[hit] = True
        assert not out.reshape(-1)[mask].any() and np.isfinite(out).all()
        assert np.array_equal(out.reshape(-1)[~mask].view(np.uint32), clean.reshape(-1)[~mask].view(np.uint32))
        ref, bound = reference_numpy(A, Bf, dirty)
        assert violations(out.astype(np.float64), ref, bound)[0] == 0


@pytest.mark.parametrize("name", ["p4", "p2"])
def test_the_recorded_upstream_case_through_the_shim_on_the_device(name):
    g14 = load_golden("g14_local_corr.npz")
    a, bf, warp_k, upstream = wrapper_tensors(g14, name)
    shim = LocalCorr()
    side = torch.cuda.Stream(DEV)
    try:
        out = shim.local_corr(a.to(DEV), bf.to(DEV), warp_k.to(DEV), mode="bilinear", normalized_coords=True)
        with torch.cuda.stream(side):                                       # the call follows torch's current stream
            side.wait_stream(torch.cuda.default_stream(DEV))
            again = shim.local_corr(a.to(DEV), bf.to(DEV), warp_k.to(DEV))
        side.synchronize()
    finally:
        shim.close()
    assert out.device == DEV and torch.equal(bits(out), bits(again))
    out = out.cpu().numpy().astype(np.float64)
    ref, bound = reference_numpy(a.numpy(), bf.numpy(), warp_k.numpy())
    bad, worst = violations(out, ref, bound)
    print(f"{name}: the device uses at most {worst:.4f} of the bound")
    assert bad == 0
    assert (np.abs(out - upstream) <= 2.0 * bound).all()


def test_a_fused_call_allocates_no_sampled_feature_tensor(dens):
    B, C, h, w, r = REAL_CASES[0]
    A, Bf, warp = on_device(*model_case(B, C, h, w, r, seed=1))
    dens.local_corr(A, Bf, warp)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated(DEV)
    torch.cuda.reset_peak_memory_stats(DEV)
    out = dens.local_corr(A, Bf, warp)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(DEV) - base
    inputs = 4 * (A.numel() + Bf.numel() + warp.numel())
    print(f"peak above the resident inputs: {peak / 2**20:.1f} MB (output {4 * out.numel() / 2**20:.1f} MB; a (C, h, w, K) temporary would be "
          f"{4 * C * h * w * (2 * r + 1) ** 2 / 2**20:.0f} MB)")
    assert base >= inputs                                 # the inputs were resident before the call: what it adds is the output, and no temporary
    assert peak <= 4 * out.numel() + 16 * 2**20
