"""The CPU twin of the local correlation (lfd_local_corr_host, through HostDensifier.local_corr) against the f64 NumPy evaluation of
tests/local_corr_ref.py, under the derived bound |out - ref| <= (C + 10) u S + 2 delta T (and exact zeros where that is 0)."""
import numpy as np
import pytest
import torch

from local_corr_ref import model_case, reference_numpy, violations
from lichtfeld_densification_plugin_amd.core import hip_backend as hb


@pytest.fixture(scope="module")
def twin():
    d = hb.HostDensifier(4)
    yield d
    d.close()


def run(twin, A, Bf, warp):
    return twin.local_corr(torch.as_tensor(A), torch.as_tensor(Bf), torch.as_tensor(warp)).numpy()


def check(out, A, Bf, warp, label):
    ref, bound = reference_numpy(A, Bf, warp)
    bad, worst = violations(out.astype(np.float64), ref, bound)
    print(f"{label}: {out.size} elements, {int((bound == 0).sum())} with bound 0, worst |out - ref| / bound = {worst:.4f}, outside the bound: {bad}")
    assert bad == 0, (label, bad, worst)
    return ref, bound


# (B, C, h, w, r, H1, W1): the two model shapes scaled down, then every C with every K, H1 != W1, N != H1 * W1, B = 3
CASES = [(1, 192, 16, 16, 3, None, None), (1, 48, 32, 32, 1, None, None)]
CASES += [(3, C, 6, 5, r, 9, 7) for C in (1, 7, 48, 192) for r in (0, 1, 3)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%d_C%d_h%d_w%d_r%d_H%s_W%s" % c)
def test_twin_is_under_the_bound(twin, case):
    B, C, h, w, r, H1, W1 = case
    A, Bf, warp = model_case(B, C, h, w, r, seed=C * 100 + r, H1=H1, W1=W1)
    out = run(twin, A, Bf, warp)
    assert out.shape == (B, h * w, (2 * r + 1) ** 2) and out.dtype == np.float32
    _ref, bound = check(out, A, Bf, warp, str(case))
    assert 0 < int((bound == 0).sum()) < bound.size            # with sigma = 0.3 a share of the samples lies outside the map, not all


@pytest.mark.parametrize("C", [7, 48])
def test_strided_inputs_give_the_bits_of_their_contiguous_copies(twin, C):
    """What upstream's wrapper hands over: channel-first memory seen through permuted views."""
    A, Bf, warp = model_case(3, C, 6, 5, 1, seed=11, H1=9, W1=7)
    a_view = torch.as_tensor(np.ascontiguousarray(A.transpose(0, 2, 1))).permute(0, 2, 1)            # (B, N, C) over (B, C, N) memory
    bf_view = torch.as_tensor(np.ascontiguousarray(Bf.transpose(0, 3, 1, 2))).permute(0, 2, 3, 1)    # (B, H1, W1, C) over (B, C, H1, W1)
    assert not a_view.is_contiguous() and not bf_view.is_contiguous()
    out = twin.local_corr(a_view, bf_view, torch.as_tensor(warp)).numpy()
    assert np.array_equal(out.view(np.uint32), run(twin, A, Bf, warp).view(np.uint32))
    check(out, A, Bf, warp, f"strided C={C}")


def test_all_samples_outside_are_exact_zeros(twin):
    A, Bf, warp = model_case(2, 48, 5, 5, 1, seed=3)
    warp = (np.abs(warp) + 1.5).astype(np.float32) * np.where(np.arange(warp.shape[1]) % 2, 1, -1).reshape(1, -1, 1, 1).astype(np.float32)
    out = run(twin, A, Bf, warp)
    assert not out.any()
    _ref, bound = check(out, A, Bf, warp, "outside")
    assert not bound.any()


def test_texel_centres_and_the_edge_of_the_map(twin):
    """Coordinates exactly on texel centres (ix integer: one live weight of 1, three of 0) and exactly on the map's edge x = -1, 1 (half a texel
    outside the outermost centre: half of the blend is 'outside')."""
    H1, W1, C = 8, 4, 48                       # powers of two: the centres are exact in f32
    rng = np.random.RandomState(5)
    A = (rng.standard_normal((1, H1 * W1 + 4, C)) / np.sqrt(C)).astype(np.float32)
    Bf = rng.standard_normal((1, H1, W1, C)).astype(np.float32)
    cx = (np.arange(W1) + 0.5) * 2.0 / W1 - 1.0
    cy = (np.arange(H1) + 0.5) * 2.0 / H1 - 1.0
    pts = [(x, y) for y in cy for x in cx] + [(-1.0, -1.0), (1.0, 1.0), (-1.0, cy[3]), (cx[1], 1.0)]
    warp = np.asarray(pts, np.float32).reshape(1, -1, 1, 2)
    out = run(twin, A, Bf, warp)
    check(out, A, Bf, warp, "centres + edge")
    centre = np.einsum("nc,nc->n", A[0, :H1 * W1].astype(np.float64), Bf[0].reshape(-1, C).astype(np.float64))
    assert np.allclose(out[0, :H1 * W1, 0], centre, rtol=0, atol=1e-5)
    assert out[0, H1 * W1:, 0].all()           # the edge samples touch the map


def test_non_finite_and_huge_coordinates_contribute_zero_and_leave_the_rest_alone(twin):
    A, Bf, warp = model_case(2, 48, 6, 5, 1, seed=9, H1=9, W1=7, sigma=0.05)
    clean = run(twin, A, Bf, warp)
    dirty = warp.copy()
    flat = dirty.reshape(-1, 2)
    specials = [np.inf, -np.inf, np.nan, 1e30, -1e30, 3.4e38]
    hit = np.arange(0, flat.shape[0], 7)
    for j, s in enumerate(hit):
        flat[s, j % 2] = specials[j % len(specials)]
    out = run(twin, A, Bf, dirty)
    mask = np.zeros(flat.shape[0], bool)
    mask[hit] = True
    assert not out.reshape(-1)[mask].any() and np.isfinite(out).all()
    assert np.array_equal(out.reshape(-1)[~mask].view(np.uint32), clean.reshape(-1)[~mask].view(np.uint32))
    check(out, A, Bf, dirty, "non-finite")


def test_a_dead_texel_value_never_enters_the_sum(twin):
    """padding_mode='zeros' means the texel is not read into the sum: an inf at the map's border must not leak into a sample whose
    clamped tap lands on it with weight 0 ... and a sample wholly outside stays 0."""
    A, Bf, _ = model_case(1, 7, 2, 2, 0, seed=1, H1=3, W1=3)
    Bf[0, :, 0, :] = np.inf
    warp = np.asarray([[-1.6, 0.0], [1.0 - 1e-3, 0.0]], np.float32).reshape(1, 2, 1, 2).repeat(2, axis=1)[:, :4]
    out = run(twin, A, Bf, warp)
    assert out[0, 0, 0] == 0.0 and np.isfinite(out[0, 1, 0])


def test_negative_control_a_map_shifted_by_one_texel_fails_the_bound(twin):
    A, Bf, warp = model_case(1, 48, 20, 20, 1, seed=21)
    out = run(twin, A, np.roll(Bf, 1, axis=2), warp)
    ref, bound = reference_numpy(A, Bf, warp)
    bad, worst = violations(out.astype(np.float64), ref, bound)
    print(f"negative control: {bad} of {out.size} outside the bound, worst ratio {worst:.1f}")
    assert bad > out.size // 2 and worst > 1000.0


def test_wrong_shapes_dtypes_and_devices_are_refused(twin):
    A, Bf, warp = (torch.as_tensor(t) for t in model_case(1, 4, 3, 3, 0, seed=0))
    with pytest.raises(ValueError):
        twin.local_corr(A.double(), Bf, warp)
    with pytest.raises(ValueError):
        twin.local_corr(A, Bf[..., :3], warp)
    with pytest.raises(ValueError):
        twin.local_corr(A, Bf, warp[..., :1])
