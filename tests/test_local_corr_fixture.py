"""tests/golden/g14_local_corr.npz: upstream's own local correlation (``native_torch_local_corr``, the grid_sample formulation, recorded in the
development container by tests/golden/make_local_corr_fixture.py) against the yardstick of tests/local_corr_ref.py - (a) upstream's outputs
satisfy the derived bound, so the bound does not reject the reference; (b) the CPU twin, called through the model-facing shim with the tensors
``romav2.local_correlation.local_corr_wrapper`` builds, satisfies it too and lies within twice the bound of upstream's values."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from local_corr_ref import reference_numpy, violations
from lichtfeld_densification_plugin_amd.core.local_corr import LocalCorr


def wrapper_tensors(g, name):
    """What the model's wrapper hands to ``local_corr.local_corr``: the (2r + 1)^2 window offsets - x from a linspace over +-2r / w, y over
    +-2r / h, rows first - added to the warp; feature0 as (B, N, C) divided by sqrt(C); feature1 channel-last.  Both features are VIEWS of
    channel-first memory, as they are in the model."""
    f0, f1, warp = (torch.from_numpy(g[f"{name}_{k}"]) for k in ("feature0", "feature1", "warp"))
    r = int(g[name + "_radius"])
    B, C, h, w = f0.shape
    side = 2 * r + 1
    oy = torch.linspace(-2 * r / h, 2 * r / h, side).view(side, 1).expand(side, side)
    ox = torch.linspace(-2 * r / w, 2 * r / w, side).view(1, side).expand(side, side)
    window = torch.stack([ox, oy], dim=-1).reshape(1, side * side, 2)
    warp_k = (warp[..., None, :] + window[:, None, None]).reshape(B, h * w, side * side, 2)
    a = f0.reshape(B, C, h * w).permute(0, 2, 1).float() / (C ** 0.5)
    bf = f1.permute(0, 2, 3, 1).clone().detach().float()
    upstream = torch.from_numpy(g[name + "_corr"]).reshape(B, side * side, h * w).permute(0, 2, 1)      # (B, N, K)
    return a, bf, warp_k.clone().detach(), upstream.numpy().astype(np.float64)


@pytest.fixture(scope="module")
def g14():
    return load_golden("g14_local_corr.npz")


@pytest.mark.parametrize("name", ["p4", "p2"])
def test_upstreams_recorded_outputs_satisfy_the_bound(g14, name):
    a, bf, warp_k, upstream = wrapper_tensors(g14, name)
    ref, bound = reference_numpy(a.numpy(), bf.numpy(), warp_k.numpy())
    bad, worst = violations(upstream, ref, bound)
    print(f"{name}: upstream uses at most {worst:.4f} of the bound; {int((bound == 0).sum())} of {bound.size} elements have bound 0")
    assert bad == 0 and worst < 1.0
    assert 0 < int((bound == 0).sum()) < bound.size


@pytest.mark.parametrize("name", ["p4", "p2"])
def test_the_twin_through_the_shim_satisfies_it_and_stays_within_twice_the_bound_of_upstream(g14, name):
    a, bf, warp_k, upstream = wrapper_tensors(g14, name)
    assert not a.is_contiguous() and not bf.is_contiguous()          # the permuted views the model produces
    shim = LocalCorr(host_threads=2)
    try:
        out = shim.local_corr(a, bf, warp_k, mode="bilinear", normalized_coords=True)
    finally:
        shim.close()
    assert out.shape == upstream.shape and out.dtype == torch.float32
    out = out.numpy().astype(np.float64)
    ref, bound = reference_numpy(a.numpy(), bf.numpy(), warp_k.numpy())
    bad, worst = violations(out, ref, bound)
    print(f"{name}: the twin uses at most {worst:.4f} of the bound")
    assert bad == 0
    assert (np.abs(out - upstream) <= 2.0 * bound).all()
    assert not out[bound == 0].any()
