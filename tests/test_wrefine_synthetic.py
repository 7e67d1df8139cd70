"""The synthetic side of the precision-weighted re-triangulation: ``synth_reference(noise_model=...)``, the planes a
``SyntheticMatcher`` hands out, and ``RomaMatcher``'s conversion of the model's precision to this package's pixel unit (on a stand-in model: the
real class is checked by tests/golden/check_precision_contract.py in the development container, tests/golden/g17_precision_contract.json)."""
import json
import math
import os
import types

import numpy as np
import pytest
import torch

from helpers import ROOT
from lichtfeld_densification_plugin_amd import synthetic as syn
from lichtfeld_densification_plugin_amd.core import matcher as mt

N_CAMS, MATCH, REF, K = 40, 512, 10, 3
bits = lambda t: t.contiguous().numpy().view(np.uint32 if t.dtype == torch.float32 else np.uint8)


def make(H, W, **kw):
    cams = syn.ring_cameras(N_CAMS)
    args = dict(noise_px=0.5, outlier_frac=0.05, cert_mode="tiefree", seed=0)
    args.update(kw)
    return cams, syn.synth_reference(cams, REF, syn.ring_neighbours(N_CAMS, REF, K), H, W, MATCH, MATCH, **args)


def residual_match_px(noisy, clean):
    """(k, H, W, 2) f64: observed minus noise-free, px of the match image."""
    return (noisy.warp[..., -2:].double() - clean.warp[..., -2:].double()) * 0.5 * (MATCH - 1)


def test_iid_is_the_default_and_hetero_draws_the_same_numbers():
    H, W = 48, 64
    _c, default = make(H, W)
    _c, iid = make(H, W, noise_model="iid")
    cams, het = make(H, W, noise_model="hetero")
    _c, clean = make(H, W, noise_px=0.0, outlier_frac=0.0)
    for name in ("warp", "cert", "image"):
        assert np.array_equal(bits(getattr(default, name)), bits(getattr(iid, name)))
    assert iid.precision is None and default.precision is None
    assert het.precision is not None and tuple(het.precision.shape) == (K, H, W, 3) and het.precision.dtype == torch.float32
    # no new use of the generator: certainty, image and the outlier cells are the iid call's, bit for bit
    assert np.array_equal(bits(het.cert), bits(iid.cert)) and np.array_equal(bits(het.image), bits(iid.image))
    r_iid, r_het = residual_match_px(iid, clean), residual_match_px(het, clean)
    outlier = r_iid.norm(dim=-1) > 2.0                                   # (match px: 8 sigma or more) 0.5 px noise never gets there; an outlier nearly always does
    assert 0.03 < float(outlier.double().mean()) < 0.07
    assert np.array_equal(bits(het.warp[..., -2:][outlier]), bits(iid.warp[..., -2:][outlier]))
    # ... and the SAME standard-normal draw, shaped: whitening the hetero residual with the planes gives the iid residual over noise_px
    q = het.precision.double()
    s00, s01, s11 = _inverse(q[..., 0], q[..., 1], q[..., 2])           # the covariance the planes state, its Cholesky factor L: r = L nz
    l00 = torch.sqrt(s00)
    l10 = s01 / l00
    l11 = torch.sqrt(s11 - l10 * l10)
    nz0 = r_het[..., 0] / l00
    nz1 = (r_het[..., 1] - l10 * nz0) / l11
    for j in range(K):
        sx, sy = cams[het.nbr_indices[j]].width / MATCH, cams[het.nbr_indices[j]].height / MATCH
        want0, want1 = r_iid[j, ..., 0] * sx / 0.5, r_iid[j, ..., 1] * sy / 0.5
        ok = ~outlier[j]
        assert float((nz0[j][ok] - want0[ok]).abs().max()) < 2e-3 and float((nz1[j][ok] - want1[ok]).abs().max()) < 2e-3


def _inverse(a, b, c):
    det = a * c - b * b
    return c / det, -b / det, a / det


def test_hetero_planes_are_the_covariance_of_the_noise():
    """Coarse bins of 16 x 16 cells (m = 256 samples each): with y = C^T r (Q = C C^T) white, the bin means of y0^2 and y1^2 are 1 within
    6 sqrt(2 / m), of y0 y1 0 within 6 / sqrt(m); and the standard deviations the planes state span [0.25, 2] camera px."""
    H = W = 128
    cams, het = make(H, W, noise_model="hetero", outlier_frac=0.0)
    _c, clean = make(H, W, noise_px=0.0, outlier_frac=0.0)
    r = residual_match_px(het, clean)
    q = het.precision.double()
    c00 = torch.sqrt(q[..., 0])
    c10 = q[..., 1] / c00
    c11 = torch.sqrt(q[..., 2] - c10 * c10)
    y0 = c00 * r[..., 0] + c10 * r[..., 1]
    y1 = c11 * r[..., 1]
    m = 256
    binned = lambda v: v.reshape(K, H // 16, 16, W // 16, 16).mean(dim=(2, 4))
    assert float((binned(y0 * y0) - 1.0).abs().max()) < 6.0 * math.sqrt(2.0 / m)
    assert float((binned(y1 * y1) - 1.0).abs().max()) < 6.0 * math.sqrt(2.0 / m)
    assert float(binned(y0 * y1).abs().max()) < 6.0 / math.sqrt(m)
    assert abs(float((y0 * y0 + y1 * y1).mean()) - 2.0) < 6.0 * 2.0 / math.sqrt(K * H * W)
    for j in range(K):
        sx, sy = cams[het.nbr_indices[j]].width / MATCH, cams[het.nbr_indices[j]].height / MATCH
        P = torch.stack([torch.stack([q[j, ..., 0] / (sx * sx), q[j, ..., 1] / (sx * sy)], -1),
                         torch.stack([q[j, ..., 1] / (sx * sy), q[j, ..., 2] / (sy * sy)], -1)], -2)
        sig = 1.0 / torch.sqrt(torch.linalg.eigvalsh(P))
        lo, hi = syn.HETERO_SIGMA_PX
        assert float(sig.min()) >= lo * (1 - 1e-5) and float(sig.max()) <= hi * (1 + 1e-5)
        assert float(sig.min()) < 0.3 and float(sig.max()) > 1.7                # spread over the range, log-uniformly: the median near its middle
        assert 0.5 < float(sig.median()) < 1.0
    with pytest.raises(ValueError, match="noise_model"):
        make(8, 8, noise_model="other")


def test_synthetic_matcher_hands_out_the_planes_only_when_asked():
    cams = syn.ring_cameras(8)
    nbrs = [1, 2, 7]
    for model in ("hetero", "iid"):
        m = syn.SyntheticMatcher(cams, setting="turbo", noise_model=model, cert_mode="tiefree")
        assert m.supports_precision is True
        plain = m.match_grids_batch(None, None, keys=(0, nbrs))
        assert all(len(t) == 2 for t in plain)
        m.set_precision(True)
        four = m.match_grids_batch(None, None, keys=(0, nbrs))
        assert all(len(t) == 4 and t[2] is None for t in four)
        for (w, c), t in zip(plain, four):
            assert torch.equal(w, t[0]) and torch.equal(c, t[1])
            assert tuple(t[3].shape) == (m.H, m.W, 3) and t[3].dtype == torch.float32 and t[3].is_contiguous()
        if model == "hetero":
            s = syn.synth_reference(cams, 0, nbrs, m.H, m.W, m.w_resized, m.h_resized, **m.kw)
            assert all(torch.equal(t[3], s.precision[j]) for j, t in enumerate(four))
        else:
            sx = cams[1].width / float(m.w_resized)
            assert float(four[0][3][3, 5, 0]) == pytest.approx(sx * sx / 0.25) and float(four[0][3][3, 5, 1]) == 0.0
        m.set_backward_warp(True)
        both = m.match_grids_batch(None, None, keys=(0, nbrs))
        assert all(len(t) == 4 and t[2] is not None and torch.equal(t[3], f[3]) for t, f in zip(both, four))
        m.precompute([0], np.array([[1, 2, 7]] + [[0, 0, 0]] * 7), 3)
        again = m.match_grids_batch(None, None, keys=(0, nbrs))
        assert all(torch.equal(a[3], f[3]) and torch.equal(a[0], f[0]) for a, f in zip(again, four))
        m.set_precision(False)
        assert all(len(t) == 3 for t in m.match_grids_batch(None, None, keys=(0, nbrs)))


def test_roma_matcher_converts_the_model_s_precision_to_match_pixels():
    assert mt.RomaMatcher.supports_precision is True
    m = object.__new__(mt.RomaMatcher)
    m.w_resized, m.h_resized = 640, 512
    for hr, stage in (((None, None), (640, 512)), ((960, 768), (960, 768))):
        m.model = types.SimpleNamespace(H_lr=512, W_lr=640, H_hr=hr[1], W_hr=hr[0])
        rx, ry = m.precision_scale()
        assert rx == 639 / stage[0] and ry == 511 / stage[1]
        P = torch.rand(5, 7, 2, 2, dtype=torch.float32) + 0.5
        P[..., 1, 0] = P[..., 0, 1]
        q = m._precision_plane(P)
        assert tuple(q.shape) == (5, 7, 3) and q.dtype == torch.float32 and q.is_contiguous()
        assert torch.equal(q[..., 0], P[..., 0, 0] / (rx * rx)) and torch.equal(q[..., 1], P[..., 0, 1] / (rx * ry))
        assert torch.equal(q[..., 2], P[..., 1, 1] / (ry * ry))
    m._precision = False
    m.set_precision(1)
    assert m.precision is True


def test_the_recorded_contract_with_the_real_model():
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "g17_precision_contract.json")))
    for setting in ("fast", "high"):
        e = rec[setting]["pairs_per_forward_1"]
        assert e["forward_outputs"].startswith("bit-identical") and e["plane"].endswith("bit-identical")
        assert e["positive_definite_share_plane"] >= e["positive_definite_share_model"] > 0.0
    assert rec["fast"]["pairs_per_forward_2"]["forward_outputs"].startswith("bit-identical")
