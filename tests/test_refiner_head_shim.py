"""The model-facing side of the fused refiner head (core/refiner_head.py) on the CPU: recognition of the refiners by their
structure, installation of the fused forward and its removal (also when the body raises), every structural and call-time refusal, the cached
head weights and their rebuilding, the front half (what ``block1`` is given is bit-equal to the stand-in's own), the outputs against the f64
yardstick, the four combinations with the fused local correlation and the fused conv blocks, the knob's way through the matcher, the
configuration, the command line and the pipeline, and the verdicts recorded inside the real refiners (tests/golden/g22).  The model itself is
not importable here: the stand-in refiner below has the model's attribute names, and the three functions the shim looks up in the module
that defines the refiner's class - ``bhwc_grid_sample``, ``get_normalized_grid``, ``local_correlation`` - live in this module's namespace."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import lichtfeld_densification_plugin_amd as lfd
import refiner_block_ref as RB
import refiner_head_ref as R
from helpers import ROOT
from lichtfeld_densification_plugin_amd import densify, synthetic
from lichtfeld_densification_plugin_amd.core import matcher as matcher_mod
from lichtfeld_densification_plugin_amd.core import pipeline as pl
from lichtfeld_densification_plugin_amd.core.local_corr import LocalCorr
from lichtfeld_densification_plugin_amd.core.refiner_blocks import FusedRefinerBlocks
from lichtfeld_densification_plugin_amd.core.refiner_head import FusedRefinerHead, check_structure, is_refiner
from lichtfeld_densification_plugin_amd.core.types import EXPERIMENTAL_DEFAULTS

CALLS = types.SimpleNamespace(sample=0, grid=0, corr=0, fused_corr=0)
EXTENSION = types.SimpleNamespace(local_corr=None)          # what romav2.local_correlation.local_corr is in the model: None, or a shim
DEVICE = torch.device("cpu")                                 # the model keeps its device in a global too (tests/test_gpu_refiner_head.py changes it)


# ---- the three functions of the refiner's module, stand-ins of the same interface -----------------------------------------------------------

def bhwc_grid_sample(x, grid, mode="bilinear", align_corners=None):
    CALLS.sample += 1
    return F.grid_sample(x.permute(0, 3, 1, 2), grid, mode=mode, align_corners=align_corners).permute(0, 2, 3, 1)


def get_normalized_grid(B, H, W):
    CALLS.grid += 1
    ys, xs = torch.linspace(-1 + 1 / H, 1 - 1 / H, H, device=DEVICE), torch.linspace(-1 + 1 / W, 1 - 1 / W, W, device=DEVICE)
    return torch.stack(torch.broadcast_tensors(xs[None, None, :], ys[None, :, None]), dim=-1).expand(B, H, W, 2)


def local_correlation(feature0, feature1, local_radius, warp, scale_factor):
    """(B, K, H, W): feature0 against feature1 sampled on a (2 r + 1)^2 window around ``warp``; through EXTENSION.local_corr where there is one
    (the call the model's wrapper makes), else through grid_sample."""
    CALLS.corr += 1
    B, C, H, W = feature0.shape
    r = int(local_radius)
    steps = torch.arange(-r, r + 1, dtype=torch.float32, device=feature0.device)
    window = torch.stack(torch.broadcast_tensors((2.0 / W) * steps[None, :], (2.0 / H) * steps[:, None]), dim=-1).reshape(1, 1, 1, -1, 2)
    K = window.shape[3]
    at = warp[:, :, :, None, :] + window                                         # (B, H, W, K, 2)
    if EXTENSION.local_corr is not None:
        CALLS.fused_corr += 1
        out = EXTENSION.local_corr.local_corr(feature0.reshape(B, C, H * W).permute(0, 2, 1).float() / C ** 0.5,
                                              feature1.permute(0, 2, 3, 1).float().contiguous(), at.reshape(B, H * W, K, 2).contiguous(),
                                              mode="bilinear", normalized_coords=True)
        return out.permute(0, 2, 1).reshape(B, K, H, W)
    sampled = F.grid_sample(feature1, at.reshape(B, H, W * K, 2), mode="bilinear", padding_mode="zeros", align_corners=False).reshape(B, C, H, W, K)
    return (feature0[..., None] / C ** 0.5 * sampled).sum(dim=1).permute(0, 3, 1, 2)


# ---- a refiner with the model's attribute names ---------------------------------------------------------------------------------------------

class Cfg:
    def __init__(self, **kw):
        self.feat_dim, self.proj_dim, self.displacement_emb_dim, self.local_corr_radius = 6, 8, 7, 1         # hidden width 2 * 8 + 7 + 9 = 32
        self.warp_dim, self.confidence_dim, self.refine_init = 2, 4, 4.0
        self.channels_last, self.grid_sample_mode = False, "bilinear"
        self.__dict__.update(kw)


class StandInRefiner(nn.Module):
    def __init__(self, cfg, seed=22):
        super().__init__()
        self.cfg = cfg
        K = (2 * cfg.local_corr_radius + 1) ** 2 if cfg.local_corr_radius is not None else 0
        self.hidden_dim = C = 2 * cfg.proj_dim + cfg.displacement_emb_dim + K
        torch.manual_seed(seed)
        self.proj = nn.Linear(cfg.feat_dim, cfg.proj_dim)
        self.disp_emb = nn.Conv2d(2, cfg.displacement_emb_dim, 1, 1, 0)
        self.block1 = RB.stand_in_block(RB.case((1, C, 6, 6), C == 32, seed=1))
        self.hidden_blocks = nn.Sequential(RB.stand_in_block(RB.case((1, C, 6, 6), C == 32, seed=2)))
        self.warp_head = nn.Conv2d(C, cfg.warp_dim, 1, 1, 0)
        self.confidence_head = nn.Conv2d(C, cfg.confidence_dim, 1, 1, 0)

    def forward(self, *, f_A, f_B, prev_warp, prev_confidence, scale_factor):
        B, H, W, D = f_A.shape
        pa = self.proj(f_A.reshape(B, H * W, D).float()).reshape(B, H, W, -1)
        pb = self.proj(f_B.reshape(B, H * W, D).float()).reshape(B, H, W, -1)
        pb = bhwc_grid_sample(pb, prev_warp, mode=self.cfg.grid_sample_mode, align_corners=False)
        emb = self.disp_emb(scale_factor[None, :, None, None] * (prev_warp - get_normalized_grid(B, H, W)).permute(0, 3, 1, 2))
        a, b = pa.permute(0, 3, 1, 2), pb.permute(0, 3, 1, 2)
        d = torch.cat((a, b, emb), dim=1)
        if self.cfg.local_corr_radius is not None:
            d = torch.cat((d, local_correlation(a, b, local_radius=self.cfg.local_corr_radius, warp=prev_warp, scale_factor=scale_factor)), dim=1)
        z = self.hidden_blocks(self.block1(d))
        warp, confidence = R.torch_tail(z, self.warp_head, self.confidence_head, prev_warp, prev_confidence, self.cfg.refine_init)
        return {"warp": warp, "confidence": confidence}


def make_refiner(**cfg):
    return StandInRefiner(Cfg(**cfg)).eval().requires_grad_(False)


def model_with(*refiners):
    m = nn.Module()
    m.refiners = nn.ModuleDict({str(i): r for i, r in enumerate(refiners)})
    m.elsewhere = nn.Conv2d(3, 3, 1)
    return m.eval()


def inputs(prev_dim=4, B=2, H=5, W=7, feat=6, seed=3, planar=True):
    """The keyword arguments of a refiner call; the previous state as the model hands it over: permuted views of planar memory."""
    g = torch.Generator().manual_seed(seed)
    grid = get_normalized_grid(B, H, W).cpu()
    give = (lambda t: t.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)) if planar else (lambda t: t.contiguous())
    return dict(f_A=torch.randn(B, H, W, feat, generator=g), f_B=torch.randn(B, H, W, feat, generator=g),
                prev_warp=give(grid + 0.1 * torch.randn(B, H, W, 2, generator=g)),
                prev_confidence=None if prev_dim == 0 else give(torch.randn(B, H, W, prev_dim, generator=g)),
                scale_factor=torch.tensor([float(W), float(H)]))


class Taps:
    """what ``block1`` is given and what ``hidden_blocks`` returns, per forward"""

    def __init__(self, refiner):
        self.d, self.z = [], []
        self._hooks = [refiner.block1.register_forward_pre_hook(lambda m, args: self.d.append(args[0].clone())),
                       refiner.hidden_blocks.register_forward_hook(lambda m, args, out: self.z.append(out.clone()))]

    def remove(self):
        for h in self._hooks:
            h.remove()


def inside_the_bound(refiner, z, kw, out):
    """the outputs against the f64 evaluation of the tail from that same z"""
    C = refiner.hidden_dim
    n = R.to_numpy
    head_w = np.concatenate([n(refiner.warp_head.weight).reshape(2, C), n(refiner.confidence_head.weight).reshape(4, C)], 0)
    head_b = np.concatenate([(n(m.bias) if m.bias is not None else np.zeros(k, np.float32)) for m, k in ((refiner.warp_head, 2), (refiner.confidence_head, 4))])
    pc = kw["prev_confidence"]
    rw, bw, rc, bc, _ = R.reference(n(z), head_w, head_b, n(kw["prev_warp"]), None if pc is None else n(pc), refiner.cfg.refine_init)
    (bad_w, worst_w), (bad_c, worst_c) = R.violations(n(out["warp"]), rw, bw), R.violations(n(out["confidence"]), rc, bc)
    return bad_w + bad_c, max(worst_w, worst_c)


@pytest.fixture
def shim():
    s = FusedRefinerHead(host_threads=2)
    yield s
    s.close()
    assert not s._ctx


@pytest.fixture(autouse=True)
def _fresh_counters():
    for k in vars(CALLS):
        setattr(CALLS, k, 0)
    EXTENSION.local_corr = None
    yield
    EXTENSION.local_corr = None


# ---- finding, installing, restoring ---------------------------------------------------------------------------------------------------------

def test_refiners_are_found_by_structure_and_the_forward_is_installed_and_removed(shim):
    r0, r1 = make_refiner(), make_refiner(local_corr_radius=None, displacement_emb_dim=5)
    model = model_with(r0, r1)
    assert is_refiner(r0) and not is_refiner(model.elsewhere) and not is_refiner(r0.block1)
    assert shim.refiners(model) == [r0, r1] and check_structure(r0) == 32 and check_structure(r1) == 21
    with shim.installed(model):
        assert all("forward" in r.__dict__ for r in (r0, r1)) and "forward" not in model.elsewhere.__dict__ and "forward" not in r0.block1.__dict__
        out = r0(**inputs())
    assert all("forward" not in r.__dict__ for r in (r0, r1))
    assert set(out) == {"warp", "confidence"} and out["warp"].shape == (2, 5, 7, 2) and out["confidence"].shape == (2, 5, 7, 4)
    with shim.installed(model), pytest.raises(TypeError):
        r0(inputs()["f_A"])                                    # the model's signature: keywords only
    marker = lambda **kw: kw                                   # noqa: E731
    r1.forward = marker                                        # an instance-level forward somebody else put there is what comes back
    with shim.installed(model):
        assert r1.__dict__["forward"] is not marker
    assert r1.__dict__["forward"] is marker
    # a width the shim was told to leave alone gets nothing
    skipping = FusedRefinerHead(host_threads=1, skip_widths=(32,))
    with skipping.installed(model):
        assert "forward" not in r0.__dict__ and r1.__dict__["forward"] is not marker
    skipping.close()


def test_the_forward_is_removed_when_the_body_raises(shim):
    r0, bad = make_refiner(), make_refiner()
    with pytest.raises(RuntimeError, match="the model failed"):
        with shim.installed(model_with(r0)):
            assert "forward" in r0.__dict__
            raise RuntimeError("the model failed")
    assert "forward" not in r0.__dict__
    bad.cfg.grid_sample_mode = "bicubic"                       # ... and when a later refiner cannot be served, the earlier ones are as they were
    with pytest.raises(NotImplementedError, match="bicubic"):
        with shim.installed(model_with(r0, bad)):
            raise AssertionError("not reached")
    assert "forward" not in r0.__dict__ and "forward" not in bad.__dict__


def test_every_structural_refusal_names_what_was_found(shim):
    for change, piece in [(dict(warp_head=nn.Conv2d(32, 2, 3, padding=1)), "warp head.*kernel_size=\\(3, 3\\)"),
                          (dict(warp_head=nn.Conv2d(32, 3, 1)), "warp head.*32, 3"),
                          (dict(warp_head=nn.Linear(32, 2)), "warp head.*Linear"),
                          (dict(warp_head=nn.Conv2d(32, 2, 1, stride=2)), "warp head.*stride=\\(2, 2\\)"),
                          (dict(confidence_head=nn.Conv2d(32, 1, 1)), "confidence head.*32, 1"),
                          (dict(confidence_head=nn.Conv2d(32, 4, 1, groups=4)), "confidence head.*groups=4"),
                          (dict(confidence_head=nn.Conv2d(16, 4, 1)), "confidence head.*16, 4"),
                          (dict(confidence_head=nn.Conv2d(32, 4, 1, padding=1)), "confidence head.*padding=\\(1, 1\\)"),
                          (dict(confidence_head=nn.Conv2d(32, 4, 1).double()), "float32 head parameters only, found torch.float64")]:
        r = make_refiner()
        for name, module in change.items():
            setattr(r, name, module.eval())
        for attempt in (lambda: check_structure(r), lambda: shim.forward(r, **inputs()), lambda: shim.refiners(model_with(r))):
            with pytest.raises(NotImplementedError, match=piece):
                attempt()
    for cfg, piece in [(dict(warp_dim=3), "warp_dim 3"), (dict(confidence_dim=1), "confidence_dim 1"), (dict(grid_sample_mode="bicubic"), "'bicubic'"),
                       (dict(channels_last=True), "channels_last True")]:
        r = make_refiner()
        r.cfg.__dict__.update(cfg)
        with pytest.raises(NotImplementedError, match=piece):
            check_structure(r)
        with pytest.raises(NotImplementedError, match=piece):
            with shim.installed(model_with(r)):
                raise AssertionError("not reached")


def test_every_call_time_refusal_names_what_was_found(shim):
    r, kw = make_refiner(), inputs()
    r.train()
    with pytest.raises(NotImplementedError, match="training mode"):
        shim.forward(r, **kw)
    r.eval()
    for name in ("f_A", "prev_warp", "prev_confidence"):
        with pytest.raises(NotImplementedError, match=f"no backward pass, {name} requires grad"):
            shim.forward(r, **dict(kw, **{name: kw[name].clone().requires_grad_(True)}))
    with torch.autocast(device_type="cpu", dtype=torch.bfloat16), pytest.raises(NotImplementedError, match="autocast is enabled around the refiner"):
        shim.forward(r, **kw)
    with pytest.raises(NotImplementedError, match="1 or 4 channels only, got 2"):
        shim.forward(r, **dict(kw, prev_confidence=kw["prev_confidence"][..., :2]))
    with pytest.raises(NotImplementedError, match="float32 prev_warp only, got torch.float64"):
        shim.forward(r, **dict(kw, prev_warp=kw["prev_warp"].double()))
    with pytest.raises(NotImplementedError, match="float32 prev_confidence only, got torch.bfloat16"):
        shim.forward(r, **dict(kw, prev_confidence=kw["prev_confidence"].bfloat16()))
    half = make_refiner()
    half.hidden_blocks = nn.Sequential(half.hidden_blocks[0], _Cast(torch.float16))
    with pytest.raises(NotImplementedError, match="bfloat16 or float32 activation only, the blocks returned torch.float16"):
        shim.forward(half, **kw)
    last = make_refiner()
    last.hidden_blocks = nn.Sequential(last.hidden_blocks[0], _ChannelsLast())
    with pytest.raises(NotImplementedError, match="contiguous NCHW activation only, the blocks returned strides"):
        shim.forward(last, **kw)
    grad = make_refiner()
    grad.proj.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="the activation requires grad"):
        shim.forward(grad, **kw)
    with torch.no_grad():
        assert shim.forward(grad, **kw)["warp"].shape == (2, 5, 7, 2)            # ... and under no_grad it is served
    assert shim.forward(r, **kw)["confidence"].shape == (2, 5, 7, 4)


class _ChannelsLast(nn.Module):
    def forward(self, x):
        return x.to(memory_format=torch.channels_last)


class _Cast(nn.Module):
    def __init__(self, dtype):
        super().__init__()
        self.dtype = dtype

    def forward(self, x):
        return x.to(self.dtype)


# ---- the numbers ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prev_dim", [0, 1, 4])
@pytest.mark.parametrize("radius", [1, None], ids=["corr", "nocorr"])
def test_the_front_half_is_the_models_and_the_outputs_are_inside_the_bound(shim, prev_dim, radius):
    r = make_refiner(local_corr_radius=radius, displacement_emb_dim=7 if radius else 16)
    assert r.hidden_dim == 32
    kw = inputs(prev_dim)
    taps = Taps(r)
    count = lambda: np.array([CALLS.sample, CALLS.grid, CALLS.corr])          # noqa: E731
    start = count()
    plain = r(**kw)
    own = count() - start
    with shim.installed(model_with(r)):
        fused = r(**kw)
    taps.remove()
    assert list(own) == [1, 1, 1 if radius else 0] and list(count() - start) == list(2 * own)      # looked up in this module, called as often
    assert torch.equal(taps.d[0], taps.d[1]) and torch.equal(taps.z[0], taps.z[1]) and taps.z[1].dtype == torch.bfloat16
    bad, worst = inside_the_bound(r, taps.z[1], kw, fused)
    theirs = inside_the_bound(r, taps.z[0], kw, plain)[1]
    print(f"prev_dim {prev_dim}, radius {radius}: fused worst |out - ref| / bound = {worst:.4f} ({bad} outside); the refiner's own tail: {theirs:.4f}; "
          f"max |fused - own| warp {float((fused['warp'] - plain['warp']).abs().max()):.2e}, "
          f"confidence {float((fused['confidence'] - plain['confidence']).abs().max()):.2e}")
    assert bad == 0
    assert fused["warp"].dtype == fused["confidence"].dtype == torch.float32 and fused["warp"].is_contiguous() and fused["confidence"].is_contiguous()


def test_an_f32_activation_and_a_head_without_bias(shim):
    r = make_refiner()
    r.block1.enable_amp = False
    r.hidden_blocks[0].enable_amp = False
    r.warp_head = nn.Conv2d(32, 2, 1, bias=False).eval().requires_grad_(False)
    kw = inputs(4, planar=False)
    taps = Taps(r)
    with shim.installed(model_with(r)):
        fused = r(**kw)
    taps.remove()
    assert taps.z[0].dtype == torch.float32 and torch.equal(shim._heads[(id(r), "cpu")][1][1][:2], torch.zeros(2))
    assert inside_the_bound(r, taps.z[0], kw, fused)[0] == 0


def test_head_weights_are_concatenated_once_and_again_after_a_change(shim):
    r, kw = make_refiner(), inputs()
    first = shim.forward(r, **kw)
    kept = shim._heads[(id(r), "cpu")][1]
    assert torch.equal(kept[0][:2], r.warp_head.weight.reshape(2, 32)) and torch.equal(kept[0][2:], r.confidence_head.weight.reshape(4, 32))
    assert torch.equal(kept[1], torch.cat([r.warp_head.bias, r.confidence_head.bias]))
    second = shim.forward(r, **kw)
    assert shim._heads[(id(r), "cpu")][1] is kept and torch.equal(first["warp"], second["warp"])                   # cached
    with torch.no_grad():
        r.warp_head.weight.mul_(2.0)                           # in place: same storage, new version
    third = shim.forward(r, **kw)
    assert shim._heads[(id(r), "cpu")][1] is not kept
    assert torch.allclose(third["warp"] - kw["prev_warp"], 2.0 * (first["warp"] - kw["prev_warp"]) - r.warp_head.bias / (4.0 * torch.tensor((7.0, 5.0))),
                          atol=1e-6)
    assert torch.equal(third["confidence"], first["confidence"])
    kept = shim._heads[(id(r), "cpu")][1]
    r.confidence_head.bias = nn.Parameter(torch.zeros(4), requires_grad=False)      # replaced: new storage
    fourth = shim.forward(r, **kw)
    assert shim._heads[(id(r), "cpu")][1] is not kept and torch.equal(shim._heads[(id(r), "cpu")][1][1][2:], torch.zeros(4))
    assert not torch.equal(fourth["confidence"], third["confidence"]) and torch.equal(fourth["warp"], third["warp"])


@pytest.mark.parametrize("corr", [False, True], ids=["torch-corr", "fused-corr"])
@pytest.mark.parametrize("blocks", [False, True], ids=["torch-blocks", "fused-blocks"])
def test_the_other_two_shims_keep_working_beneath_it(shim, corr, blocks, monkeypatch):
    lc = types.ModuleType("romav2.local_correlation")
    lc.local_corr = None
    monkeypatch.setitem(sys.modules, "romav2.local_correlation", lc)
    r, kw = make_refiner(), inputs(4)
    model = model_with(r)
    corr_shim, block_shim = (LocalCorr(host_threads=1) if corr else None), (FusedRefinerBlocks(host_threads=1) if blocks else None)
    block_calls = []
    if blocks:
        inner = block_shim.forward
        block_shim.forward = lambda block, x: (block_calls.append(int(x.shape[1])), inner(block, x))[1]
    taps = Taps(r)
    try:
        with matcher_mod._local_corr_installed(corr_shim), matcher_mod._refiner_blocks_installed(block_shim, model):
            EXTENSION.local_corr = lc.local_corr                                    # what the model's wrapper would look up
            plain = r(**kw)
            with matcher_mod._refiner_head_installed(shim, model):
                fused = r(**kw)
            assert "forward" not in r.__dict__ and ("forward" in r.block1.__dict__) == blocks
    finally:
        taps.remove()
        for s in (corr_shim, block_shim):
            if s is not None:
                s.close()
    assert CALLS.corr == 2 and CALLS.fused_corr == (2 if corr else 0) and block_calls == ([32] * 4 if blocks else [])
    assert torch.equal(taps.d[0], taps.d[1]) and torch.equal(taps.z[0], taps.z[1])
    assert inside_the_bound(r, taps.z[1], kw, fused)[0] == 0
    assert float((fused["warp"] - plain["warp"]).abs().max()) < 1e-5 and float((fused["confidence"] - plain["confidence"]).abs().max()) < 1e-4


# ---- the knob: matcher, configuration, command line, pipeline ------------------------------------------------------------------------------

@pytest.fixture
def stand_in(monkeypatch):
    """``romav2`` with a RoMaV2 of the interface core/matcher.py uses whose ``refiners`` hold one stand-in refiner; ``match_from_features``
    records whether the refiner carries an instance-level forward while the model runs, and runs it."""
    seen = types.SimpleNamespace(installed=[], outs=[], fail=False, kw=inputs(1))

    class RoMaV2(nn.Module):
        class Cfg:
            def __init__(self, **kw):
                pass

        def __init__(self, cfg):
            super().__init__()
            self.f = nn.Identity()
            self.refiners = nn.ModuleDict({"1": make_refiner()})
            self.H_lr = self.W_lr = 16
            self.H_hr = self.W_hr = None
            self.bidirectional = False

        def apply_setting(self, setting):
            pass

        def _load_image(self, im):
            return im.float()

        def match_from_features(self, f_list_A, img_A_lr, imB, img_A_hr):
            refiner = self.refiners["1"]
            seen.installed.append("forward" in refiner.__dict__)
            if seen.fail:
                raise RuntimeError("the model failed")
            seen.outs.append(refiner(**seen.kw))
            return {"warp_AB": torch.zeros(1, 16, 16, 2), "overlap_AB": torch.zeros(1, 16, 16, 1)}

    pkg = types.ModuleType("romav2")
    pkg.RoMaV2 = RoMaV2
    monkeypatch.setitem(sys.modules, "romav2", pkg)
    return seen


def _image():
    return torch.zeros(20, 24, 3, dtype=torch.uint8)


def test_the_matcher_installs_the_shim_for_the_duration_of_a_match(stand_in):
    seen = stand_in
    m = matcher_mod.RomaMatcher(device="cpu", fused_refiner_head=True)
    assert m.supports_fused_refiner_head and m.fused_refiner_head and not m.fused_local_corr and not m.fused_refiner_blocks
    refiner = m.model.refiners["1"]
    assert "forward" not in refiner.__dict__                   # creating the matcher installs nothing
    assert len(m.match_grids_batch(_image(), [_image(), _image()])) == 2
    assert seen.installed == [True, True] and "forward" not in refiner.__dict__
    with torch.no_grad():
        own = refiner(**seen.kw)
    assert float((seen.outs[0]["warp"] - own["warp"]).abs().max()) < 1e-5 and float((seen.outs[0]["confidence"] - own["confidence"]).abs().max()) < 1e-4
    shim = m._refiner_head
    assert shim._ctx                                                                  # the model's call reached the twin
    seen.fail = True
    with pytest.raises(RuntimeError, match="the model failed"):
        m.match_grids_batch(_image(), [_image()])
    assert seen.installed[-1] is True and "forward" not in refiner.__dict__          # restored when the model raises
    seen.fail = False
    m.set_fused_refiner_head(False)
    assert not m.fused_refiner_head and not shim._ctx                                 # switched off: its contexts are closed
    m.match_grids_batch(_image(), [_image()])
    assert seen.installed[-1] is False
    m.set_fused_refiner_head(True)
    shim = m._refiner_head
    m.match_grids_batch(_image(), [_image()])
    assert seen.installed[-1] is True and shim._ctx
    m.close()
    assert not shim._ctx                                                              # closed with the matcher


def test_with_the_knob_off_nothing_new_is_imported_or_touched(stand_in, monkeypatch):
    seen = stand_in
    monkeypatch.delitem(sys.modules, "lichtfeld_densification_plugin_amd.core.refiner_head", raising=False)
    m = matcher_mod.RomaMatcher(device="cpu")
    assert not m.fused_refiner_head
    refiner = m.model.refiners["1"]
    with torch.no_grad():
        want = refiner(**seen.kw)
    m.match_grids_batch(_image(), [_image()])
    assert seen.installed == [False]
    assert torch.equal(seen.outs[0]["warp"], want["warp"]) and torch.equal(seen.outs[0]["confidence"], want["confidence"])   # its own forward, bit for bit
    assert "lichtfeld_densification_plugin_amd.core.refiner_head" not in sys.modules
    m.close()


def test_the_knob_is_experimental_off_by_default_and_a_bool():
    assert EXPERIMENTAL_DEFAULTS["fused_refiner_head"] is False
    assert lfd.DensePipelineConfig(output_path="a.ply").exp("fused_refiner_head") is False
    for backend in ("device", "host"):
        assert lfd.DensePipelineConfig(output_path="a.ply", backend=backend, experimental={"fused_refiner_head": True}).problem() is None
    for wrong in (1, 0, "yes", None, 1.0):
        with pytest.raises(ValueError, match=r"experimental\['fused_refiner_head'\] must be True or False"):
            lfd.DensePipelineConfig(output_path="a.ply", experimental={"fused_refiner_head": wrong})


def test_the_command_line_flag():
    ap = densify.build_argparser()
    assert densify._experimental_from_args(ap.parse_args(["--scene_root", "s"])) == {}
    assert densify._experimental_from_args(ap.parse_args(["--scene_root", "s", "--fused_refiner_head"])) == {"fused_refiner_head": True}


class _PlainMatcher:
    sample_thresh = 0.9
    w_resized = h_resized = 32

    def match_grids_batch(self, imA, imB_list):
        raise AssertionError("the run must be refused before the first match")

    def close(self):
        pass


def _config(tmp_path, on):
    return lfd.DensePipelineConfig(output_path=os.path.join(str(tmp_path), "o.ply"), nns_per_ref=1, viz_interval=0, backend="host",
                                   experimental={"fused_refiner_head": on})


def test_an_injected_matcher_without_the_capability_refuses_the_knob(tmp_path):
    cams = synthetic.ring_cameras(2, seed=0)
    with pytest.raises(ValueError, match="supports_fused_refiner_head"):
        pl.run_dense_pipeline(cams, [0, 1], np.array([[1], [0]]), _config(tmp_path, True), matcher=_PlainMatcher())


def test_an_injected_matcher_with_the_capability_receives_the_knob(tmp_path):
    calls = []

    class Capable(_PlainMatcher):
        supports_fused_refiner_head = True

        def set_fused_refiner_head(self, on):
            calls.append(on)

        def match_grids_batch(self, imA, imB_list):
            raise RuntimeError("stop here")

    cams = synthetic.ring_cameras(2, seed=0)
    for on in (True, False):
        with pytest.raises(Exception):
            pl.run_dense_pipeline(cams, [0, 1], np.array([[1], [0]]), _config(tmp_path, on), matcher=Capable())
    assert calls == [True, False]


# ---- inside the real refiners: the recorded verdicts (tests/golden/check_refiner_head_contract.py) ------------------------------------------

def test_the_recorded_contract_inside_the_real_refiners():
    with open(os.path.join(ROOT, "tests", "golden", "g22_refiner_head_contract.json")) as fh:
        record = json.load(fh)
    assert sorted(record["refiners"]) == ["patch 1", "patch 2", "patch 4"]
    widths = {"patch 4": (512, 1), "patch 2": (128, 4), "patch 1": (32, 4)}
    for name, entry in record["refiners"].items():
        assert (entry["hidden_width"], entry["prev_confidence_channels"]) == widths[name]
        assert entry["block1_input_bit_equal"] is True and entry["z_bit_equal"] is True
        assert entry["fused_outside_bound"] == {"warp": 0, "confidence": 0}
        assert len(entry["prev_warp_strides"]) == 4                                 # handed over as bhwc_interpolate returns it (interleaved on the CPU)
        for key in ("warp", "confidence"):
            # a wiring error is orders of magnitude above the rounding of either tail
            assert entry["fused_vs_model"][key] <= 4.0 * (entry["fused_vs_f64"][key] + entry["model_vs_f64"][key]) + 1e-12
            assert entry["fused_vs_f64"][key] < 1e-5 * max(1.0, entry["magnitude"][key])
