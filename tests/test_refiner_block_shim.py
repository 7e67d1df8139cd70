"""The model-facing side of the fused refiner block (core/refiner_blocks.py) on the CPU: recognition of the blocks by their
structure, installation of the fused forward and its removal (also when the body raises), every refusal, re-folding after a parameter
changed, the fused forward against the f64 yardstick - torch's own bf16 sequence printed beside it -, the block's own 1x1 convolution for
widths other than 32, and the knob's way through the matcher, the configuration, the command line and the pipeline.  The model itself is not
importable here: tests/refiner_block_ref.py builds stand-in blocks with the attribute names of the model's."""
import os
import sys
import types

import numpy as np
import pytest
import torch
from torch import nn

import lichtfeld_densification_plugin_amd as lfd
import refiner_block_ref as R
from lichtfeld_densification_plugin_amd import densify, synthetic
from lichtfeld_densification_plugin_amd.core import matcher as matcher_mod
from lichtfeld_densification_plugin_amd.core import pipeline as pl
from lichtfeld_densification_plugin_amd.core.refiner_blocks import FusedRefinerBlocks, check_structure, is_block
from lichtfeld_densification_plugin_amd.core.types import EXPERIMENTAL_DEFAULTS

SHAPE32, SHAPE33 = (2, 32, 7, 9), (1, 33, 9, 9)


def model_with(*blocks):
    """a module tree shaped like the model's: ``refiners`` a ModuleDict of modules that hold blocks (and other layers)"""
    m = nn.Module()
    m.refiners = nn.ModuleDict({str(i): nn.Sequential(b, nn.Conv2d(int(b.conv_depthwise.in_channels), 2, 1)) for i, b in enumerate(blocks)})
    m.elsewhere = nn.Conv2d(3, 3, 5, padding=2, groups=3)
    return m.eval()


@pytest.fixture
def shim():
    s = FusedRefinerBlocks(host_threads=2)
    yield s
    s.close()
    assert not s._ctx


def x_of(d, dtype=torch.float32):
    return torch.from_numpy(d["x"].copy()).to(dtype)


def test_blocks_are_found_by_structure_and_the_forward_is_installed_and_removed(shim):
    b32, b33 = R.stand_in_block(R.case(SHAPE32, True)), R.stand_in_block(R.case(SHAPE33))
    model = model_with(b32, b33)
    assert is_block(b32) and not is_block(model.elsewhere) and not is_block(model.refiners["0"])
    assert shim.blocks(model) == [b32, b33]
    with shim.installed(model):
        assert all("forward" in b.__dict__ for b in (b32, b33))
        assert "forward" not in model.elsewhere.__dict__ and "forward" not in model.refiners["0"][1].__dict__
        inside = b32(x_of(R.case(SHAPE32, True)))
    assert all("forward" not in b.__dict__ for b in (b32, b33))
    assert inside.dtype == torch.bfloat16
    # an instance-level forward somebody else put there is what comes back
    marker = lambda x: x       # noqa: E731
    b33.forward = marker
    with shim.installed(model):
        assert b33.__dict__["forward"] is not marker
    assert b33.__dict__["forward"] is marker


def test_the_forward_is_removed_when_the_body_raises(shim):
    b32 = R.stand_in_block(R.case(SHAPE32, True))
    model = model_with(b32)
    with pytest.raises(RuntimeError, match="the model failed"):
        with shim.installed(model):
            assert "forward" in b32.__dict__
            raise RuntimeError("the model failed")
    assert "forward" not in b32.__dict__
    # ... and when a later block of the same model cannot be served, the earlier ones are as they were
    bad = R.stand_in_block(R.case(SHAPE33))
    bad.conv_depthwise = nn.Conv2d(33, 33, 3, padding=1, groups=33)
    with pytest.raises(NotImplementedError, match="5x5"):
        with shim.installed(model_with(b32, bad)):
            raise AssertionError("not reached")
    assert "forward" not in b32.__dict__ and "forward" not in bad.__dict__


def test_every_refusal_names_what_was_found(shim):
    d = R.case(SHAPE33)
    x = x_of(d)
    blk = R.stand_in_block(d)
    blk.train()
    with pytest.raises(NotImplementedError, match="training mode"):
        shim.forward(blk, x)
    with pytest.raises(NotImplementedError, match="enable_amp False"):
        shim.forward(R.stand_in_block(d, enable_amp=False), x)
    for change, piece in [(dict(conv_depthwise=nn.Conv2d(33, 33, 3, padding=1, groups=33)), r"5x5.*\(3, 3\)"),
                          (dict(conv_depthwise=nn.Conv2d(33, 33, 5, stride=2, padding=2, groups=33)), r"stride \(2, 2\)"),
                          (dict(conv_depthwise=nn.Conv2d(33, 33, 5, padding=4, dilation=2, groups=33)), r"dilation \(2, 2\)"),
                          (dict(conv_depthwise=nn.Conv2d(33, 33, 5, padding=2, groups=33, padding_mode="reflect")), "padding_mode 'reflect'"),
                          (dict(conv_depthwise=nn.Conv2d(33, 33, 5, padding=1, groups=33)), r"padding \(1, 1\)"),
                          (dict(conv_depthwise=nn.Conv2d(33, 33, 5, padding=2, groups=11)), "groups 11"),
                          (dict(norm=nn.GroupNorm(3, 33)), "GroupNorm"),
                          (dict(norm=nn.BatchNorm2d(33, track_running_stats=False)), "track_running_stats False"),
                          (dict(norm=nn.BatchNorm2d(33, affine=False)), "affine False"),
                          (dict(relu=nn.GELU()), "GELU"),
                          (dict(conv_pointwise=nn.Conv2d(33, 33, 3, padding=1)), "1x1"),
                          (dict(conv_pointwise=nn.Conv2d(33, 66, 1)), "1x1")]:
        blk = R.stand_in_block(d)
        for name, module in change.items():
            setattr(blk, name, module.eval())
        with pytest.raises(NotImplementedError, match=piece):
            check_structure(blk)
        with pytest.raises(NotImplementedError, match=piece):
            shim.forward(blk, x)
        with pytest.raises(NotImplementedError, match=piece):
            shim.blocks(model_with(blk))
    blk = R.stand_in_block(d)
    for dtype in (torch.float16, torch.float64):
        with pytest.raises(NotImplementedError, match=str(dtype).replace("torch.", "")):
            shim.forward(blk, x.to(dtype))
    with pytest.raises(NotImplementedError, match="backward"):
        shim.forward(blk, x.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError, match=r"\(B, 33, H, W\)"):
        shim.forward(blk, x[:, :32])
    assert shim.forward(blk, x).shape == x.shape             # and the block itself is served


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_the_fused_forward_is_inside_the_bound(shim, dtype):
    """C == 32: the whole block is the one call"""
    for shape in (SHAPE32, (1, 32, 17, 67)):
        d = R.case(shape, True)
        blk = R.stand_in_block(d)
        calls = []
        hook = blk.conv_pointwise.register_forward_hook(lambda *a: calls.append(1))
        x = x_of(d, dtype) if dtype == torch.float32 else torch.from_numpy(d["xb"].copy()).to(dtype)
        with torch.no_grad():
            plain = blk(x)
            n_plain = len(calls)
            with shim.installed(model_with(blk)):
                fused = blk(x)
        hook.remove()
        assert len(calls) == n_plain                         # the block's own 1x1 convolution did not run
        bad, worst = R.violations(R.to_numpy(fused), d["ref"], d["bound"])
        theirs = R.violations(R.to_numpy(plain), d["ref"], d["bound"])[1]
        print(f"{shape} {dtype}: fused worst |out - ref| / bound = {worst:.4f} ({bad} outside); the block's own forward: {theirs:.2f}")
        assert bad == 0 and fused.dtype == torch.bfloat16 and fused.shape == plain.shape


def test_for_other_widths_the_blocks_own_pointwise_convolution_runs(shim):
    d = R.case(SHAPE33)
    blk = R.stand_in_block(d)
    seen = []
    hook = blk.conv_pointwise.register_forward_hook(lambda m, inp, out: seen.append((inp[0], out, torch.is_autocast_enabled("cpu"))))
    x = x_of(d)
    with torch.no_grad(), shim.installed(model_with(blk)):
        fused = blk(x)
    hook.remove()
    assert len(seen) == 1
    hidden, out, autocast_on = seen[0]
    assert autocast_on and hidden.dtype == torch.bfloat16 and out is fused and fused.dtype == torch.bfloat16
    bad, worst = R.violations(R.to_numpy(hidden), d["ref"], d["bound"])      # what the 1x1 convolution was given: the fused hidden value
    with torch.no_grad():
        plain = blk(x)
    print(f"{SHAPE33}: hidden value worst |out - ref| / bound = {worst:.4f}; max |fused block - the block's own forward| = "
          f"{float((fused.float() - plain.float()).abs().max()):.4f} at magnitude {float(plain.float().abs().max()):.2f}")
    assert bad == 0
    assert float((fused.float() - plain.float()).abs().max()) <= 0.05 * float(plain.float().abs().max())     # two bf16 pipelines, loosely


def test_parameters_are_folded_once_and_again_after_a_change(shim):
    d = R.case(SHAPE32, True)
    blk = R.stand_in_block(d)
    x = x_of(d)
    first = shim.forward(blk, x)
    kept = shim._folded[id(blk)][1]
    assert shim.forward(blk, x) is not first and shim._folded[id(blk)][1] is kept          # cached
    s_want, t_want = R.fold(d["bn_gamma"], d["bn_beta"], d["bn_mean"], d["bn_var"], d["dw_b"], eps=blk.norm.eps)
    assert np.array_equal(kept[1].numpy(), s_want) and np.array_equal(kept[2].numpy(), t_want)     # f64 arithmetic, rounded once
    assert np.array_equal(kept[3].numpy(), d["wt"])
    with torch.no_grad():
        blk.norm.running_var.mul_(4.0)                       # in place: same storage, new version
    second = shim.forward(blk, x)
    assert shim._folded[id(blk)][1] is not kept
    s2, t2 = R.fold(d["bn_gamma"], d["bn_beta"], d["bn_mean"], 4.0 * d["bn_var"], d["dw_b"], eps=blk.norm.eps)
    ref, bound = R.reference(d["xb"], d["dw_w"], s2, t2, d["wt"], d["pw_b"])
    assert R.violations(R.to_numpy(second), ref, bound)[0] == 0
    assert R.violations(R.to_numpy(first), ref, bound)[0] > 0                             # (the change is one the bound can tell)
    blk.conv_pointwise.bias = nn.Parameter(torch.zeros(32), requires_grad=False)           # replaced: new storage
    third = shim.forward(blk, x)
    ref, bound = R.reference(d["xb"], d["dw_w"], s2, t2, d["wt"], np.zeros(32, np.float32))
    assert R.violations(R.to_numpy(third), ref, bound)[0] == 0


# ---- the knob: matcher, configuration, command line, pipeline ------------------------------------------------------------------------------

@pytest.fixture
def stand_in(monkeypatch):
    """``romav2`` with a RoMaV2 of the interface core/matcher.py uses whose ``refiners`` hold one stand-in block; ``match_from_features``
    records whether the block carries an instance-level forward while the model runs, and runs it."""
    d = R.case(SHAPE32, True)
    seen = types.SimpleNamespace(installed=[], outs=[], fail=False, case=d)

    class RoMaV2(nn.Module):
        class Cfg:
            def __init__(self, **kw):
                pass

        def __init__(self, cfg):
            super().__init__()
            self.f = nn.Identity()
            self.refiners = nn.ModuleDict({"1": nn.Sequential(R.stand_in_block(d))})
            self.H_lr = self.W_lr = 16
            self.H_hr = self.W_hr = None
            self.bidirectional = False

        def apply_setting(self, setting):
            pass

        def _load_image(self, im):
            return im.float()

        def match_from_features(self, f_list_A, img_A_lr, imB, img_A_hr):
            blk = self.refiners["1"][0]
            seen.installed.append("forward" in blk.__dict__)
            if seen.fail:
                raise RuntimeError("the model failed")
            seen.outs.append(blk(x_of(d)))
            return {"warp_AB": torch.zeros(1, 16, 16, 2), "overlap_AB": torch.zeros(1, 16, 16, 1)}

    pkg = types.ModuleType("romav2")
    pkg.RoMaV2 = RoMaV2
    monkeypatch.setitem(sys.modules, "romav2", pkg)
    return seen


def _image():
    return torch.zeros(20, 24, 3, dtype=torch.uint8)


def test_the_matcher_installs_the_shim_for_the_duration_of_a_match(stand_in):
    seen = stand_in
    m = matcher_mod.RomaMatcher(device="cpu", fused_refiner_blocks=True)
    assert m.supports_fused_refiner_blocks and m.fused_refiner_blocks and not m.fused_local_corr
    blk = m.model.refiners["1"][0]
    assert "forward" not in blk.__dict__                       # creating the matcher installs nothing
    assert len(m.match_grids_batch(_image(), [_image(), _image()])) == 2
    assert seen.installed == [True, True] and "forward" not in blk.__dict__
    d = seen.case
    assert R.violations(R.to_numpy(seen.outs[0]), d["ref"], d["bound"])[0] == 0      # the model's call reached the twin
    seen.fail = True
    with pytest.raises(RuntimeError, match="the model failed"):
        m.match_grids_batch(_image(), [_image()])
    assert seen.installed[-1] is True and "forward" not in blk.__dict__              # restored when the model raises
    seen.fail = False
    shim = m._refiner_blocks
    m.set_fused_refiner_blocks(False)
    assert not m.fused_refiner_blocks and not shim._ctx                              # switched off: its contexts are closed
    m.match_grids_batch(_image(), [_image()])
    assert seen.installed[-1] is False
    m.set_fused_refiner_blocks(True)
    shim = m._refiner_blocks
    m.match_grids_batch(_image(), [_image()])
    assert seen.installed[-1] is True and shim._ctx
    m.close()
    assert not shim._ctx                                                              # closed with the matcher


def test_with_the_knob_off_nothing_new_is_imported_or_touched(stand_in, monkeypatch):
    seen = stand_in
    monkeypatch.delitem(sys.modules, "lichtfeld_densification_plugin_amd.core.refiner_blocks", raising=False)
    m = matcher_mod.RomaMatcher(device="cpu")
    assert not m.fused_refiner_blocks
    blk = m.model.refiners["1"][0]
    with torch.no_grad():
        want = blk(x_of(seen.case))
    m.match_grids_batch(_image(), [_image()])
    assert seen.installed == [False]
    assert torch.equal(seen.outs[0], want)                                            # the block's own forward, bit for bit
    assert "lichtfeld_densification_plugin_amd.core.refiner_blocks" not in sys.modules
    m.close()


def test_the_knob_is_experimental_off_by_default_and_a_bool():
    assert EXPERIMENTAL_DEFAULTS["fused_refiner_blocks"] is False
    assert lfd.DensePipelineConfig(output_path="a.ply").exp("fused_refiner_blocks") is False
    for backend in ("device", "host"):
        assert lfd.DensePipelineConfig(output_path="a.ply", backend=backend, experimental={"fused_refiner_blocks": True}).problem() is None
    for wrong in (1, 0, "yes", None, 1.0):
        with pytest.raises(ValueError, match=r"experimental\['fused_refiner_blocks'\] must be True or False"):
            lfd.DensePipelineConfig(output_path="a.ply", experimental={"fused_refiner_blocks": wrong})


def test_the_command_line_flag():
    ap = densify.build_argparser()
    assert densify._experimental_from_args(ap.parse_args(["--scene_root", "s"])) == {}
    assert densify._experimental_from_args(ap.parse_args(["--scene_root", "s", "--fused_refiner_blocks"])) == {"fused_refiner_blocks": True}


class _PlainMatcher:
    sample_thresh = 0.9
    w_resized = h_resized = 32

    def match_grids_batch(self, imA, imB_list):
        raise AssertionError("the run must be refused before the first match")

    def close(self):
        pass


def _config(tmp_path, on):
    return lfd.DensePipelineConfig(output_path=os.path.join(str(tmp_path), "o.ply"), nns_per_ref=1, viz_interval=0, backend="host",
                                   experimental={"fused_refiner_blocks": on})


def test_an_injected_matcher_without_the_capability_refuses_the_knob(tmp_path):
    cams = synthetic.ring_cameras(2, seed=0)
    with pytest.raises(ValueError, match="supports_fused_refiner_blocks"):
        pl.run_dense_pipeline(cams, [0, 1], np.array([[1], [0]]), _config(tmp_path, True), matcher=_PlainMatcher())


def test_an_injected_matcher_with_the_capability_receives_the_knob(tmp_path):
    calls = []

    class Capable(_PlainMatcher):
        supports_fused_refiner_blocks = True

        def set_fused_refiner_blocks(self, on):
            calls.append(on)

        def match_grids_batch(self, imA, imB_list):
            raise RuntimeError("stop here")

    cams = synthetic.ring_cameras(2, seed=0)
    for on in (True, False):
        with pytest.raises(Exception):
            pl.run_dense_pipeline(cams, [0, 1], np.array([[1], [0]]), _config(tmp_path, on), matcher=Capable())
    assert calls == [True, False]
