"""The model-facing side of the fused local correlation: the shim's refusals (core/local_corr.py), the installation of the shim as
``romav2.local_correlation.local_corr`` for the duration of a ``RomaMatcher.match_grids_batch`` call (core/matcher.py) - against a stand-in
module tree in ``sys.modules``, RoMa-v2 itself is not needed - and the refusal of the knob for a matcher that cannot honour it (core/pipeline.py)."""
import os
import sys
import types

import numpy as np
import pytest
import torch

import lichtfeld_densification_plugin_amd as lfd
from lichtfeld_densification_plugin_amd import synthetic
from lichtfeld_densification_plugin_amd.core import matcher as matcher_mod
from lichtfeld_densification_plugin_amd.core import pipeline as pl
from lichtfeld_densification_plugin_amd.core.local_corr import LocalCorr
from lichtfeld_densification_plugin_amd.core.types import EXPERIMENTAL_DEFAULTS
from local_corr_ref import model_case, reference_numpy, violations


def _tensors(C=8):
    return tuple(torch.as_tensor(t) for t in model_case(1, C, 4, 4, 1, seed=2))


def test_the_shim_refuses_what_the_kernel_does_not_implement():
    shim = LocalCorr(host_threads=1)
    a, bf, warp = _tensors()
    try:
        with pytest.raises(NotImplementedError, match="bilinear"):
            shim.local_corr(a, bf, warp, mode="nearest")
        with pytest.raises(NotImplementedError, match="normalized_coords"):
            shim.local_corr(a, bf, warp, normalized_coords=False)
        with pytest.raises(NotImplementedError, match="float32"):
            shim.local_corr(a.half(), bf, warp)
        with pytest.raises(NotImplementedError, match="float32"):
            shim.local_corr(a, bf.double(), warp)
        with pytest.raises(NotImplementedError, match="backward"):
            shim.local_corr(a.clone().requires_grad_(True), bf, warp)
        out = shim.local_corr(a, bf, warp, mode="bilinear", normalized_coords=True)          # upstream's call, keywords and all
        ref, bound = reference_numpy(a.numpy(), bf.numpy(), warp.numpy())
        assert violations(out.numpy().astype(np.float64), ref, bound)[0] == 0
        assert torch.equal(shim(a, bf, warp), out)
    finally:
        shim.close()
    assert not shim._ctx


class _Seen(list):
    pass


@pytest.fixture
def stand_in(monkeypatch):
    """``romav2`` with a RoMaV2 of the interface core/matcher.py uses, and ``romav2.local_correlation`` with the attribute the real module has
    (None: the CUDA-only extension is missing).  ``match_from_features`` records what the attribute is while the model runs and, when it is a
    shim, calls it the way the model's wrapper does."""
    seen = _Seen()
    seen.fail = False
    lc = types.ModuleType("romav2.local_correlation")
    lc.local_corr = None

    class RoMaV2(torch.nn.Module):
        class Cfg:
            def __init__(self, **kw):
                pass

        def __init__(self, cfg):
            super().__init__()
            self.f = torch.nn.Identity()
            self.H_lr = self.W_lr = 16
            self.H_hr = self.W_hr = None
            self.bidirectional = False

        def apply_setting(self, setting):
            pass

        def _load_image(self, im):
            return im.float()

        def match_from_features(self, f_list_A, img_A_lr, imB, img_A_hr):
            seen.append(lc.local_corr)
            if seen.fail:
                raise RuntimeError("the model failed")
            if lc.local_corr is not None:
                a, bf, warp = _tensors()
                seen.out = lc.local_corr.local_corr(a, bf, warp, mode="bilinear", normalized_coords=True)
            return {"warp_AB": torch.zeros(1, 16, 16, 2), "overlap_AB": torch.zeros(1, 16, 16, 1)}

    pkg = types.ModuleType("romav2")
    pkg.RoMaV2 = RoMaV2
    pkg.local_correlation = lc
    monkeypatch.setitem(sys.modules, "romav2", pkg)
    monkeypatch.setitem(sys.modules, "romav2.local_correlation", lc)
    return lc, seen


def _image():
    return torch.zeros(20, 24, 3, dtype=torch.uint8)


def test_the_shim_is_installed_for_the_duration_of_a_match_and_restored(stand_in):
    lc, seen = stand_in
    m = matcher_mod.RomaMatcher(device="cpu", fused_local_corr=True)
    assert m.supports_fused_local_corr and m.fused_local_corr
    assert lc.local_corr is None                                   # creating the matcher installs nothing
    res = m.match_grids_batch(_image(), [_image(), _image()])
    assert len(res) == 2 and len(seen) == 2
    assert all(isinstance(s, LocalCorr) for s in seen) and seen[0] is seen[1]
    assert lc.local_corr is None                                   # ... and afterwards the module is as it was
    a, bf, warp = _tensors()
    ref, bound = reference_numpy(a.numpy(), bf.numpy(), warp.numpy())
    assert violations(seen.out.numpy().astype(np.float64), ref, bound)[0] == 0      # the model's call reached the twin
    # a value somebody else put there is what comes back, not None
    marker = object()
    lc.local_corr = marker
    m.match_grids_batch(_image(), [_image()])
    assert lc.local_corr is marker and isinstance(seen[-1], LocalCorr)
    lc.local_corr = None
    m.close()
    assert not seen[0]._ctx                                        # the shim's contexts are closed with the matcher


def test_the_attribute_is_restored_when_the_model_raises(stand_in):
    lc, seen = stand_in
    m = matcher_mod.RomaMatcher(device="cpu", fused_local_corr=True)
    seen.fail = True
    with pytest.raises(RuntimeError, match="the model failed"):
        m.match_grids_batch(_image(), [_image()])
    assert isinstance(seen[0], LocalCorr) and lc.local_corr is None
    m.close()


def test_with_the_knob_off_the_attribute_is_never_touched(stand_in, monkeypatch):
    lc, seen = stand_in

    class Guard(types.ModuleType):
        def __setattr__(self, name, value):
            raise AssertionError(f"romav2.local_correlation.{name} was written with the knob off")

    guard = Guard("romav2.local_correlation")
    guard.__dict__["local_corr"] = None
    monkeypatch.setitem(sys.modules, "romav2.local_correlation", guard)
    monkeypatch.delitem(sys.modules, "lichtfeld_densification_plugin_amd.core.local_corr", raising=False)
    m = matcher_mod.RomaMatcher(device="cpu")
    assert not m.fused_local_corr
    m.match_grids_batch(_image(), [_image()])
    assert seen == [None]
    assert "lichtfeld_densification_plugin_amd.core.local_corr" not in sys.modules      # no new import either
    m.set_fused_local_corr(True)
    m.set_fused_local_corr(False)                                  # switched on and off again: still untouched
    m.match_grids_batch(_image(), [_image()])
    assert seen == [None, None]
    m.close()


def test_the_knob_is_experimental_and_off_by_default():
    assert EXPERIMENTAL_DEFAULTS["fused_local_corr"] is False
    cfg = lfd.DensePipelineConfig(output_path="a.ply")
    assert cfg.exp("fused_local_corr") is False
    for backend in ("device", "host"):
        assert lfd.DensePipelineConfig(output_path="a.ply", backend=backend, experimental={"fused_local_corr": True}).problem() is None


class _PlainMatcher:
    sample_thresh = 0.9
    w_resized = h_resized = 32

    def match_grids_batch(self, imA, imB_list):
        raise AssertionError("the run must be refused before the first match")

    def close(self):
        pass


def test_an_injected_matcher_without_the_capability_refuses_the_knob(tmp_path):
    cams = synthetic.ring_cameras(2, seed=0)
    cfg = lfd.DensePipelineConfig(output_path=os.path.join(str(tmp_path), "o.ply"), nns_per_ref=1, viz_interval=0, backend="host",
                                  experimental={"fused_local_corr": True})
    with pytest.raises(ValueError, match="supports_fused_local_corr"):
        pl.run_dense_pipeline(cams, [0, 1], np.array([[1], [0]]), cfg, matcher=_PlainMatcher())


def test_an_injected_matcher_with_the_capability_receives_the_knob(tmp_path):
    calls = []

    class Capable(_PlainMatcher):
        supports_fused_local_corr = True

        def set_fused_local_corr(self, on):
            calls.append(on)

        def match_grids_batch(self, imA, imB_list):
            raise RuntimeError("stop here")

    cams = synthetic.ring_cameras(2, seed=0)
    for on in (True, False):
        cfg = lfd.DensePipelineConfig(output_path=os.path.join(str(tmp_path), "o.ply"), nns_per_ref=1, viz_interval=0, backend="host",
                                      experimental={"fused_local_corr": on})
        with pytest.raises(Exception):
            pl.run_dense_pipeline(cams, [0, 1], np.array([[1], [0]]), cfg, matcher=Capable())
    assert calls == [True, False]
