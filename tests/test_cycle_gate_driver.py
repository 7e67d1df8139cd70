"""The forward-backward filter in the driver, on the host backend (core/pipeline.py, core/hotpath.py, core/matcher.py, synthetic.py): the knob
changes nothing when it is off, the floor travels with the gated planes (an enormous threshold gives the knob-off cloud bit for bit, in both
modes), no point is emitted from a pair the f64 reference rejects, a matcher that cannot hand out the backward warp is refused, and RomaMatcher
forces and restores ``model.bidirectional`` round every call - against a stand-in ``romav2``, the model itself is not needed."""
import logging
import os
import sys
import types

import numpy as np
import pytest
import torch

import cycle_ref
import cycle_scene
import lichtfeld_densification_plugin_amd as lfd
from lichtfeld_densification_plugin_amd import densify, synthetic
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from lichtfeld_densification_plugin_amd.core import matcher as matcher_mod
from lichtfeld_densification_plugin_amd.core import pipeline as pl
from lichtfeld_densification_plugin_amd.core.types import EXPERIMENTAL_DEFAULTS


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    return cycle_scene.make_scene(str(tmp_path_factory.mktemp("cycle_scene")))


def test_the_knob_is_experimental_off_by_default_and_validated():
    assert EXPERIMENTAL_DEFAULTS["cycle_thresh_px"] == 0.0
    assert lfd.DensePipelineConfig(output_path="a.ply").exp("cycle_thresh_px") == 0.0
    for mode in ("sampled", "dense"):
        for backend in ("device", "host"):
            assert lfd.DensePipelineConfig(output_path="a.ply", triangulation_mode=mode, backend=backend, no_filter=True,
                                           experimental={"cycle_thresh_px": 1.5}).problem() is None
    assert lfd.DensePipelineConfig(output_path="a.ply", stream_output=True, triangulation_mode="dense", refs_per_launch=4,
                                   experimental={"cycle_thresh_px": 1.0}).problem() is None
    for bad in (-1.0, float("inf"), float("nan"), "wide"):
        with pytest.raises(ValueError, match="cycle_thresh_px"):
            lfd.DensePipelineConfig(output_path="a.ply", experimental={"cycle_thresh_px": bad})
    args = densify.build_argparser().parse_args(["--scene_root", "x", "--cycle_thresh_px", "1.25"])
    assert args.cycle_thresh_px == 1.25
    assert densify.build_argparser().parse_args(["--scene_root", "x"]).cycle_thresh_px == 0.0


def test_the_kernels_floor_is_min_thresh_zero_only_when_the_planes_arrive_gated():
    off = lfd.DensePipelineConfig(output_path="a.ply", certainty_thresh=0.2)
    on = lfd.DensePipelineConfig(output_path="a.ply", certainty_thresh=0.2, experimental={"cycle_thresh_px": 1.0})
    neg = lfd.DensePipelineConfig(output_path="a.ply", certainty_thresh=-0.5, experimental={"cycle_thresh_px": 1.0})
    assert hb.make_params(off).certainty_thresh == np.float32(0.2)
    assert hb.make_params(on).certainty_thresh == 0.0
    assert hb.make_params(neg).certainty_thresh == -0.5
    assert on.certainty_thresh == 0.2                      # what the exactness checks of core/hotpath.py read is the configured value


@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_with_the_knob_off_no_new_code_runs(scene, mode, monkeypatch):
    def never(*a, **kw):
        raise AssertionError("the gate ran with the knob off")
    monkeypatch.setattr(hb.HostDensifier, "cycle_gate", never)
    m = cycle_scene.matcher_for(scene)
    plain = cycle_scene.run(scene, m, "plain.ply", triangulation_mode=mode)
    assert m.backward is False
    m.set_backward_warp(True)                              # a warm matcher left in the other state is switched back by the run
    zero = cycle_scene.run(scene, m, "zero.ply", triangulation_mode=mode, experimental={"cycle_thresh_px": 0.0})
    assert m.backward is False
    assert plain.xyz.shape[0] > 1000 and cycle_scene.same_cloud(plain, zero)


@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_an_enormous_threshold_gives_the_knob_off_cloud_bit_for_bit(scene, mode, caplog):
    """Forward warps clipped inside [-0.99, 0.99], tau = 1e9: nothing is rejected, every plane reaches the kernels carrying the floor, the kernels floor
    at 0 - the same values in the same cells, hence the same arg-max, the same weights, the same RNG draws, the same points."""
    off = cycle_scene.run(scene, cycle_scene.matcher_for(scene, clipped=True), "off.ply", triangulation_mode=mode)
    m = cycle_scene.matcher_for(scene, clipped=True)
    with caplog.at_level(logging.INFO, logger="lfd_densify"):
        on = cycle_scene.run(scene, m, "on.ply", triangulation_mode=mode, experimental={"cycle_thresh_px": 1e9})
    assert m.backward is True
    assert off.xyz.shape[0] > 1000 and cycle_scene.same_cloud(off, on)
    lines = [r.getMessage() for r in caplog.records if "Forward-backward filter" in r.getMessage()]
    cells = len(scene["refs"]) * 3 * 320 * 320
    assert lines == [f"Forward-backward filter: threshold 1e+09 px, {cells} cells, 0.00 % rejected"]


@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_no_point_comes_from_a_pair_the_reference_rejects(scene, mode):
    kw = dict(occlusion_steps=True, out_of_range=0.3)
    with cycle_scene.recorded_cells() as base:
        off = cycle_scene.run(scene, cycle_scene.matcher_for(scene, **kw), "slab_off.ply", triangulation_mode=mode)
    m = cycle_scene.matcher_for(scene, **kw)
    with cycle_scene.recorded_cells() as emitted:
        on = cycle_scene.run(scene, m, "slab_on.ply", triangulation_mode=mode, experimental={"cycle_thresh_px": 1.0})
    assert len(emitted) == len(base) == len(scene["refs"])
    assert 0 < on.xyz.shape[0] and (mode == "sampled" or on.xyz.shape[0] < 0.9 * off.xyz.shape[0])
    offending = would_have = 0
    for r, cells in zip(scene["refs"], emitted):
        nbrs = [int(n) for n in scene["nn"][r][:3]]
        _key, fields = m.fields(r, nbrs)
        refs = [cycle_ref.reference(c.numpy(), w.numpy(), b.numpy(), m.w_resized, m.h_resized, 0.2, 1.0) for w, c, b in fields]
        for cell, slot in cells:
            ref = refs[slot]
            y, x = divmod(cell, 320)
            offending += int(not ref["keep"][y, x] and not ref["band"][y, x])
    for r, cells in zip(scene["refs"], base):
        nbrs = [int(n) for n in scene["nn"][r][:3]]
        _key, fields = m.fields(r, nbrs)
        refs = [cycle_ref.reference(c.numpy(), w.numpy(), b.numpy(), m.w_resized, m.h_resized, 0.2, 1.0) for w, c, b in fields]
        would_have += sum(int(not refs[slot]["keep"][divmod(cell, 320)]) for cell, slot in cells)
    assert offending == 0
    assert would_have > 0.02 * sum(len(c) for c in base)          # ... and without the filter such points ARE emitted: the test can fail


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
                                  experimental={"cycle_thresh_px": 1.0})
    with pytest.raises(ValueError, match="supports_backward_warp"):
        pl.run_dense_pipeline(cams, [0, 1], np.array([[1], [0]]), cfg, matcher=_PlainMatcher())


def test_a_matcher_that_declares_the_capability_but_returns_pairs_is_an_error(scene):
    class Forgetful(synthetic.SyntheticMatcher):
        def set_backward_warp(self, on):
            pass
    m = Forgetful(scene["cams"], setting="turbo")
    with pytest.raises(RuntimeError, match="no backward warp"):
        cycle_scene.run(scene, m, "forgetful.ply", experimental={"cycle_thresh_px": 1.0})


def test_the_synthetic_backward_field_is_the_neighbours_own_and_is_handed_out_only_when_asked_for(scene):
    m = cycle_scene.matcher_for(scene)
    r = scene["refs"][0]
    nbrs = [int(n) for n in scene["nn"][r][:3]]
    pairs = m.match_grids_batch(None, [None] * 3, keys=(r, nbrs))
    assert all(len(p) == 2 for p in pairs)
    m.set_backward_warp(True)
    assert m.precompute([r], scene["nn"], 3) == 1 and len(m.back_table) == 1
    triples = m.match_grids_batch(None, [None] * 3, keys=(r, nbrs))
    assert all(len(t) == 3 and t[2].shape == (320, 320, 2) for t in triples)
    for (w, c, b), (w0, c0), n in zip(triples, pairs, nbrs):
        assert torch.equal(w, w0) and torch.equal(c, c0)
        own = synthetic.synth_reference(scene["cams"], n, [r], 320, 320, 320, 320, noise_px=0.5, outlier_frac=0.05).warp[0]
        assert torch.equal(b, own)
    triples[0][1].zero_()                                   # the driver gates in place: the table keeps its own certainty
    assert torch.equal(m.match_grids_batch(None, [None] * 3, keys=(r, nbrs))[0][1], pairs[0][1])
    m.set_backward_warp(False)
    assert all(len(p) == 2 for p in m.match_grids_batch(None, [None] * 3, keys=(r, nbrs)))


# ---- RomaMatcher against a stand-in romav2 ---------------------------------------------------------------------------------------------------
@pytest.fixture
def stand_in(monkeypatch):
    """``romav2.RoMaV2`` of the interface core/matcher.py uses.  Like the real class, it returns ``warp_BA`` only when ``bidirectional`` is set
    while it runs; ``seen`` records that flag at every forward."""
    seen = []
    state = {"fail": False}

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
            self.bidirectional = setting in ("precise",)

        def _load_image(self, im):
            return im.float()

        def _resize_match_image(self, im):
            return torch.zeros(im.shape[0], 3, 16, 16), None

        def _preds(self, n):
            seen.append(bool(self.bidirectional))
            if state["fail"]:
                raise RuntimeError("the model failed")
            ba = torch.arange(n, dtype=torch.float32).view(n, 1, 1, 1).expand(n, 16, 16, 2) + 0.5 if self.bidirectional else None
            return {"warp_AB": torch.zeros(n, 16, 16, 2), "overlap_AB": torch.zeros(n, 16, 16, 1), "warp_BA": ba}

        def match_from_features(self, f_list_A, img_A_lr, imB, img_A_hr):
            return self._preds(1)

        def _match_core(self, f_list_A, img_A_lr, img_B_lr, img_A_hr, img_B_hr):
            return self._preds(int(img_B_lr.shape[0]))

    pkg = types.ModuleType("romav2")
    pkg.RoMaV2 = RoMaV2
    monkeypatch.setitem(sys.modules, "romav2", pkg)
    return seen, state


def _image():
    return torch.zeros(1, 3, 20, 24)


@pytest.mark.parametrize("pairs_per_forward", [1, 2])
def test_bidirectional_is_forced_for_the_call_and_restored(stand_in, pairs_per_forward):
    seen, state = stand_in
    m = matcher_mod.RomaMatcher(device="cpu", setting="fast", pairs_per_forward=pairs_per_forward)
    assert m.supports_backward_warp and not m.backward_warp and m.model.bidirectional is False
    res = m.match_grids_batch(_image(), [_image()] * 3)
    assert all(len(r) == 2 for r in res) and set(seen) == {False}
    m.set_backward_warp(True)
    assert m.model.bidirectional is False                   # switching the knob touches nothing
    del seen[:]
    res = m.match_grids_batch(_image(), [_image()] * 3)
    assert set(seen) == {True} and len(seen) == (3 if pairs_per_forward == 1 else 2)
    assert m.model.bidirectional is False                   # ... and afterwards the model is as it was
    assert len(res) == 3 and all(len(r) == 3 for r in res)
    for i, (w, c, b) in enumerate(res):
        assert w.shape == (16, 16, 2) and c.shape == (16, 16) and b.shape == (16, 16, 2) and b.is_contiguous()
        # pair i of its own chunk: chunks of one hold index 0, a chunk of two holds 0 and 1
        assert float(b[0, 0, 0]) == (0.5 if pairs_per_forward == 1 else (i % 2) + 0.5)
    state["fail"] = True
    with pytest.raises(RuntimeError, match="the model failed"):
        m.match_grids_batch(_image(), [_image()])
    assert m.model.bidirectional is False                   # restored when the model raises, too
    state["fail"] = False
    m.set_backward_warp(False)
    del seen[:]
    assert all(len(r) == 2 for r in m.match_grids_batch(_image(), [_image()])) and seen == [False]
    m.close()


def test_a_bidirectional_preset_is_left_alone_and_four_channel_warps_carry_the_triple(stand_in):
    seen, _state = stand_in
    m = matcher_mod.RomaMatcher(device="cpu", setting="precise", two_channel=False)
    assert m.model.bidirectional is True
    m.set_backward_warp(True)
    res = m.match_grids_batch(_image(), [_image()])
    assert seen == [True] and m.model.bidirectional is True
    assert res[0][0].shape == (16, 16, 4) and res[0][2].shape == (16, 16, 2)
    m.close()
