#!/usr/bin/env python3
"""The fused refiner head inside the REAL conv refiners - development container only, like check_refiner_block_contract.py: the reference
tree does not exist on the GPU box, and nothing of it is copied.

    python tests/golden/check_refiner_head_contract.py [--write]      -> tests/golden/g22_refiner_head_contract.json

Upstream's three ``ConvRefiner`` modules (RoMaV2/src/romav2/refiner.py; patch 4 / 2 / 1, hidden width 512 / 128 / 32) with seeded weights
and seeded BatchNorm statistics run on the CPU on seeded inputs twice: as they are, and with ``core.refiner_head.FusedRefinerHead`` installed
(the CPU twin of lfd_refiner_head).  The previous warp and confidence are handed over through the model's ``bhwc_interpolate``, so the strided
views are the real ones; the confidence has 1 channel for patch 4 and 4 channels for the others.  Asserted here: what ``block1`` is given
(forward pre-hook) and ``z`` (forward hook on ``hidden_blocks``) are bit-equal between the two runs, and the fused outputs lie inside the
derived bound (tests/refiner_head_ref.py) around the f64 evaluation of the tail from that same ``z``.  Recorded per refiner:
max |fused - model|, max |fused - f64| and max |model - f64| for ``warp`` and ``confidence``."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from check_matcher_contract import install_stubs  # noqa: E402

CASES = {"4": (256, 24, 1), "2": (128, 40, 4), "1": (64, 48, 4)}   # patch -> (feature dimension, grid side as in g20, channels of the previous confidence)
BATCH = 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    install_stubs()
    import refiner_head_ref as R
    from romav2.geometry import bhwc_interpolate, get_normalized_grid
    from romav2.refiner import ConvRefiner, Refiners
    from lichtfeld_densification_plugin_amd.core.refiner_head import FusedRefinerHead, is_refiner
    torch.manual_seed(22)
    refiners = Refiners(Refiners.Cfg()).eval()
    with torch.no_grad():
        for m in refiners.modules():
            if isinstance(m, torch.nn.BatchNorm2d):                  # a trained model's statistics are not (0, 1)
                m.running_mean.normal_(0.0, 0.2)
                m.running_var.uniform_(0.5, 2.0)
    holder = torch.nn.Module()
    holder.refiners = refiners
    shim = FusedRefinerHead()
    assert [r for r in refiners.modules() if is_refiner(r)] == [refiners[p] for p in ("4", "2", "1")] == shim.refiners(holder)
    record = {"what": "ConvRefiner outputs on the CPU, seeded weights, BatchNorm statistics and inputs, B = %d, previous state through "
                      "bhwc_interpolate; fused = FusedRefinerHead installed (CPU twin), model = the refiner's own forward, f64 = the f64 evaluation "
                      "of the tail from the same z; max |difference| each" % BATCH,
              "condition": "block1 input and z bit-equal between the two runs; fused inside the derived bound around f64", "refiners": {}}
    for patch, (feat, side, prev_dim) in CASES.items():
        refiner = refiners[patch]
        assert isinstance(refiner, ConvRefiner)
        coarse = side // 2
        grid = get_normalized_grid(BATCH, coarse, coarse)
        prev_warp = bhwc_interpolate(grid + 0.05 * torch.randn(BATCH, coarse, coarse, 2), size=(side, side), mode="bilinear", align_corners=False)
        prev_conf = bhwc_interpolate(torch.randn(BATCH, coarse, coarse, prev_dim), size=(side, side), mode="bilinear", align_corners=False)
        inputs = dict(f_A=torch.randn(BATCH, side, side, feat), f_B=torch.randn(BATCH, side, side, feat), prev_warp=prev_warp,
                      prev_confidence=prev_conf, scale_factor=torch.tensor([float(side), float(side)]))
        seen = {"d": [], "z": []}
        hooks = [refiner.block1.register_forward_pre_hook(lambda m, args: seen["d"].append(args[0].clone())),
                 refiner.hidden_blocks.register_forward_hook(lambda m, args, out: seen["z"].append(out.clone()))]
        with torch.inference_mode():
            model = refiner(**inputs)
            with shim.installed(holder):
                assert "forward" in refiner.__dict__
                fused = refiner(**inputs)
        for h in hooks:
            h.remove()
        assert "forward" not in refiner.__dict__
        d_equal, z_equal = bool(torch.equal(seen["d"][0], seen["d"][1])), bool(torch.equal(seen["z"][0], seen["z"][1]))
        z = seen["z"][1]
        C = refiner.hidden_dim
        head_w = np.concatenate([refiner.warp_head.weight.detach().numpy().reshape(2, C), refiner.confidence_head.weight.detach().numpy().reshape(4, C)], 0)
        head_b = np.concatenate([refiner.warp_head.bias.detach().numpy(), refiner.confidence_head.bias.detach().numpy()])
        rw, bw, rc, bc, _ = R.reference(z.float().numpy(), head_w, head_b, prev_warp.numpy(), prev_conf.numpy(), refiner.cfg.refine_init)
        out_w, out_c = R.violations(fused["warp"].numpy(), rw, bw), R.violations(fused["confidence"].numpy(), rc, bc)
        dist = lambda p, q: float(np.abs(np.asarray(p, np.float64) - np.asarray(q, np.float64)).max())          # noqa: E731
        entry = {"hidden_width": C, "grid": [side, side], "prev_confidence_channels": prev_dim, "z_dtype": str(z.dtype).replace("torch.", ""),
                 "prev_warp_contiguous": bool(prev_warp.is_contiguous()), "prev_warp_strides": list(prev_warp.stride()),
                 "block1_input_bit_equal": d_equal, "z_bit_equal": z_equal,
                 "fused_outside_bound": {"warp": out_w[0], "confidence": out_c[0]},
                 "fused_worst_over_bound": {"warp": out_w[1], "confidence": out_c[1]},
                 "fused_vs_model": {"warp": dist(fused["warp"].numpy(), model["warp"].numpy()), "confidence": dist(fused["confidence"].numpy(), model["confidence"].numpy())},
                 "fused_vs_f64": {"warp": dist(fused["warp"].numpy(), rw), "confidence": dist(fused["confidence"].numpy(), rc)},
                 "model_vs_f64": {"warp": dist(model["warp"].numpy(), rw), "confidence": dist(model["confidence"].numpy(), rc)},
                 "magnitude": {"warp": float(np.abs(rw).max()), "confidence": float(np.abs(rc).max())}}
        record["refiners"]["patch " + patch] = entry
        print("patch", patch, json.dumps(entry))
        assert d_equal and z_equal, (patch, d_equal, z_equal)
        assert out_w[0] == 0 and out_c[0] == 0, (patch, out_w, out_c)
    shim.close()
    if a.write:
        dst = os.path.join(HERE, "g22_refiner_head_contract.json")
        with open(dst, "w") as fh:
            json.dump(record, fh, indent=1, sort_keys=True)
            fh.write("\n")
        print("wrote", dst)


if __name__ == "__main__":
    main()
