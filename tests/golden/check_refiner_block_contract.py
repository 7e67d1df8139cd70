#!/usr/bin/env python3
"""The fused refiner block inside the REAL conv refiners - development container only, like check_local_corr_contract.py: the reference
tree does not exist on the GPU box, and nothing of it is copied.

    python tests/golden/check_refiner_block_contract.py [--write]      -> tests/golden/g20_refiner_block_contract.json

Upstream's three ``ConvRefiner`` modules (RoMaV2/src/romav2/refiner.py; patch 4 / 2 / 1, hidden width 512 / 128 / 32, nine blocks each) with
seeded weights and seeded BatchNorm statistics run on the CPU on seeded inputs three times: as they are (bf16 autocast in every block), with
``core.refiner_blocks.FusedRefinerBlocks`` installed (the CPU twin of lfd_refiner_block), and with ``enable_amp`` off in every block - the
f32 evaluation both bf16 pipelines approximate.  Recorded per refiner: the largest absolute differences of ``warp`` and ``confidence``
between fused and fallback, fused and f32, fallback and f32.  Condition (asserted here, DESIGN.md 4.18 quotes the numbers): the fused
distance to the f32 evaluation does not exceed twice the fallback's own - the yardstick is the reference's two paths, both measured here."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from check_matcher_contract import install_stubs  # noqa: E402

CASES = {"4": (256, 24), "2": (128, 40), "1": (64, 48)}          # patch -> (feature dimension of the refiner's input, grid side)
BATCH = 2


def run(refiner, inputs):
    with torch.inference_mode():
        out = refiner(**inputs)
    return out["warp"].float().clone(), out["confidence"].float().clone()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    install_stubs()
    from romav2.geometry import get_normalized_grid
    from romav2.refiner import Block, Refiners
    from lichtfeld_densification_plugin_amd.core.refiner_blocks import FusedRefinerBlocks, is_block
    torch.manual_seed(20)
    refiners = Refiners(Refiners.Cfg()).eval()
    with torch.no_grad():
        for m in refiners.modules():
            if isinstance(m, torch.nn.BatchNorm2d):                  # a trained model's statistics are not (0, 1)
                m.running_mean.normal_(0.0, 0.2)
                m.running_var.uniform_(0.5, 2.0)
    holder = torch.nn.Module()
    holder.refiners = refiners
    launches = []

    class Counting(FusedRefinerBlocks):
        def forward(self, block, x):
            launches.append(int(x.shape[1]))
            return super().forward(block, x)

    shim = Counting()
    record = {"what": "max |difference| of ConvRefiner outputs on the CPU, seeded weights, BatchNorm statistics and inputs, B = %d; fused = "
                      "FusedRefinerBlocks installed, fallback = the model's own bf16 autocast blocks, f32 = enable_amp off in every block" % BATCH,
              "condition": "fused_vs_f32 <= 2 * fallback_vs_f32, for warp and for confidence", "refiners": {}}
    for patch, (feat, side) in CASES.items():
        refiner = refiners[patch]
        blocks = [m for m in refiner.modules() if is_block(m)]
        assert len(blocks) == 9 and all(isinstance(b, Block) for b in blocks)
        grid = get_normalized_grid(BATCH, side, side)
        inputs = dict(f_A=torch.randn(BATCH, side, side, feat), f_B=torch.randn(BATCH, side, side, feat),
                      prev_warp=grid + 0.1 * torch.randn(BATCH, side, side, 2), prev_confidence=None,
                      scale_factor=torch.tensor([float(side), float(side)]))
        wb, cb = run(refiner, inputs)
        del launches[:]
        with shim.installed(holder):
            wf, cf = run(refiner, inputs)
        assert all("forward" not in b.__dict__ for b in blocks)
        assert launches == [refiner.hidden_dim] * 9, launches
        for b in blocks:
            b.enable_amp = False
        w32, c32 = run(refiner, inputs)
        for b in blocks:
            b.enable_amp = True
        d = lambda p, q: float((p - q).abs().max())          # noqa: E731
        entry = {"hidden_width": refiner.hidden_dim, "blocks": len(blocks), "grid": [side, side],
                 "fused_vs_fallback": {"warp": d(wf, wb), "confidence": d(cf, cb)},
                 "fused_vs_f32": {"warp": d(wf, w32), "confidence": d(cf, c32)},
                 "fallback_vs_f32": {"warp": d(wb, w32), "confidence": d(cb, c32)},
                 "magnitude": {"warp": float(w32.abs().max()), "confidence": float(c32.abs().max())}}
        record["refiners"]["patch " + patch] = entry
        print("patch", patch, json.dumps(entry))
        for key in ("warp", "confidence"):
            assert entry["fused_vs_f32"][key] <= 2.0 * entry["fallback_vs_f32"][key], (patch, key, entry)
    shim.close()
    if a.write:
        dst = os.path.join(HERE, "g20_refiner_block_contract.json")
        with open(dst, "w") as fh:
            json.dump(record, fh, indent=1, sort_keys=True)
            fh.write("\n")
        print("wrote", dst)


if __name__ == "__main__":
    main()
