#!/usr/bin/env python3
"""The fused local correlation inside the REAL conv refiners - development container only, like check_matcher_contract.py: the reference
tree does not exist on the GPU box, and nothing of it is copied.

    python tests/golden/check_local_corr_contract.py [--write]      -> tests/golden/g15_local_corr_contract.json

Upstream's ``ConvRefiner`` modules (RoMaV2/src/romav2/refiner.py; patch 4: 192 channels, 7 x 7 window; patch 2: 48 channels, 3 x 3 window) with
seeded weights run on the CPU on seeded inputs three times: with upstream's grid_sample fallback at 1 torch thread, the same at 16 threads,
and with ``core.local_corr.LocalCorr`` (the CPU twin of lfd_local_corr) installed as ``romav2.local_correlation.local_corr``.  Recorded: the
largest absolute differences of ``warp`` and ``confidence`` between the shim and the fallback, next to the same differences between the two
runs of the fallback - the model's own run-to-run noise.  No threshold is asserted: the record states both (DESIGN.md 4.6 quotes them)."""
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

CASES = {"4": (256, 24), "2": (128, 40)}          # patch -> (feature dimension of the refiner's input, grid side)
BATCH = 2


def run(refiner, inputs, threads):
    torch.set_num_threads(threads)
    with torch.inference_mode():
        out = refiner(**inputs)
    return out["warp"].float().clone(), out["confidence"].float().clone()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    install_stubs()
    import romav2.local_correlation as lc
    from romav2.geometry import get_normalized_grid
    from romav2.refiner import Refiners
    from lichtfeld_densification_plugin_amd.core.local_corr import LocalCorr
    from lichtfeld_densification_plugin_amd.core.matcher import _local_corr_installed
    assert lc.local_corr is None, "the CUDA extension is importable here: the comparison is against the fallback"
    torch.manual_seed(15)
    refiners = Refiners(Refiners.Cfg()).eval()
    calls = []

    class Counting(LocalCorr):
        def local_corr(self, *args, **kw):
            calls.append(1)
            return super().local_corr(*args, **kw)

    shim = Counting()
    threads_before = torch.get_num_threads()
    record = {"what": "max |difference| of ConvRefiner outputs on the CPU, seeded weights and inputs, B = %d" % BATCH, "refiners": {}}
    for patch, (feat, side) in CASES.items():
        refiner = refiners[patch]
        grid = get_normalized_grid(BATCH, side, side)
        inputs = dict(f_A=torch.randn(BATCH, side, side, feat), f_B=torch.randn(BATCH, side, side, feat),
                      prev_warp=grid + 0.1 * torch.randn(BATCH, side, side, 2), prev_confidence=None,
                      scale_factor=torch.tensor([float(side), float(side)]))
        del calls[:]
        w1, c1 = run(refiner, inputs, 1)
        w16, c16 = run(refiner, inputs, 16)
        with _local_corr_installed(shim):
            ws, cs = run(refiner, inputs, 16)
        assert lc.local_corr is None
        entry = {"shim_calls": len(calls),
                 "channels": refiner.cfg.proj_dim, "radius": refiner.cfg.local_corr_radius, "grid": [side, side],
                 "shim_vs_fallback": {"warp": float((ws - w16).abs().max()), "confidence": float((cs - c16).abs().max())},
                 "fallback_1_vs_16_threads": {"warp": float((w1 - w16).abs().max()), "confidence": float((c1 - c16).abs().max())},
                 "magnitude": {"warp": float(w16.abs().max()), "confidence": float(c16.abs().max())}}
        record["refiners"]["patch " + patch] = entry
        print("patch", patch, json.dumps(entry))
    torch.set_num_threads(threads_before)
    shim.close()
    if a.write:
        dst = os.path.join(HERE, "g15_local_corr_contract.json")
        with open(dst, "w") as fh:
            json.dump(record, fh, indent=1, sort_keys=True)
            fh.write("\n")
        print("wrote", dst)


if __name__ == "__main__":
    main()
