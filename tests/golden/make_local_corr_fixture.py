#!/usr/bin/env python3
"""Record upstream's own local correlation for tests/test_local_corr_fixture.py - development container only, like make_golden.py: the
reference tree does not exist on the GPU box, and nothing of it is copied.

    python tests/golden/make_local_corr_fixture.py        -> tests/golden/g14_local_corr.npz

``local_correlation`` of RoMaV2/src/romav2/local_correlation.py (it needs only torch) is loaded from the reference tree by file path and run on
the CPU in f32 on seeded inputs; its CUDA extension is absent, so what runs is ``native_torch_local_corr`` - the grid_sample formulation every
ROCm user gets today.  Stored: the inputs (feature0, feature1 (B, C, h, w), warp (B, h, w, 2), the radius) and upstream's output (B, K, h, w).
"""
from __future__ import annotations

import importlib.util
import os

import numpy as np
import torch

from ref_import import REFERENCE_ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = {"p4": (1, 192, 8, 8, 3), "p2": (2, 48, 12, 12, 1)}       # name -> (B, C, h, w, r): the two refiners, scaled down


def main():
    path = os.path.join(os.environ.get("LFD_REFERENCE_ROOT", REFERENCE_ROOT), "RoMaV2", "src", "romav2", "local_correlation.py")
    spec = importlib.util.spec_from_file_location("_upstream_local_correlation", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.local_corr is None, "the CUDA extension is importable here: this fixture records the fallback"
    torch.manual_seed(14)
    out = {}
    for name, (B, C, h, w, r) in CASES.items():
        f0, f1 = torch.randn(B, C, h, w), torch.randn(B, C, h, w)
        gx = torch.linspace(-1 + 1 / w, 1 - 1 / w, w)
        gy = torch.linspace(-1 + 1 / h, 1 - 1 / h, h)
        grid = torch.stack(torch.meshgrid(gx, gy, indexing="xy"), dim=-1)[None].expand(B, h, w, 2)
        warp = grid + 0.3 * torch.randn(B, h, w, 2)
        with torch.no_grad():
            corr = mod.local_correlation(f0, f1, r, warp, None)
        assert corr.shape == (B, (2 * r + 1) ** 2, h, w) and corr.dtype == torch.float32
        out[name + "_feature0"], out[name + "_feature1"] = f0.numpy(), f1.numpy()
        out[name + "_warp"], out[name + "_corr"], out[name + "_radius"] = warp.numpy(), corr.numpy(), np.int32(r)
    dst = os.path.join(HERE, "g14_local_corr.npz")
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
