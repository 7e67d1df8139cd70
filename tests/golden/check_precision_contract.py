#!/usr/bin/env python3
"""The precision planes the precision-weighted re-triangulation consumes, against the REAL RoMaV2 class - development container
only, like check_cycle_contract.py: the reference tree does not exist on the GPU box, and nothing of it is copied.

    python tests/golden/check_precision_contract.py [--write]      -> tests/golden/g17_precision_contract.json

With the stubs and the seeded weights of check_matcher_contract.py, on the CPU, for the presets fast and high:
  - ``RomaMatcher.set_precision(True)`` turns the pairs / triples into 4-tuples (warp, cert, warp_BA or None, precision); warp and certainty are
    BIT-EQUAL with the flag on and off (one pair per forward; fast also with two, where the 4-tuples must equal that mode's own pairs);
  - the plane (H, W, 3) f32 equals the entries [0,0], [0,1], [1,1] of the model's own ``preds["precision_AB"]`` - what ``RoMaV2.match`` returns
    for the same pair - divided by the documented factors ``precision_scale()``: rx rx, rx ry, ry ry with rx = (w_match - 1) / W_stage;
  - the plane is positive definite (p00 > 0, p11 > 0, p00 p11 - p01^2 > 0 in f64) wherever the model's matrix is."""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from check_matcher_contract import _build, _images, _sha, install_stubs  # noqa: E402


def _pd(a, b, c):
    a, b, c = a.double(), b.double(), c.double()
    return (a > 0) & (c > 0) & (a * c - b * b > 0)


def _check_plane(m, q, P):
    """q: our (H, W, 3) plane; P: the model's (H, W, 2, 2).  Returns the share of positive definite cells."""
    rx, ry = m.precision_scale()
    assert q.dtype == torch.float32 and q.is_contiguous() and tuple(q.shape) == tuple(P.shape[:2]) + (3,)
    want = torch.stack([P[..., 0, 0] / (rx * rx), P[..., 0, 1] / (rx * ry), P[..., 1, 1] / (ry * ry)], dim=-1).to(torch.float32)
    assert torch.equal(q, want), "the plane is not the model's entries divided by the documented factors"
    assert torch.equal(P[..., 0, 1], P[..., 1, 0]), "the model's matrix is not symmetric"
    model_pd, ours_pd = _pd(P[..., 0, 0], P[..., 0, 1], P[..., 1, 1]), _pd(q[..., 0], q[..., 1], q[..., 2])
    assert bool((ours_pd | ~model_pd).all()), "a cell the model has positive definite is not in the plane"
    return float(model_pd.double().mean()), float(ours_pd.double().mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    install_stubs()
    ours = importlib.import_module("lichtfeld_densification_plugin_amd.core.matcher")
    imA, imB1, imB2 = _images(3, [(97, 75), (120, 80), (64, 96)])
    record = {"what": "RomaMatcher.set_precision against the real RoMaV2 class, seeded weights, CPU", "torch": torch.__version__}

    for setting, ppfs in (("fast", (1, 2)), ("high", (1,))):
        t0 = time.time()
        entry = {}
        for ppf in ppfs:
            m = _build(ours.RomaMatcher, setting, pairs_per_forward=ppf)
            nbrs = [imB1, imB2] if setting == "fast" else [imB1]
            plain = m.match_grids_batch(imA, nbrs)
            m.set_precision(True)
            with_p = m.match_grids_batch(imA, nbrs)
            assert all(len(p) == 2 for p in plain) and all(len(t) == 4 and t[2] is None for t in with_p)
            assert all(torch.equal(p[0], t[0]) and torch.equal(p[1], t[1]) for p, t in zip(plain, with_p)), \
                f"{setting}: warp / certainty differ with the precision flag on"
            m.set_backward_warp(True)
            both = m.match_grids_batch(imA, nbrs)             # with the backward warp as well: element 2 is filled, the plane is the same
            assert all(len(t) == 4 and t[2] is not None and torch.equal(t[3], w[3]) for t, w in zip(both, with_p))
            m.set_backward_warp(False)
            shares = None
            if ppf == 1:
                with torch.inference_mode():
                    preds = m.model.match(imA, imB1)
                assert torch.equal(with_p[0][0], preds["warp_AB"][0])
                shares = _check_plane(m, with_p[0][3], preds["precision_AB"][0])
            else:
                one = _build(ours.RomaMatcher, setting, pairs_per_forward=1)
                one.set_precision(True)
                single = one.match_grids_batch(imA, nbrs)
                d = max(float((s_[3] - t[3]).abs().max() / s_[3].abs().max()) for s_, t in zip(single, with_p))
                entry["pairs_per_forward_2_vs_1_max_rel_diff"] = d
                one.close()
            m.set_precision(False)
            assert all(len(p) == 2 for p in m.match_grids_batch(imA, nbrs[:1]))
            rx, ry = m.precision_scale()
            entry[f"pairs_per_forward_{ppf}"] = {"forward_outputs": "bit-identical with the flag on and off", "scale": [rx, ry],
                                                 "plane_sha256": [_sha(t[3]) for t in with_p]}
            if shares is not None:
                entry[f"pairs_per_forward_{ppf}"].update(plane="the model's own entries / (rx rx, rx ry, ry ry), bit-identical",
                                                         positive_definite_share_model=shares[0], positive_definite_share_plane=shares[1])
            entry["grid"] = [int(v) for v in with_p[0][1].shape]
            m.close()
        entry["seconds"] = round(time.time() - t0, 1)
        record[setting] = entry
        print(setting, json.dumps(entry), flush=True)
    if a.write:
        dst = os.path.join(HERE, "g17_precision_contract.json")
        with open(dst, "w") as fh:
            json.dump(record, fh, indent=1, sort_keys=True)
            fh.write("\n")
        print("wrote", dst)


if __name__ == "__main__":
    main()
