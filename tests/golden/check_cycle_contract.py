#!/usr/bin/env python3
"""The backward warp the forward-backward filter consumes, against the REAL RoMaV2 class - development container only, like
check_matcher_contract.py: the reference tree does not exist on the GPU box, and nothing of it is copied.

    python tests/golden/check_cycle_contract.py [--write]      -> tests/golden/g16_cycle_contract.json

With the stubs and the seeded weights of check_matcher_contract.py, on the CPU:
  fast   (the model runs one way): ``RomaMatcher.set_backward_warp(True)`` forces ``model.bidirectional`` for the duration of a call.  The forward
         outputs - ``warp_AB`` and the certainty - must be BIT-EQUAL with and without the forced backward pass, one pair per forward and several
         (the second is reported when it is not: batched arithmetic may round differently, as check_matcher_contract.py records), and the flag
         must be False again afterwards.
  high   (the plugin's bidirectional preset): the third element of the triples is the model's own ``warp_BA`` - what ``RoMaV2.match`` returns for
         the same pair - bit for bit, and the flag is left alone."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    install_stubs()
    ours = importlib.import_module("lichtfeld_densification_plugin_amd.core.matcher")
    imA, imB1, imB2 = _images(3, [(97, 75), (120, 80), (64, 96)])
    record = {"what": "RomaMatcher.set_backward_warp against the real RoMaV2 class, seeded weights, CPU", "torch": torch.__version__}

    t0 = time.time()
    entry = {}
    for ppf in (1, 2):
        m = _build(ours.RomaMatcher, "fast", pairs_per_forward=ppf)
        assert m.model.bidirectional is False
        plain = m.match_grids_batch(imA, [imB1, imB2])
        m.set_backward_warp(True)
        forced = m.match_grids_batch(imA, [imB1, imB2])
        assert m.model.bidirectional is False, "model.bidirectional was not restored"
        assert all(len(p) == 2 for p in plain) and all(len(t) == 3 for t in forced)
        H, W = plain[0][1].shape
        assert all(tuple(t[2].shape) == (H, W, 2) and bool(torch.isfinite(t[2]).all()) for t in forced)
        exact = all(torch.equal(p[0], t[0]) and torch.equal(p[1], t[1]) for p, t in zip(plain, forced))
        dw = max(float((p[0] - t[0]).abs().max()) for p, t in zip(plain, forced))
        dc = max(float((p[1] - t[1]).abs().max()) for p, t in zip(plain, forced))
        entry[f"pairs_per_forward_{ppf}"] = {"forward_outputs": "bit-identical with and without the forced backward pass" if exact else
                                             f"NOT bit-identical: max |d warp| {dw:.3e}, max |d cert| {dc:.3e}",
                                             "warp_AB_sha256": [_sha(p[0]) for p in plain], "warp_BA_sha256": [_sha(t[2]) for t in forced]}
        if ppf == 1:
            assert exact, f"fast: forcing the backward pass changes the forward outputs ({dw}, {dc})"
        m.close()
    entry["grid"] = [int(H), int(W)]
    entry["seconds"] = round(time.time() - t0, 1)
    record["fast"] = entry
    print("fast", json.dumps(entry), flush=True)

    t0 = time.time()
    m = _build(ours.RomaMatcher, "high")
    assert m.model.bidirectional is True
    m.set_backward_warp(True)
    (w, c, b), = m.match_grids_batch(imA, [imB1])
    assert m.model.bidirectional is True
    with torch.inference_mode():
        preds = m.model.match(imA, imB1)
    own = preds["warp_BA"][0]
    assert torch.equal(w, preds["warp_AB"][0]), "high: the forward warp differs from RoMaV2.match's"
    assert b.shape == own.shape and torch.equal(b, own), "high: the triple's backward warp is not the model's own warp_BA"
    record["high"] = {"grid": [int(v) for v in c.shape], "warp_BA": "the model's own, bit-identical", "warp_BA_sha256": _sha(own),
                      "seconds": round(time.time() - t0, 1)}
    m.close()
    print("high", json.dumps(record["high"]), flush=True)
    if a.write:
        dst = os.path.join(HERE, "g16_cycle_contract.json")
        with open(dst, "w") as fh:
            json.dump(record, fh, indent=1, sort_keys=True)
            fh.write("\n")
        print("wrote", dst)


if __name__ == "__main__":
    main()
