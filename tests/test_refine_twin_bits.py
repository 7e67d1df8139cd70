"""The twins of the support filter and of both re-triangulation calls give the recorded bits: SHA-256 of their outputs on the seeded probe scenes
(tests/support_scene.py, tests/wrefine_scene.py) against tests/golden/g18_refine_twin_bits.json, which was recorded from the build that still
had one copy of the per-point code per variant (``python tests/test_refine_twin_bits.py --record`` writes it again).  What folds those copies
must leave every hash where it is, on one thread and on sixteen."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (HERE, os.path.dirname(HERE)) if p not in sys.path]         # (for --record: pytest has both already)
import support_scene as sc
import wrefine_scene as ws
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

FIXTURE = os.path.join(HERE, "golden", "g18_refine_twin_bits.json")
THR = ws.THR


def sha(t) -> str:
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def scenes():
    """name -> (references, tau): the two probe scenes of the host tests, and ragged slots with masks, four-channel warps and an empty reference."""
    ragged = [ws.reference_inputs(ref, k, 24, 32, channels=4, masks=True) for ref, k in ((10, 3), (20, 1), (30, 3), (35, 2))]
    ragged[2].mask_a = torch.zeros((sc.MATCH, sc.MATCH), dtype=torch.uint8)
    return {"k3_64x48_c2": ([ws.reference_inputs(10, 3, 48, 64)], 1.6),
            "k8_37x29_c4": ([ws.reference_inputs(10, 8, 29, 37, channels=4)], 3.0),
            "ragged_masks_c4": (ragged, 1.6)}


def compute(n_threads: int) -> dict:
    twin = hb.HostDensifier(n_threads)
    twin.upload_cameras(sc.cameras())
    out = {}
    for name, (refs, tau) in scenes().items():
        batch = hb.PreparedBatch(refs, sc.MATCH, sc.MATCH)
        src = twin.triangulate_dense(batch, sc.params(reproj_thresh=THR))
        h = {"input": {"n": int(src.count), "xyz": sha(src.xyz), "err": sha(src.err), "cell": sha(src.cell), "slot": sha(src.slot)}}
        res, support = twin.support_filter(batch, src, 1, tau, with_support=True)
        h["support_filter"] = {"xyz": sha(res.xyz), "err": sha(res.err), "support": sha(support),
                               "ref_offsets_out": sha(np.asarray(res.ref_offsets, np.int64))}
        patched = [q.clone() for q in refs[0].precision]
        patched[1][10:20, 8:28] = torch.tensor([1.0, 5.0, 1.0])                  # indefinite
        patched[1][12, 10] = float("nan")
        planes = {"refine": None, "weighted_valid": batch,
                  "weighted_one_invalid_patch": hb.PreparedBatch([ws.with_planes(refs[0], patched)] + refs[1:], sc.MATCH, sc.MATCH),
                  "weighted_all_nan": hb.PreparedBatch([ws.filled(r, (float("nan"),) * 3) for r in refs], sc.MATCH, sc.MATCH)}
        for call, b in planes.items():
            counters = torch.zeros(2 if b is None else 3, dtype=torch.int64)
            r, status = twin.refine_multiview(batch if b is None else b, src, tau, THR, with_status=True, counters=counters, precision=b is not None)
            h[call] = {"xyz": sha(r.xyz), "err": sha(r.err), "status": sha(status), "counters": counters.tolist()}
        out[name] = h
    twin.close()
    return out


@pytest.mark.parametrize("n_threads", [1, 16])
def test_twins_give_the_recorded_bits(n_threads):
    with open(FIXTURE) as f:
        want = json.load(f)
    got = compute(n_threads)
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name]["input"] == want[name]["input"], f"{name}: the two-view points fed to the calls differ from the recorded ones"
        for call in want[name]:
            assert got[name][call] == want[name][call], (name, call)
    # the scenes reach both ends: points refined and fallen back everywhere, weighted rows only where every plane is valid
    for name in want:
        assert want[name]["refine"]["counters"][0] > 100 and want[name]["weighted_valid"]["counters"][2] > 100
        assert want[name]["weighted_all_nan"]["counters"] == want[name]["refine"]["counters"] + [0]
        assert 0 < want[name]["weighted_one_invalid_patch"]["counters"][2] < want[name]["weighted_valid"]["counters"][2]


if __name__ == "__main__":
    if "--record" in sys.argv:
        with open(FIXTURE, "w") as f:
            json.dump(compute(4), f, indent=1, sort_keys=True)
            f.write("\n")
    print(json.dumps(compute(4), indent=1, sort_keys=True))
