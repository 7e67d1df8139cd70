"""bench.py --dump-outputs: the last step's survivors mapped back to the workload's reference order (the timed loop rotates the references
from batch to batch), and a sample that depends on the arguments alone.  No GPU: a stand-in for the output buffers."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _buffers(counts_by_workload_ref, rot):
    """Output of a batch that holds the references rotated by `rot`: every row carries its workload reference's index."""
    n = len(counts_by_workload_ref)
    order = [(p + rot) % n for p in range(n)]
    counts = [counts_by_workload_ref[g] for g in order]
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    tag = torch.cat([torch.full((c,), float(g)) for g, c in zip(order, counts)])
    res = SimpleNamespace(ref_offsets=offs, xyz=tag.view(-1, 1).repeat(1, 3), rgb=tag.view(-1, 1).repeat(1, 3) + 0.5, err=tag + 0.25)
    return SimpleNamespace(collect=lambda: res)


def test_dump_is_in_workload_order_whatever_the_rotation():
    counts = [3, 0, 5, 2, 7]
    for rot in range(5):
        a = bench.last_step_outputs(_buffers(counts, rot), rot, cells_per_ref=16)
        np.testing.assert_array_equal(a["points_per_reference"], np.array(counts, np.float64))
        np.testing.assert_array_equal(a["sample_references"], np.arange(5, dtype=np.float64))
        expect = np.concatenate([np.full(c, g, np.float32) for g, c in enumerate(counts)])
        np.testing.assert_array_equal(a["xyz"], np.repeat(expect[:, None], 3, axis=1))
        np.testing.assert_array_equal(a["rgb"], np.repeat(expect[:, None], 3, axis=1) + 0.5)
        np.testing.assert_array_equal(a["err"], expect + 0.25)
        assert a["points_per_reference"].dtype == np.float64 and a["xyz"].dtype == np.float32


def test_dump_sample_fits_the_budget_and_depends_on_the_arguments_only():
    cells = bench.DUMP_BUDGET_BYTES // (28 * 3)          # three whole references fit
    counts = [4, 1, 6, 2, 9, 3, 5]
    picks = []
    for rot in (0, 3):
        for scale in (1, 2):
            c = [x * scale for x in counts]
            a = bench.last_step_outputs(_buffers(c, rot), rot, cells_per_ref=cells)
            pick = a["sample_references"].astype(int)
            assert len(pick) == 3 and list(pick) == sorted(set(pick))
            np.testing.assert_array_equal(a["err"], np.concatenate([np.full(c[g], g + 0.25, np.float32) for g in pick]))
            picks.append(tuple(pick))
    assert len(set(picks)) == 1
