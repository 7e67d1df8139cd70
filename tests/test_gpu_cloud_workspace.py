"""The five stages on the final cloud - lfd_voxel_downsample, lfd_consensus_filter, lfd_freespace_filter, lfd_fuse_oriented, lfd_knn_dist2 - carve
ONE workspace of the context.  One HipDensifier runs them interleaved at n = 257, then 70 001, then 257 again: the large size gives 18 radix
workgroups and three or more passes at a cell of about one median spacing, and the return to 257 runs every stage in a buffer that another
stage sized and dirtied.  Every output is compared as the stage's own test file compares it: bit-equal to the CPU twin given the same arrays
(fuse normals within one f32 ulp), lfd_voxel_downsample bit-equal to the NumPy branch of densify._voxel_downsample."""
import sys

import numpy as np
import pytest
import torch

import freespace_scene as fs
import fuse_ref
from lichtfeld_densification_plugin_amd import densify
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from test_gpu_consensus import both as consensus_both
from test_gpu_freespace import both as freespace_both
from test_gpu_fuse import bits
from test_gpu_fuse import both as fuse_both
from test_gpu_gaussians import both as knn_both

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CELL = 0.004            # about the median nearest-neighbour distance of the 70 001-point cloud (0.0037)
PLANE = (64, 41)


@pytest.fixture(scope="module")
def dens():
    d = hb.HipDensifier(DEV)
    yield d
    d.close()


@pytest.fixture(scope="module")
def twin():
    d = hb.HostDensifier(16)
    yield d
    d.close()


def scene(n, n_refs, seed):
    """a clustered cloud of n_refs ring cameras (a few points far outside, so the grid is wide), normals around +z with a third of them flipped
    and a few unusable, colours; and the same cloud with a few non-finite rows for the two stages that accept them"""
    xyz, counts, P, wh = fs.ring_cloud(n_refs, n, seed, clustered=True)
    rng = np.random.default_rng(seed + 1000)
    nrm = fuse_ref.unit(np.array([0.0, 0.0, 1.0]) + rng.normal(0.0, 0.3, (n, 3)))
    nrm[rng.random(n) < 0.33] *= -1.0
    nrm = nrm.astype(np.float32)
    nrm[rng.choice(n, 6, replace=False)] = np.array([[np.nan, 0, 1], [0, 0, 0], [np.inf, 0, 0]] * 2, np.float32)
    rgb = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
    holes = xyz.copy()
    at = rng.choice(n, 9, replace=False)
    holes[at[:3], 0], holes[at[3:6], 2], holes[at[6:], 1] = np.nan, np.inf, -np.inf
    return dict(xyz=xyz, holes=holes, nrm=nrm, rgb=rgb, err=rng.uniform(0.0, 2.0, n).astype(np.float32), counts=counts, P=P, wh=wh)


def run_voxel(dens, twin, s):
    exp_x, exp_c = densify._voxel_downsample(s["xyz"], s["rgb"], CELL)
    got_x, got_c = dens.voxel_downsample(torch.from_numpy(s["xyz"]).to(DEV), torch.from_numpy(s["rgb"]).to(DEV), CELL)
    assert got_x.dtype == torch.float32 and got_c.dtype == torch.float32
    np.testing.assert_array_equal(got_x.cpu().numpy(), exp_x)
    np.testing.assert_array_equal(got_c.cpu().numpy(), exp_c)
    return [got_x, got_c]


def run_consensus(dens, twin, s):
    d = consensus_both(dens, twin, s["holes"], s["rgb"], s["err"], s["counts"], 2.0 * CELL, 1, True)
    return [d[0], d[1], d[2], d[3], d[4]]


def run_freespace(dens, twin, s):
    d = freespace_both(dens, twin, s["holes"], s["counts"], s["P"], s["wh"], PLANE, 0.02, 1, True)
    return list(d[:6])


def run_fuse(dens, twin, s):
    d, nv = fuse_both(dens, twin, s["xyz"], s["nrm"], s["rgb"], CELL, "shared workspace")
    return list(d) + [np.array([nv])]


def run_knn(dens, twin, s):
    d, stats = knn_both(dens, twin, s["xyz"])
    return [d, np.array(stats, np.float64)]


STAGES = {"voxel": run_voxel, "consensus": run_consensus, "freespace": run_freespace, "fuse": run_fuse, "knn": run_knn}


def test_the_five_stages_interleaved_in_one_workspace(dens, twin, monkeypatch):
    monkeypatch.setitem(sys.modules, "open3d", None)                   # the reference of the voxel filter is the NumPy branch
    small, large = scene(257, 3, seed=41), scene(70001, 5, seed=42)
    lo, hi = large["xyz"].min(axis=0).astype(np.float64), large["xyz"].max(axis=0).astype(np.float64)
    assert (70001 + 4095) // 4096 == 18                                 # radix workgroups (chunks of 4096)
    assert np.prod(np.floor((hi - lo) / CELL) + 1.0) > 2.0 ** 16       # three or more 8-bit passes
    first = {}
    # each round in another order: every stage finds the words of a different predecessor
    rounds = [(small, ["voxel", "consensus", "freespace", "fuse", "knn"]), (large, ["knn", "fuse", "consensus", "voxel", "freespace"]),
              (small, ["freespace", "knn", "voxel", "consensus", "fuse"])]
    for r, (s, order) in enumerate(rounds):
        for name in order:
            out = STAGES[name](dens, twin, s)
            if r == 0:
                first[name] = [bits(x).copy() if x is not None else None for x in out]
            if r == 1:
                assert out[0].shape[0] > 0                              # no stage of the large round is trivially empty
            if r == 2:                                                  # the small cloud again, behind the large one: the bits of the first round
                for a, b in zip(first[name], out):
                    assert (a is None and b is None) or np.array_equal(a, bits(b)), name
