"""The stages behind triangulation at the sizes a production run gives them, where their launches change behaviour - each regime is asserted
on plain integer arithmetic, so a change of the plan constants (cloud_plan() in csrc/lfd_api.hip, the one-workgroup scans) makes a test say so.

Stages on the final cloud (voxel, consensus, free-space, fuse, kNN, cap), one HipDensifier, the stages interleaved in its shared workspace:
  n =   266 241   1041 workgroups: the min / max pass is capped at 1024 and strides, the compaction tail's scan walks two counts per thread
  n = 1 052 673   4113 workgroups: every kernel launched with min(n_wg, 4096) workgroups runs a second iteration of its stride loop
  n = 4 198 401   1026 chunks of 4096: G is capped, the chunk grows to 4608 (nine scatter rounds of 512), G is recomputed to 912
Stages on a batch's points (support filter, plain and weighted re-triangulation, depth-sigma gate, normals), on the collected points and on the
launch's own buffers:
  four references of 288 x 288   capacity 331 776, 1296 workgroups: lfd_compact_scan_kernel, the gates' shared scan, walks two counts per thread
  fourteen references of 6 x 8   a workgroup stages the constants of seven references one after the other, a dead reference among them

Every output is held to the rule of the stage's own test file, through that file's helper where it has one: bit-equal to the CPU twin given the
same arrays (fuse normals and point normals within one f32 ulp, the re-triangulation's and the gate's rules as written there),
lfd_voxel_downsample bit-equal to the NumPy branch of densify._voxel_downsample.  The twin compacts in a sequential loop and finds a point's reference by walking the offsets: it shares none of the
machinery these sizes reach."""
import dataclasses
import sys

import numpy as np
import pytest
import torch

import normals_ref as nr
import support_scene as sc
import wrefine_scene as ws
from lichtfeld_densification_plugin_amd import densify
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from test_gpu_cap import three
from test_gpu_cloud_workspace import scene
from test_gpu_consensus import both as consensus_both
from test_gpu_depth_sigma import compare as sigma_compare
from test_gpu_depth_sigma import gap_threshold, ulps
from test_gpu_freespace import both as freespace_both
from test_gpu_fuse import bits, within_one_ulp
from test_gpu_fuse import both as fuse_both
from test_gpu_gaussians import both as knn_both
from test_gpu_refine import compare as refine_compare
from test_gpu_support_filter import compare as support_compare
from test_gpu_wrefine import compare as wrefine_compare

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TAU, THR = 1.6, ws.THR
PLANE = (64, 41)

N_SCAN = 266_241
N_STRIDE = 1_052_673
N_CAP = 4_198_401
# cell sizes: about the median nearest-neighbour distance of the cloud - the square root of the median of the twin's knn_dist2 (the mean squared
# distance to the three nearest) is 0.0031 for scene(N_SCAN, 5, seed=43) and 0.0019 for scene(N_STRIDE, 5, seed=44)
CELL = {257: 0.004, N_SCAN: 0.003, N_STRIDE: 0.002}
BUDGET = {257: 64, N_SCAN: 16_001, N_STRIDE: N_STRIDE // 16}


@pytest.fixture(scope="module")
def dens():
    d = hb.HipDensifier(DEV)
    d.upload_cameras(sc.cameras())
    yield d
    d.close()


@pytest.fixture(scope="module")
def twin():
    d = hb.HostDensifier(16)
    d.upload_cameras(sc.cameras())
    yield d
    d.close()


@pytest.fixture(autouse=True)
def numpy_branch(monkeypatch):
    """the reference of the voxel filter is the NumPy branch, whatever is installed"""
    monkeypatch.setitem(sys.modules, "open3d", None)


# ---- stages on the final cloud --------------------------------------------------------------------------------------------------------------------
def run_voxel(dens, twin, s, n):
    exp_x, exp_c = densify._voxel_downsample(s["xyz"], s["rgb"], CELL[n])
    got_x, got_c = dens.voxel_downsample(torch.from_numpy(s["xyz"]).to(DEV), torch.from_numpy(s["rgb"]).to(DEV), CELL[n])
    assert got_x.dtype == torch.float32 and got_c.dtype == torch.float32
    np.testing.assert_array_equal(got_x.cpu().numpy(), exp_x)
    np.testing.assert_array_equal(got_c.cpu().numpy(), exp_c)
    assert n == 257 or 1 < got_x.shape[0] < n
    return [got_x, got_c]


def run_consensus(dens, twin, s, n):
    d = consensus_both(dens, twin, s["holes"], s["rgb"], s["err"], s["counts"], 2.0 * CELL[n], 1, True)
    assert n == 257 or 0 < int(d[0].shape[0]) < n
    return [d[0], d[1], d[2], d[3], d[4]]


def run_freespace(dens, twin, s, n):
    d = freespace_both(dens, twin, s["holes"], s["counts"], s["P"], s["wh"], PLANE, 0.02, 1, True)
    assert n == 257 or 0 < int(d[0].shape[0]) < n
    return list(d[:6])


def run_fuse(dens, twin, s, n):
    d, nv = fuse_both(dens, twin, s["xyz"], s["nrm"], s["rgb"], CELL[n], f"{n} points")
    assert n == 257 or 1 < nv < n
    return list(d) + [np.array([nv])]


def run_knn(dens, twin, s, n):
    d, stats = knn_both(dens, twin, s.get("xyz_knn", s["xyz"]))
    assert d.shape == (n,) and (n == 257 or 0 < stats[3] < n // 10)   # the far points, and only they, are left to the brute-force pass
    return [d, np.array(stats, np.float64)]


def run_cap(dens, twin, s, n):
    keep, stats = three(dens, twin, s["xyz"], s["err"], BUDGET[n])
    assert keep.size == BUDGET[n] < n                                # exactly its budget
    return [keep, np.array(stats, np.float64)]


STAGES = {"voxel": run_voxel, "consensus": run_consensus, "freespace": run_freespace, "fuse": run_fuse, "knn": run_knn, "cap": run_cap}


def test_cloud_stages_past_the_scan_boundary(dens, twin):
    n = N_SCAN
    n_wg = (n + 255) // 256
    assert n_wg == 1041 > 1024                                       # n_part = min(1024, n_wg): the min / max pass strides
    assert (n_wg + 1023) // 1024 == 2                                # the compaction tail's scan: two counts per thread, idle threads behind n_wg
    assert n_wg <= 4096 and (n + 4095) // 4096 <= 1024               # ... and neither of the other two boundaries
    small, large = scene(257, 3, seed=41), scene(n, 5, seed=43)
    first = {}
    # each round in another order (every stage finds the words of a different predecessor); the small cloud lands in a workspace this size dirtied
    rounds = [(257, small, ["voxel", "consensus", "freespace", "fuse", "knn", "cap"]), (n, large, ["knn", "cap", "fuse", "consensus", "voxel", "freespace"]),
              (257, small, ["freespace", "knn", "voxel", "cap", "consensus", "fuse"])]
    for r, (size, s, order) in enumerate(rounds):
        for name in order:
            out = STAGES[name](dens, twin, s, size)
            if r == 0:
                first[name] = [bits(x).copy() if x is not None else None for x in out]
            if r == 2:                                                # the small cloud again, behind the large one: the bits of the first round
                for a, b in zip(first[name], out):
                    assert (a is None and b is None) or np.array_equal(a, bits(b)), name


@pytest.fixture(scope="module")
def stride_scene():
    """scene(N_STRIDE), made once.  Its 3 % far rows (31 338) are each finished by the kNN's brute-force pass, n distances apiece: 3e10 in all,
    some 24 s for a twin of 16 threads.  The kNN call alone gets ``xyz_knn``: the same cloud with all but 1000 of the far rows moved onto the
    ground beside another point - the same n, the same launches, some 4 s for the twin.  The other stages see the cloud as it is."""
    s = scene(N_STRIDE, 5, seed=44)
    far = np.abs(s["xyz"]).max(axis=1) > 2.0
    move, near = np.flatnonzero(far)[1000:], np.flatnonzero(~far)
    assert move.size > 20_000
    s["xyz_knn"] = s["xyz"].copy()
    s["xyz_knn"][move] = s["xyz"][near[:move.size]] + np.float32(0.001)
    return s


@pytest.mark.parametrize("name", ["consensus", "freespace", "fuse", "knn", "cap"])
def test_cloud_stages_past_the_stride_boundary(dens, twin, stride_scene, name):
    n = N_STRIDE
    assert (n + 255) // 256 == 4113 > 4096                           # grid = min(n_wg, 4096): i += gridDim.x * 256 runs a second time
    assert n - 4096 * 256 == 4097                                    # ... for the 4097 points behind the first sweep
    assert (n + 4095) // 4096 <= 1024                                # G is not capped yet
    STAGES[name](dens, twin, stride_scene, n)


def test_the_sort_past_the_cap_on_its_workgroups(dens):
    n = N_CAP
    assert (n + 4095) // 4096 == 1026 > 1024                         # G = min(1024, ...) is capped
    chunk = ((n + 1023) // 1024 + 511) // 512 * 512
    assert chunk == 4608 and chunk // 512 == 9 and (n + chunk - 1) // chunk == 912      # nine scatter rounds per workgroup, G recomputed
    rng = np.random.default_rng(12)
    xyz, rgb = rng.uniform(-5.0, 5.0, size=(n, 3)).astype(np.float32), rng.random((n, 3)).astype(np.float32)
    exp_x, exp_c = densify._voxel_downsample(xyz, rgb, 0.1)          # 100^3 voxels for 4.2 million points
    got_x, got_c = dens.voxel_downsample(torch.from_numpy(xyz).to(DEV), torch.from_numpy(rgb).to(DEV), 0.1)
    assert got_x.dtype == torch.float32 and got_c.dtype == torch.float32
    np.testing.assert_array_equal(got_x.cpu().numpy(), exp_x)
    np.testing.assert_array_equal(got_c.cpu().numpy(), exp_c)
    assert 1 < got_x.shape[0] < n // 3                               # many voxels of several points


# ---- stages on a batch's points ---------------------------------------------------------------------------------------------------------------------
def owned(res):
    """A collected result whose arrays are its own (collect hands out views of the buffers, which an in-place launch overwrites)."""
    return dataclasses.replace(res, xyz=res.xyz.clone(), rgb=res.rgb.clone(), err=res.err.clone(), cell=res.cell.clone(), slot=res.slot.clone(), _packed=None)


TINY_K = [(1, 2, 3)[i % 3] for i in range(14)]
TINY_DEAD = (0, 7, 13)
SCENES = {
    # name: (H, W, (reference, k, dead) per reference, depth step of the normals)
    "scale": (288, 288, [(10, 3, False), (17, 3, False), (24, 3, False), (31, 3, False)], 0.05),
    "tiny": (6, 8, [(3 + 2 * i, TINY_K[i], i in TINY_DEAD) for i in range(14)], 0.5),
}


class Launch:
    """One batch of the probe scene with its precision planes, on the device and on the host, and the buffers of its dense launch."""

    def __init__(self, dens, name):
        self.name = name
        self.H, self.W, self.spec, self.step = SCENES[name]
        made = [ws.reference_inputs(ref, k, self.H, self.W, device=DEV if name == "scale" else "cpu") for ref, k, _dead in self.spec]
        for ri, (_ref, _k, dead) in zip(made, self.spec):
            if dead:                                                  # the reference's own mask blanks it: the dense kernel has no candidate there
                ri.mask_a = torch.zeros((sc.MATCH, sc.MATCH), dtype=torch.uint8, device=ri.image.device)
        self.refs_h, self.refs_d = [ws.to_device(ri, "cpu") for ri in made], [ws.to_device(ri, DEV) for ri in made]
        self.batch, self.batch_h = hb.PreparedBatch(self.refs_d, sc.MATCH, sc.MATCH), hb.PreparedBatch(self.refs_h, sc.MATCH, sc.MATCH)
        self.out = hb.OutputBuffers(len(self.spec) * self.H * self.W, len(self.spec), self.batch.k, DEV)
        self.dens = dens
        self.src = None

    def fresh(self):
        """the dense launch into the buffers (again: a stage may have refined them in place); (buffers, the collected points, owning their arrays)"""
        self.dens.launch_dense(self.batch, sc.params(reproj_thresh=THR), self.out)
        self.dens.check_launches()
        with torch.cuda.stream(self.dens.stream):
            src = owned(self.out.collect())
        if self.src is None:
            self.src = src
            self.check_regime()
        assert sc.same_points(src, self.src)
        return self.out, src

    def check_regime(self):
        off, cap = np.asarray(self.src.ref_offsets), self.out.capacity
        if self.name == "scale":
            assert cap == 331_776 and (cap + 255) // 256 == 1296 and (1296 + 1023) // 1024 == 2      # the buffers: two counts per thread of a scan
            assert self.src.count > 262_144                           # ... and real counts behind entry 1024, for the collected points as well
            assert (((self.src.count + 255) // 256) + 1023) // 1024 == 2
        else:
            assert self.src.count <= 528 and cap == 672 and (cap + 255) // 256 == 3
            assert all(off[r] == off[r + 1] for r in TINY_DEAD) and all(off[r] < off[r + 1] for r in range(14) if r not in TINY_DEAD)
            crowded = False
            for b in range((self.src.count + 255) // 256):           # the 256 consecutive points of workgroup b
                lo, hi = 256 * b, min(256 * (b + 1), self.src.count)
                live = [r for r in range(14) if off[r] < off[r + 1] and off[r] < hi and off[r + 1] > lo]
                dead = [r for r in TINY_DEAD if lo < off[r] < hi]
                crowded = crowded or (len(live) >= 4 and len(dead) >= 1)
            assert crowded                                            # four or more references in one workgroup, a dead one strictly inside it


@pytest.fixture(scope="module", params=sorted(SCENES))
def launch(request, dens):
    return Launch(dens, request.param)


def test_support_filter(dens, twin, launch):
    out, src = launch.fresh()
    got, _sup = support_compare(dens, twin, launch.refs_d, src, 1)
    from_buffers, _sup = support_compare(dens, twin, launch.refs_d, src, 1, src_buffers=out)
    assert sc.same_points(got, from_buffers) and 0 < got.count < src.count
    if launch.name == "tiny":                                         # a k = 1 reference has no other neighbour: the filter empties it
        off_in, off_out = np.asarray(src.ref_offsets), np.asarray(got.ref_offsets)
        alone = [r for r in range(14) if TINY_K[r] == 1 and r not in TINY_DEAD]
        assert len(alone) == 4 and all(off_in[r] < off_in[r + 1] and off_out[r] == off_out[r + 1] for r in alone)
        assert any(off_out[r] < off_out[r + 1] for r in range(14) if TINY_K[r] > 1)


def test_plain_re_triangulation(dens, twin, launch):
    out, src = launch.fresh()
    _st, n_acc, n_fall = refine_compare(dens, twin, launch.refs_h, launch.refs_d, src, buffers=out)
    assert n_acc > 100 and n_fall > 10


def test_weighted_re_triangulation(dens, twin, launch):
    out, src = launch.fresh()
    _st, n_acc, n_fall, n_wacc = wrefine_compare(dens, twin, launch.refs_h, launch.refs_d, src, TAU, buffers=out)
    assert n_wacc > 100 and n_fall > 10


def test_depth_sigma_gate_with_the_refinement_s_status(dens, twin, launch):
    out, src = launch.fresh()
    sigma_compare(dens, twin, launch.refs_h, launch.refs_d, src, TAU, "status")
    # the launch's own buffers: refined in place, then through the gate with that launch's status, nothing read back in between
    _same, status = dens.refine_multiview(launch.batch, out, TAU, THR, with_status=True, precision=True)
    kw = dict(refine_status=status, support_thresh_px=TAU, with_sigma=True)
    with torch.cuda.stream(dens.stream):
        refined_h = sc.result_on_host(owned(out.collect()))
    kw_h = dict(kw, refine_status=status[:src.count].cpu().contiguous())
    _r0, sigma_h, _o = twin.depth_sigma_filter(launch.batch_h, refined_h, 0.0, **kw_h)
    mx = gap_threshold(sigma_h.numpy())
    want, _s, want_out = twin.depth_sigma_filter(launch.batch_h, refined_h, mx, **kw_h)
    got, sigma, sigma_out = dens.depth_sigma_filter(launch.batch, out, mx, **kw)
    assert isinstance(got, hb.OutputBuffers) and got is not out and got.sigma_filtered
    dens.check_launches()
    with torch.cuda.stream(dens.stream):
        res = got.collect()
    sg, sh = sigma[:src.count].cpu().numpy(), sigma_h.numpy()
    fin = np.isfinite(sh)
    assert not np.isnan(sg).any() and np.array_equal(np.isposinf(sg), np.isposinf(sh)) and int(ulps(sg[fin], sh[fin]).max()) <= 1
    assert sc.same_points(sc.result_on_host(res), want), "the compacted arrays, offsets or per-slot counts differ from the twin's"
    assert np.array_equal(bits(sigma_out[:res.count]), bits(want_out))
    assert res.sigma_in == src.count and 0 < res.count < src.count


def test_normals_at_radius_three(dens, twin, launch):
    out, src = launch.fresh()
    R, n = 3, src.count
    counters = torch.zeros(2, dtype=torch.int64, device=DEV)
    same, status = dens.estimate_normals(launch.batch, out, R, launch.step, THR, with_status=True, counters=counters)
    dens.check_launches()
    assert same is out and out.normals_valid
    nd, sd = out.normals[:n].cpu().numpy(), status[:n].cpu().numpy()
    got, status_c = dens.estimate_normals(launch.batch, src, R, launch.step, THR, with_status=True)      # the collected points: the same bits
    assert torch.equal(status_c, status[:n]) and np.array_equal(bits(got.normals), bits(nd))
    fitted = (sd & 0x80) != 0
    assert counters.cpu().tolist() == [int(fitted.sum()), n - int(fitted.sum())] and fitted.sum() > 100 and (~fitted).sum() > 10
    want, status_t = twin.estimate_normals(launch.batch_h, sc.result_on_host(src), R, launch.step, THR, with_status=True)
    nt, stt = want.normals.numpy(), status_t.numpy()
    differ = sd != stt
    print(f"{launch.name}: {n} points, {int(fitted.sum())} fitted, statuses that differ from the twin's: {int(differ.sum())}, normal components that "
          f"differ: {int((bits(nd) != bits(nt)).sum())} of {nd.size}")
    if differ.any():                                                  # the probe scene is noisy: only where the f64 reference puts a decision in band
        ref = nr.over_references(sc.cameras(), launch.refs_h, sc.result_on_host(src), sc.MATCH, sc.MATCH, R, launch.step, THR)
        assert not (differ & ~ref["flagged"]).any()
    assert within_one_ulp(nd[~differ], nt[~differ]).all()
