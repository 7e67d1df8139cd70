"""The far-field shell on the device (lfd_far_accumulate / lfd_far_emit through HipDensifier) against the NumPy reference of
tests/far_ref.py and the CPU twin, exact.  Shapes: three references of 24 x 40 cells (960 cells: the fourth workgroup of a reference is
partial - 192 lanes - and the next reference starts in a workgroup of its own) with 1, 3 and 2 neighbours in a batch of k = 3; 2- and
4-channel warps; with and without mask_a / mask_b; NaN certainties, NaN and infinite observations, targets outside the neighbour; S = 32;
a camera whose optical axis is (1, 1, 0) / sqrt 2 with equal f32 entries (face ties); a narrow field at S = 8 in which all 3 x 960 cells fall
into one direction cell (full contention, the in-wave run reduction); k = 8 and 16 (the kernel's other slot counts); emit with too small a
capacity, a threshold above every count and an empty table; a second launch doubles the table; both contexts refuse each other's calls."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import colour_scene as cs
import far_ref
import far_scene as fs
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from lichtfeld_densification_plugin_amd.core.types import CameraRecord

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LFD_ERR_STATE, LFD_ERR_CAPACITY = 4, 3
TAU, CERT, VIEWS = 0.8, 0.5, 2
MATCH, H, W = 64, 24, 40


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def narrow_cameras():
    """Four cameras of a 0.2 degree field of view with the optical axis (1, 1, 0) / sqrt 2 - the f32 entries of that row of R are equal - and
    the principal point in the image's corner: the ray of camera pixel u = 0 has |d_0| == |d_1| exactly (a tie between the faces +x and +y,
    which the lower index wins), every other ray has |d_0| > |d_1|, and all of them lie within 0.005 of the axis: one direction cell at S = 8."""
    f, w, h = 120000.0, 400, 400
    K = np.array([[f, 0.0, 0.0], [0.0, f, 0.0], [0.0, 0.0, 1.0]])
    s = math.sqrt(0.5)
    out = []
    for i in range(4):
        fwd = np.array([s, s, 0.0])
        right = np.array([s, -s, 0.0])
        down = np.cross(fwd, right)
        R = np.stack([right, down, fwd], axis=0)
        c = np.array([0.05 * i, -0.05 * i, 0.0])
        out.append(CameraRecord.from_krt(i + 1, K, R, -R @ c, w, h, image_path=f"narrow/{i}.png"))
    return out


def narrow_refs(cams, channels=2):
    """Three references, every neighbour sees every cell at infinity: xb = xa (the cameras share their rotation), certainty 0.9.  With four
    channels the first three columns carry the A-coordinate -1 exactly: camera pixel u = 0, the tie."""
    ax = far_ref.axis(W)
    ay = far_ref.axis(H)
    ident = np.stack(np.meshgrid(ax, ay), axis=-1).astype(np.float32)
    if channels == 4:
        ident[:, :3, 0] = -1.0
    wp = ident if channels == 2 else np.concatenate([ident, ident], axis=-1)
    rng = np.random.default_rng(5)
    refs = []
    for r in range(3):
        nbrs = [c for c in range(4) if c != r]
        refs.append(hb.ReferenceInputs(ref_cam=r, nbr_cams=nbrs, cert=[torch.full((H, W), 0.9) for _ in nbrs],
                                       warp=[torch.from_numpy(wp.copy()) for _ in nbrs],
                                       image=torch.from_numpy(rng.integers(0, 256, (MATCH, MATCH, 3), dtype=np.uint8))))
    return refs


@pytest.fixture(scope="module")
def dens():
    d = hb.HipDensifier(DEV)
    d.upload_cameras(fs.cameras())
    yield d
    d.close()


@pytest.fixture(scope="module")
def twin():
    d = hb.HostDensifier(16)
    d.upload_cameras(fs.cameras())
    yield d
    d.close()


_made = {}


def case(channels, masks, hurt):
    key = (channels, masks, hurt)
    if key not in _made:
        refs = []
        for r, n in ((0, 1), (1, 3), (2, 2)):
            ri = fs.make(r, fs.others(r, n), H, W, match=MATCH, channels=channels, masks=masks).inputs
            if hurt:
                cert, warp = [c.clone() for c in ri.cert], [w.clone() for w in ri.warp]
                cert[0][2, 3:9] = float("nan")
                warp[0][3, 5:11, -2] = float("nan")
                warp[-1][4, 7:13, -1] = float("inf")
                warp[0][5, 2:8, -2] = 1.5
                if channels == 4:
                    warp[0][6, 1:5, 0] = float("nan")                  # the A-coordinate itself: d is NaN, the cell is not far
                ri = hb.ReferenceInputs(ref_cam=ri.ref_cam, nbr_cams=ri.nbr_cams, cert=cert, warp=warp, image=ri.image, mask_a=ri.mask_a,
                                        mask_b=ri.mask_b)
            refs.append(ri)
        _made[key] = refs
    return _made[key]


def on_device(refs):
    return hb.PreparedBatch([fs.to_device(r, DEV) for r in refs], MATCH, MATCH)


@pytest.mark.parametrize("channels,masks,hurt,S", [(2, False, False, 32), (4, True, True, 32), (2, True, True, 8), (4, False, False, 256)])
def test_device_equals_reference_and_twin(dens, twin, channels, masks, hurt, S):
    refs = case(channels, masks, hurt)
    want, want_counters, per = far_ref.accumulate(fs.cameras(), refs, MATCH, MATCH, TAU, CERT, VIEWS, S)
    assert want_counters.min() > 50 and all((~c["far"]).sum() > 50 for c in per)
    counters = torch.zeros(3, dtype=torch.int64, device=DEV)
    table = dens.far_accumulate(on_device(refs), TAU, CERT, VIEWS, S, counters=counters)
    host = twin.far_accumulate(hb.PreparedBatch(refs, MATCH, MATCH), TAU, CERT, VIEWS, S)
    assert np.array_equal(u64(table), want) and np.array_equal(u64(host), want)
    assert np.array_equal(counters.cpu().numpy(), want_counters)
    # a second launch adds the same again
    dens.far_accumulate(on_device(refs), TAU, CERT, VIEWS, S, table=table, counters=counters)
    assert np.array_equal(table.cpu().numpy(), 2 * want.view(np.int64)) and np.array_equal(counters.cpu().numpy(), 2 * want_counters)
    # emit: the twin's and the reference's bits
    centre, radius = np.array([0.3, -0.2, 0.1]), 12.5
    keys, xyz, rgb, nrm, smp = far_ref.emit(2 * want.view(np.int64), S, 2, centre, radius)
    got = dens.far_emit(table, S, 2, centre, radius, with_normals=True)
    assert keys.size > 5
    for g, w_ in zip(got[:3], (xyz, rgb, nrm)):
        assert np.array_equal(cs.bits(g), cs.bits(w_))
    assert np.array_equal(got[3].cpu().numpy(), smp)


@pytest.mark.parametrize("k", [8, 16])
def test_the_other_slot_counts(dens, k):
    """References of k neighbours drawn (with repetition) from the rig's other cameras: the kernel's 8- and 16-slot instantiations."""
    refs = []
    for r in (0, 3):
        nbrs = [fs.others(r, 3)[j % 3] for j in range(k)]
        refs.append(fs.make(r, nbrs, H, W, match=MATCH).inputs)
    want, want_counters, _per = far_ref.accumulate(fs.cameras(), refs, MATCH, MATCH, TAU, CERT, VIEWS, 32)
    counters = torch.zeros(2, dtype=torch.int64, device=DEV)
    table = dens.far_accumulate(on_device(refs), TAU, CERT, VIEWS, 32, counters=counters)
    assert np.array_equal(u64(table), want) and np.array_equal(counters.cpu().numpy(), want_counters) and want_counters.min() > 50


@pytest.mark.parametrize("channels", [2, 4])
def test_full_contention_and_face_ties(channels):
    cams = narrow_cameras()
    assert cams[0].R[2, 0] == cams[0].R[2, 1]                          # equal f32 entries
    refs = narrow_refs(cams, channels)
    want, want_counters, per = far_ref.accumulate(cams, refs, MATCH, MATCH, TAU, CERT, VIEWS, 8)
    assert np.array_equal(want_counters, [H * W] * 3)
    rows = np.nonzero(want[:, 6])[0]
    assert rows.size == 1 and int(want[rows[0], 6]) == 3 * H * W       # one direction cell takes every sample
    d = per[0]["d"]
    assert (np.abs(d[:, 0]) > np.abs(d[:, 1])).any()
    if channels == 4:
        assert (np.abs(d[:, 0]) == np.abs(d[:, 1])).sum() == 3 * H and int(per[0]["key"].min()) // 64 == 0      # the ties are face 0's
    dens = hb.HipDensifier(DEV)
    try:
        dens.upload_cameras(cams)
        batch = hb.PreparedBatch([fs.to_device(r, DEV) for r in refs], MATCH, MATCH)
        counters = torch.zeros(3, dtype=torch.int64, device=DEV)
        table = dens.far_accumulate(batch, TAU, CERT, VIEWS, 8, counters=counters)
        assert np.array_equal(u64(table), want) and np.array_equal(counters.cpu().numpy(), want_counters)
        # the same through finer cells: the ties decide faces, runs break inside waves
        want32, _c, _p = far_ref.accumulate(cams, refs, MATCH, MATCH, TAU, CERT, VIEWS, 512)
        assert np.count_nonzero(want32[:, 6]) > 1
        assert np.array_equal(u64(dens.far_accumulate(batch, TAU, CERT, VIEWS, 512)), want32)
    finally:
        dens.close()


def test_emit_capacity_threshold_and_empty_table(dens):
    refs = case(2, False, False)
    S = 32
    table = dens.far_accumulate(on_device(refs), TAU, CERT, VIEWS, S)
    centre = np.zeros(3)
    full = dens.far_emit(table, S, 1, centre, 5.0, with_normals=True)
    n = int(full[0].shape[0])
    assert n > 20
    rc, n_out, xyz, rgb, nrm, smp = hb._far_emit_call(dens._lib.lfd_far_emit, dens._ctx, table, S, 1, centre, 5.0, True, n - 7, DEV)
    torch.cuda.synchronize()
    assert rc == LFD_ERR_CAPACITY and n_out == n and xyz.shape[0] == n - 7
    for a, b in zip((xyz, rgb, nrm), full[:3]):
        assert np.array_equal(cs.bits(a), cs.bits(b[:n - 7]))
    assert np.array_equal(smp.cpu().numpy(), full[3][:n - 7].cpu().numpy())
    top = int(table[:, 6].max().item())
    assert dens.far_emit(table, S, top + 1, centre, 5.0)[0].shape[0] == 0
    assert dens.far_emit(table, S, top, centre, 5.0)[0].shape[0] >= 1
    assert dens.far_emit(hb.far_table(8, DEV), 8, 1, centre, 5.0)[0].shape[0] == 0


def test_contexts_refuse_each_others_calls(dens, twin):
    refs = case(2, False, False)
    table = hb.far_table(8, DEV)
    rc, _t = hb._far_accumulate_call(dens._lib.lfd_far_accumulate_host, dens._ctx, on_device(refs), TAU, CERT, VIEWS, 8, table, None, DEV)
    assert rc == LFD_ERR_STATE
    n_out = C.c_int64(0)
    c3 = (C.c_double * 3)(0.0, 0.0, 0.0)
    assert dens._lib.lfd_far_emit_host(dens._ctx, table.data_ptr(), 8, 1, c3, 1.0, None, None, None, None, 0, C.byref(n_out)) == LFD_ERR_STATE
    host_table = hb.far_table(8, torch.device("cpu"))
    rc, _t = hb._far_accumulate_call(twin._lib.lfd_far_accumulate, twin._ctx, hb.PreparedBatch(refs, MATCH, MATCH), TAU, CERT, VIEWS, 8, host_table,
                                     None, torch.device("cpu"))
    assert rc == LFD_ERR_STATE and int(host_table.abs().sum()) == 0


class Node:
    """A camera node as the GUI hands it to dense_init_from_lfs."""

    def __init__(self, cam):
        self.has_camera, self.camera_uid = True, cam.uid
        self.camera_width, self.camera_height = cam.width, cam.height
        self.camera_focal_x, self.camera_focal_y = float(cam.K[0, 0]), float(cam.K[1, 1])
        self.camera_R, self.camera_T = cam.R, cam.t.reshape(3)
        self.image_path, self.has_mask, self.mask_path = cam.image_path, False, None


@pytest.mark.parametrize("mode,refs_per_launch,exp", [("dense", 0, {"far_shell": "merge"}), ("sampled", 2, {"far_shell": "file", "far_shell_radius": 50.0}),
                                                      ("sampled", 1, {"far_shell": "file", "far_shell_radius": 50.0})])
def test_the_driver_on_the_device_writes_the_host_backends_shell(tmp_path, mode, refs_per_launch, exp):
    """Dense mode, 'merge', automatic radius: the whole file - cloud, then shell - and the json are the host backend's byte for byte (the
    radius comes from the cloud where it lives).  Sampled mode goes through the asynchronous schedules, where a launch's table travels with
    its buffers until its result is committed: the shell file and the json are the host backend's (a fixed radius: the two backends draw
    different samples of the same ground)."""
    import json
    import os

    import lichtfeld_densification_plugin_amd as lfd
    from lichtfeld_densification_plugin_amd import densify
    cams = fs.write_scene(str(tmp_path / "scene"))
    nodes = [Node(c) for c in cams]
    recs = densify.extract_cameras_from_lfs(nodes)
    files = {}
    for backend in ("device", "host"):
        out = str(tmp_path / f"{backend}.ply")
        cfg = lfd.DensePipelineConfig(output_path=out, num_refs=0.75, nns_per_ref=3, seed=3, viz_interval=0, pack_workers=1, matches_per_ref=2500,
                                      backend=backend, triangulation_mode=mode, refs_per_launch=refs_per_launch if backend == "device" else 0,
                                      experimental=exp)
        kw = {"device": DEV} if backend == "device" else {}
        rc, msg = densify.dense_init_from_lfs(nodes, cfg, matcher=fs.Matcher(recs, device=DEV if backend == "device" else "cpu"), **kw)
        assert rc == 0, msg
        files[backend] = out
    js = {b: json.load(open(files[b] + ".shell.json")) for b in files}
    assert js["device"] == js["host"] and js["device"]["cells_kept"] > 200 and js["device"]["far_cells_with_a_point"] == 0
    assert len(js["device"]["far_cells"]) == 3 and min(js["device"]["far_cells"].values()) > 10000
    if exp["far_shell"] == "merge":
        assert open(files["device"], "rb").read() == open(files["host"], "rb").read()
    else:
        shells = [os.path.splitext(files[b])[0] + "_shell.ply" for b in ("device", "host")]
        assert open(shells[0], "rb").read() == open(shells[1], "rb").read()
