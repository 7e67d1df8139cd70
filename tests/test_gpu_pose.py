"""The pose refinement's statistics on the device (lfd_pose_accumulate through HipDensifier) against the NumPy reference of
tests/pose_ref.py and the CPU twin, every integer of the table.  Shapes: 16 x 16 cells (exactly one full workgroup) and 24 x 20 (480 cells:
the second workgroup is partly idle); k = 3, 5 and 9 (the three slot instantiations) with one reference below k; 2- and 4-channel warps; with
and without masks; NaN certainties, a certainty exactly at the threshold, NaN and infinite observations, targets outside the neighbour, a pair
with coincident centres; a residual exactly at pose_inlier_px; launch geometry; sentinels behind the table; and one driver run on the device
that writes the host backend's poses.json."""
import numpy as np
import pytest
import torch

import pose_ref
import pose_scene as ps
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LFD_ERR_STATE = 4
CERT, TABLE_PX, MATCH = 0.5, 1.5, 64
RECORDS = ps.cameras(ps.TABLE_WRONG)


@pytest.fixture(scope="module")
def dens():
    d = hb.HipDensifier(DEV)
    d.upload_cameras(RECORDS)
    yield d
    d.close()


@pytest.fixture(scope="module")
def twin():
    d = hb.HostDensifier(16)
    d.upload_cameras(RECORDS)
    yield d
    d.close()


def on_device(refs, cameras=RECORDS):
    return hb.PreparedBatch([ps.to_device(r, DEV) for r in refs], MATCH, MATCH, cameras=cameras)


@pytest.mark.parametrize("H,W,k,channels,masks,poisoned", [(16, 16, 3, 2, False, False), (24, 20, 3, 4, True, True), (24, 20, 5, 2, True, True),
                                                           (16, 16, 9, 4, False, True), (24, 20, 9, 2, False, False),
                                                           (16, 16, 5, 4, True, False)])
def test_device_equals_reference_and_twin(dens, twin, H, W, k, channels, masks, poisoned):
    refs = ps.batch_case(H, W, k, channels, masks, poisoned)
    want, per = pose_ref.table(RECORDS, refs, k, MATCH, MATCH, CERT, TABLE_PX)
    assert want[:, 0].sum() > 100 * k and want[:, 1].sum() > 0 and (want[:, 3] > 0).sum() >= 2 * k
    if poisoned:
        assert want[k - 1, 0] == 0 and want[k - 1, 1] == 0 and want[k - 1, 2] > 50      # the pair with coincident centres
    # a sentinel row behind the n_refs * k rows of the table
    table_all = torch.zeros((3 * k + 1, 32), dtype=torch.int64, device=DEV)
    table_all[3 * k] = -77
    table = dens.pose_accumulate(on_device(refs), CERT, TABLE_PX, table=table_all[:3 * k])
    host = twin.pose_accumulate(hb.PreparedBatch(refs, MATCH, MATCH, cameras=RECORDS), CERT, TABLE_PX)
    assert np.array_equal(table.cpu().numpy(), want) and np.array_equal(host.numpy(), want)
    assert (table_all[3 * k] == -77).all().item()
    # the row of the slot the second reference does not have stays zero; a second launch adds the same again
    if k > 1:
        assert (want[2 * k - 1] == 0).all()
    dens.pose_accumulate(on_device(refs), CERT, TABLE_PX, table=table)
    assert np.array_equal(table.cpu().numpy(), 2 * want)


def test_the_table_does_not_depend_on_launch_geometry(dens):
    refs = ps.batch_case(24, 20, 3, 2, True, True)
    want, _p = pose_ref.table(RECORDS, refs, 3, MATCH, MATCH, CERT, TABLE_PX)
    parts = [dens.pose_accumulate(on_device([r]), CERT, TABLE_PX).cpu().numpy() for r in refs]
    assert parts[1].shape == (2, 32)
    assert np.array_equal(parts[0], want[0:3]) and np.array_equal(parts[1], want[3:5]) and np.array_equal(parts[2], want[6:9])
    # the same reference three times in one launch: three equal blocks of rows
    three = dens.pose_accumulate(on_device([refs[2]] * 3), CERT, TABLE_PX).cpu().numpy()
    assert np.array_equal(three, np.concatenate([want[6:9]] * 3))


def test_a_residual_exactly_at_pose_inlier_px_is_an_outlier_on_the_device():
    recs, ri, deltas = ps.exact_rig()
    want, _per = pose_ref.table(recs, [ri], 1, 65, 65, CERT, ps.EXACT_PX)
    assert want[0, :3].tolist() == [5 * 8, 3 * 8, 0]
    d = hb.HipDensifier(DEV)
    try:
        d.upload_cameras(recs)
        table = d.pose_accumulate(hb.PreparedBatch([ps.to_device(ri, DEV)], 65, 65, cameras=recs), CERT, ps.EXACT_PX)
        assert np.array_equal(table.cpu().numpy(), want)
    finally:
        d.close()


def test_contexts_refuse_each_others_calls(dens, twin):
    refs = ps.batch_case(16, 16, 3, 2, False, False)
    table = hb.pose_table(3, 3, DEV)
    rc, _t = hb._pose_accumulate_call(dens._lib.lfd_pose_accumulate_host, dens._ctx, on_device(refs), CERT, 8.0, table, DEV)
    assert rc == LFD_ERR_STATE
    host_table = hb.pose_table(3, 3, torch.device("cpu"))
    rc, _t = hb._pose_accumulate_call(twin._lib.lfd_pose_accumulate, twin._ctx, hb.PreparedBatch(refs, MATCH, MATCH), CERT, 8.0, host_table,
                                      torch.device("cpu"))
    assert rc == LFD_ERR_STATE and int(host_table.abs().sum()) == 0
    torch.cuda.synchronize()
    assert int(table.abs().sum().item()) == 0


class Node:
    """A camera node as the GUI hands it to dense_init_from_lfs."""

    def __init__(self, cam):
        self.has_camera, self.camera_uid = True, cam.uid
        self.camera_width, self.camera_height = cam.width, cam.height
        self.camera_focal_x, self.camera_focal_y = float(cam.K[0, 0]), float(cam.K[1, 1])
        self.camera_R, self.camera_T = cam.R, cam.t.reshape(3)
        self.image_path, self.has_mask, self.mask_path = cam.image_path, False, None


@pytest.mark.parametrize("mode,refs_per_launch", [("dense", 0), ("sampled", 2)])
def test_the_driver_on_the_device_writes_the_host_backends_poses(tmp_path, mode, refs_per_launch):
    """One record rotated by 0.5 degrees, 0.5 px of matching noise: poses.json of the device run is the host backend's byte for byte - dense
    mode, and sampled mode through the asynchronous schedules, where a launch's table travels with its buffers until its result is
    committed."""
    import os

    import lichtfeld_densification_plugin_amd as lfd
    from lichtfeld_densification_plugin_amd import densify
    from lichtfeld_densification_plugin_amd.core import poses as pose_report
    cams = ps.write_scene(str(tmp_path / "scene"), (2, (0.5, 0.0, 0.0), (0.0, 0.0, 0.0)))
    nodes = [Node(c) for c in cams]
    recs = densify.extract_cameras_from_lfs(nodes)
    files = {}
    for backend in ("device", "host"):
        out = str(tmp_path / backend / "out.ply")
        os.makedirs(os.path.dirname(out))
        cfg = lfd.DensePipelineConfig(output_path=out, num_refs=1.0, nns_per_ref=3, seed=3, viz_interval=0, pack_workers=1, matches_per_ref=2500,
                                      backend=backend, triangulation_mode=mode, refs_per_launch=refs_per_launch if backend == "device" else 0,
                                      experimental={"pose_refine": "report"})
        kw = {"device": DEV} if backend == "device" else {}
        matcher = ps.Matcher(recs, device=DEV if backend == "device" else "cpu", noise_px=0.5)
        rc, msg = densify.dense_init_from_lfs(nodes, cfg, matcher=matcher, **kw)
        assert rc == 0, msg
        files[backend] = out
    text = {b: open(files[b] + ".poses.json", "rb").read() for b in files}
    assert text["device"] == text["host"]
    js = pose_report.from_json(text["device"].decode())
    assert len(js["pairs"]) == 24 and js["scene"]["usable_pairs"] == 24 and 0.3 < js["cameras"][2]["rotation_step_deg"] < 0.55
