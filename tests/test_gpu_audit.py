"""The epipolar audit on the device (lfd_epipolar_audit through HipDensifier) against the NumPy reference of tests/audit_ref.py
and the CPU twin, every element of the table and of the cell map.  Shapes: 16 x 16 cells (exactly one full workgroup) and 24 x 20 (480 cells:
the second workgroup is partly idle); k = 3, 5 and 9 (the three slot instantiations) with one reference below k; 2- and 4-channel warps; with
and without masks; NaN certainties, a certainty exactly at the threshold, NaN and infinite observations, targets outside the neighbour, a pair
whose F has rows 0 and 1 zero; the extremes of the in-wave aggregation; launch geometry; the per-lane variant; sentinels behind both outputs."""
import dataclasses

import numpy as np
import pytest
import torch

import audit_ref
import audit_scene as asc
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LFD_ERR_STATE = 4
CERT, MATCH = 0.5, 64


def u64(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.fixture(scope="module")
def dens():
    d = hb.HipDensifier(DEV)
    d.upload_cameras(asc.cameras())
    yield d
    d.close()


@pytest.fixture(scope="module")
def twin():
    d = hb.HostDensifier(16)
    d.upload_cameras(asc.cameras())
    yield d
    d.close()


def on_device(refs, cameras=None):
    return hb.PreparedBatch([asc.to_device(r, DEV) for r in refs], MATCH, MATCH, cameras=cameras)


def hurt(ri, poisoned):
    """The reference with its pairs' matrices attached and, if ``poisoned``, with every kind of entry the rule singles out."""
    cams = asc.cameras()
    cert, warp = [c.clone() for c in ri.cert], [w.clone() for w in ri.warp]
    a = cams[ri.ref_cam]
    fund = [np.asarray(hb.fundamental_from_world2cam(a.K, a.R, a.t, cams[n].K, cams[n].R, cams[n].t), np.float32) for n in ri.nbr_cams]
    if poisoned:
        cert[0][2, 3:9] = float("nan")
        cert[0][6, 1:15] = CERT
        warp[0][3, 5:11, -2] = float("nan")
        warp[-1][4, 7:13, -1] = float("inf")
        warp[0][5, 2:8, -2] = 1.5
        fund[-1] = fund[-1].copy()
        fund[-1][:2, :] = 0.0
    return dataclasses.replace(ri, cert=cert, warp=warp, fundamental=fund)


_made = {}


def case(H, W, k, channels, masks, poisoned):
    """Three references with k, k - 1 (at least 1) and k neighbours drawn (with repetition) from the rig's other cameras."""
    key = (H, W, k, channels, masks, poisoned)
    if key not in _made:
        refs = []
        for r, n in ((1, k), (4, max(1, k - 1)), (2, k)):
            near = asc.neighbours(r, 5)
            ri = asc.make(r, [near[j % 5] for j in range(n)], H, W, match=MATCH, channels=channels, masks=masks).inputs
            refs.append(hurt(ri, poisoned))
        _made[key] = refs
    return _made[key]


@pytest.mark.parametrize("H,W,k,channels,masks,poisoned", [(16, 16, 3, 2, False, False), (24, 20, 3, 4, True, True), (24, 20, 5, 2, True, True),
                                                           (16, 16, 9, 4, False, True), (24, 20, 9, 2, False, False),
                                                           (16, 16, 5, 4, True, False)])
def test_device_equals_reference_and_twin(dens, twin, H, W, k, channels, masks, poisoned):
    refs = case(H, W, k, channels, masks, poisoned)
    want, want_best, per = audit_ref.audit(asc.cameras(), refs, k, MATCH, MATCH, CERT)
    assert want[:, 0].sum() > 100 * k and (not masks or (want_best == 255).sum() > 0)
    if poisoned:
        assert want[k - 1, 0] == 0 and want[k - 1, 1] > 50            # the degenerate pair
    # sentinels behind n_refs * H * W of best and behind n_refs * k rows of the table
    best_all = torch.full((3 * H * W + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    table_all = torch.zeros((3 * k + 1, 66), dtype=torch.int64, device=DEV)
    table_all[3 * k] = -77
    best = best_all[:3 * H * W].view(3, H * W)
    table = dens.epipolar_audit(on_device(refs), CERT, table=table_all[:3 * k], best=best)
    hbest = torch.zeros((3, H * W), dtype=torch.uint8)
    host = twin.epipolar_audit(hb.PreparedBatch(refs, MATCH, MATCH), CERT, best=hbest)
    assert np.array_equal(u64(table), want) and np.array_equal(u64(host), want)
    assert np.array_equal(best.cpu().numpy(), want_best) and np.array_equal(hbest.numpy(), want_best)
    assert (best_all[3 * H * W:] == 0xA5).all().item() and (table_all[3 * k] == -77).all().item()
    # the row of the slot the second reference does not have stays zero; a second launch without a map adds the same again
    if k > 1:
        assert (want[2 * k - 1] == 0).all()
    dens.epipolar_audit(on_device(refs), CERT, table=table)
    assert np.array_equal(table.cpu().numpy(), 2 * want.view(np.int64))


def extremes():
    """One reference of 16 x 16 cells (four waves) and three slots whose observations are the cell's own coordinates - on this rig of equal
    orientations the epipolar line of a cell is its own image row, so that is a match on the line.  Slot 0: every lane of every wave in bin 0.
    Slot 1: lane l of every wave displaced by l / 8 + 1 / 16 px across the line (towards the image's middle): every bin occurs in every wave.
    Slot 2: the second wave (cells 64 .. 127) has no confident cell."""
    H = W = 16
    cams = asc.cameras()
    ri = asc.make(2, [1, 3, 0], H, W, match=MATCH).inputs
    ident = torch.from_numpy(np.stack(np.meshgrid(audit_ref.far_ref.axis(W), audit_ref.far_ref.axis(H)), axis=-1).astype(np.float32))
    cert = [torch.full((H, W), 0.9) for _ in range(3)]
    warp = [ident.clone() for _ in range(3)]
    lane = (torch.arange(H * W) % 64).reshape(H, W).to(torch.float32)
    px = (lane / 8.0 + 1.0 / 16.0) * torch.where(torch.arange(H).reshape(H, 1) < H // 2, 1.0, -1.0)
    warp[1][..., 1] += px / (cams[3].height / float(MATCH)) / (0.5 * (MATCH - 1))
    cert[2].view(-1)[64:128] = 0.1
    return dataclasses.replace(ri, cert=cert, warp=warp)


def test_the_extremes_of_the_in_wave_aggregation(dens):
    ri = extremes()
    want, want_best, per = audit_ref.audit(asc.cameras(), [ri], 3, MATCH, MATCH, CERT)
    conf, bn = per[0]["usable"], per[0]["bin"]
    for wave in range(4):
        sl = slice(64 * wave, 64 * wave + 64)
        assert conf[sl, 0].all() and (bn[sl, 0] == 0).all()            # one bin for the whole wave
        assert conf[sl, 1].all() and set(bn[sl, 1].tolist()) == set(range(64))
    assert not per[0]["conf"][64:128, 2].any() and per[0]["conf"][128:, 2].all() and per[0]["conf"][:64, 2].all()
    best = torch.zeros((1, 256), dtype=torch.uint8, device=DEV)
    table = dens.epipolar_audit(on_device([ri], asc.cameras()), CERT, best=best)
    assert np.array_equal(u64(table), want) and np.array_equal(best.cpu().numpy(), want_best)


def test_launch_geometry_and_the_per_lane_variant(dens, monkeypatch):
    refs = case(24, 20, 3, 2, True, True)
    want, _b, _p = audit_ref.audit(asc.cameras(), refs, 3, MATCH, MATCH, CERT)
    parts = [u64(dens.epipolar_audit(on_device([r]), CERT)) for r in refs]
    assert parts[1].shape == (2, 66)
    assert np.array_equal(parts[0], want[0:3]) and np.array_equal(parts[1], want[3:5]) and np.array_equal(parts[2], want[6:9])
    monkeypatch.setenv("LFD_AUDIT_NO_AGGREGATE", "1")
    per_lane = dens.epipolar_audit(on_device(refs), CERT)
    ext = dens.epipolar_audit(on_device([extremes()], asc.cameras()), CERT)
    monkeypatch.delenv("LFD_AUDIT_NO_AGGREGATE")
    assert np.array_equal(u64(per_lane), want)
    assert np.array_equal(u64(ext), audit_ref.audit(asc.cameras(), [extremes()], 3, MATCH, MATCH, CERT)[0])


def test_contexts_refuse_each_others_calls(dens, twin):
    refs = case(16, 16, 3, 2, False, False)
    table = hb.audit_table(3, 3, DEV)
    rc, _t = hb._epipolar_audit_call(dens._lib.lfd_epipolar_audit_host, dens._ctx, on_device(refs), CERT, table, None, DEV)
    assert rc == LFD_ERR_STATE
    host_table = hb.audit_table(3, 3, torch.device("cpu"))
    rc, _t = hb._epipolar_audit_call(twin._lib.lfd_epipolar_audit, twin._ctx, hb.PreparedBatch(refs, MATCH, MATCH), CERT, host_table, None,
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


@pytest.mark.parametrize("mode,refs_per_launch", [("dense", 0), ("sampled", 2), ("sampled", 1)])
def test_the_driver_on_the_device_writes_the_host_backends_report(tmp_path, mode, refs_per_launch):
    """One record pitched by 0.5 degrees, a rectangle of cells displaced: audit.json and every map file of the device run are the host
    backend's byte for byte - dense mode, and sampled mode through the asynchronous schedules, where a launch's table travels with its
    buffers until its result is committed."""
    import json
    import os

    import lichtfeld_densification_plugin_amd as lfd
    from lichtfeld_densification_plugin_amd import densify
    cams = asc.write_scene(str(tmp_path / "scene"), (2, 0.5))
    nodes = [Node(c) for c in cams]
    recs = densify.extract_cameras_from_lfs(nodes)
    files = {}
    for backend in ("device", "host"):
        out = str(tmp_path / backend / "out.ply")
        os.makedirs(os.path.dirname(out))
        cfg = lfd.DensePipelineConfig(output_path=out, num_refs=1.0, nns_per_ref=3, seed=3, viz_interval=0, pack_workers=1, matches_per_ref=2500,
                                      backend=backend, triangulation_mode=mode, refs_per_launch=refs_per_launch if backend == "device" else 0,
                                      experimental={"epipolar_audit": "report", "audit_maps_dir": "epi"})
        kw = {"device": DEV} if backend == "device" else {}
        matcher = asc.Matcher(recs, device=DEV if backend == "device" else "cpu", displaced=(10, 30, 20, 44))
        rc, msg = densify.dense_init_from_lfs(nodes, cfg, matcher=matcher, **kw)
        assert rc == 0, msg
        files[backend] = out
    text = {b: open(files[b] + ".audit.json", "rb").read() for b in files}
    assert text["device"] == text["host"]
    js = json.loads(text["device"])
    assert js["scene"]["suspects"] == [int(cams[2].uid)] and len(js["pairs"]) == 18 and len(js["maps"]["references"]) == 6
    for e in js["maps"]["references"]:
        maps = [open(os.path.join(os.path.dirname(files[b]), "epi", e["map"]), "rb").read() for b in ("device", "host")]
        assert maps[0] == maps[1] and len(maps[0]) > 1000
