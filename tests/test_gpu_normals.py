"""The per-point normals on the device (lfd_estimate_normals through HipDensifier.estimate_normals) against the CPU twin and the
f64 reference of tests/normals_ref.py - all sides are given the SAME input points, the device's own two-view points.  The shapes are the CPU
tier's: two references of 20 x 24 cells (480 points each: the second workgroup straddles the two references) and of 6 x 8 cells (every window
clipped), two- and four-channel warps, the smallest and the largest radius.  Noise-free the statuses equal the twin's exactly and the
components agree within one f32 ulp; with matching noise and gross outliers a status may differ only where the reference puts a decision in
band and the angle to the reference's normal stays within its bound everywhere else.  The counters are the recount of the status bytes,
lfd_pack_ply_normals gives NumPy's records byte for byte, both contexts refuse each other's entry point."""
import dataclasses

import numpy as np
import pytest
import torch

import normals_ref as nr
import normals_scene as ns
import support_scene
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from lichtfeld_densification_plugin_amd.core.writers import ply_records

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LFD_ERR_STATE = 4
REFS = (10, 20)
K = 3
STEP = 0.5


@pytest.fixture(scope="module")
def dens():
    d = hb.HipDensifier(DEV)
    d.upload_cameras(ns.cameras())
    yield d
    d.close()


@pytest.fixture(scope="module")
def twin():
    d = hb.HostDensifier(16)
    d.upload_cameras(ns.cameras())
    yield d
    d.close()


def to_device(ri):
    dev = lambda t: t.to(DEV) if t is not None else None
    return hb.ReferenceInputs(ref_cam=ri.ref_cam, nbr_cams=list(ri.nbr_cams), cert=[dev(c) for c in ri.cert], warp=[dev(w) for w in ri.warp],
                              image=dev(ri.image), mask_a=dev(ri.mask_a), mask_b=[dev(m) for m in ri.mask_b] if ri.mask_b is not None else None)


def on_host(res):
    return dataclasses.replace(res, xyz=res.xyz.cpu(), rgb=res.rgb.cpu(), err=res.err.cpu(), cell=res.cell.cpu(), slot=res.slot.cpu(), _packed=None)


def both(dens, twin, kind, H, W, channels, R, step, **scene):
    """The device's and the twin's normals of the device's own dense points of one scene: (host inputs, points on the host, device normals,
    device status, twin normals, twin status), the counters checked on the way."""
    refs_h = [ns.reference_inputs(kind, ref, K, H, W, channels=channels, **scene)[0] for ref in REFS]
    batch_d = hb.PreparedBatch([to_device(ri) for ri in refs_h], ns.W_MATCH, ns.H_MATCH)
    src = dens.triangulate_dense(batch_d, ns.params())
    counters = torch.zeros(2, dtype=torch.int64, device=DEV)
    got, status = dens.estimate_normals(batch_d, src, R, step, ns.THR, with_status=True, counters=counters)
    again, status2 = dens.estimate_normals(batch_d, src, R, step, ns.THR, with_status=True)
    dens.check_launches()
    assert torch.equal(status, status2) and np.array_equal(ns.bits(got.normals), ns.bits(again.normals))
    for name in ("xyz", "rgb", "err", "cell", "slot"):
        assert np.array_equal(ns.bits(getattr(got, name)), ns.bits(getattr(src, name)))
    st = status.cpu().numpy()
    fitted = int(((st & 0x80) != 0).sum())
    assert counters.cpu().tolist() == [fitted, src.count - fitted]
    src_h = on_host(src)
    want, status_t = twin.estimate_normals(hb.PreparedBatch(refs_h, ns.W_MATCH, ns.H_MATCH), src_h, R, step, ns.THR, with_status=True)
    return refs_h, src_h, got.normals.cpu().numpy(), st, want.normals.numpy(), status_t.numpy()


def within_one_ulp(a, b):
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32))


@pytest.mark.parametrize("R", [1, 2, 4])
@pytest.mark.parametrize("channels", [2, 4])
@pytest.mark.parametrize("H,W", [(20, 24), (6, 8)])
def test_noise_free_device_equals_twin(dens, twin, H, W, channels, R):
    for kind, step, scene in (("plane", STEP, {"tilt_deg": 40.0}), ("plane", STEP, {"tilt_deg": 75.0}), ("slab", 0.05, {}), ("crease", STEP, {})):
        _refs, src, nd, sd, nt, stt = both(dens, twin, kind, H, W, channels, R, step, **scene)
        assert src.count == len(REFS) * H * W
        assert np.array_equal(sd, stt), kind
        ok = within_one_ulp(nd, nt)
        print(f"{kind} {scene} {W}x{H} c{channels} R{R}: {int((ns.bits(nd) != ns.bits(nt)).sum())} of {nd.size} components differ, all within one ulp: {ok.all()}")
        assert ok.all(), kind


@pytest.mark.parametrize("R", [1, 2, 3])
@pytest.mark.parametrize("scene", ["noisy", "in_band"])
def test_noisy_device_against_twin_and_reference(dens, twin, scene, R):
    """``noisy``: the scene whose reference flags at most BAND_CAP of the points (tests/test_normals_host.py checks the same scene and seed on
    the CPU); ``in_band``: outliers along the epipolar lines, where the reference does flag points.  Either way a status may differ only on a
    flagged point and the angle is within the bound everywhere else."""
    spec = dict(ns.NOISY if scene == "noisy" else ns.IN_BAND)
    kind, H, W, channels = spec.pop("kind"), spec.pop("H"), spec.pop("W"), spec.pop("channels")
    refs_h, src, nd, sd, nt, stt = both(dens, twin, kind, H, W, channels, R, ns.NOISY_STEP, **spec)
    ref = nr.over_references(ns.cameras(), refs_h, src, ns.W_MATCH, ns.H_MATCH, R, ns.NOISY_STEP, ns.THR)
    flagged = ref["flagged"]
    print(f"{scene} R{R}: {src.count} points, {int(flagged.sum())} flagged, statuses device != twin {int((sd != stt).sum())}, device != reference "
          f"{int((sd != ref['status']).sum())}")
    assert src.count > 0.8 * len(REFS) * H * W
    if scene == "noisy":
        assert flagged.mean() <= support_scene.BAND_CAP
    else:
        assert 0 < flagged.sum() < 0.1 * src.count
    assert not ((sd != stt) & ~flagged).any()
    assert not ((sd != ref["status"]) & ~flagged).any() and not ((stt != ref["status"]) & ~flagged).any()
    assert ((sd & 0x7f) < (2 * R + 1) ** 2).sum() > 0.1 * src.count      # the outliers do leave windows with fewer cells
    rest = ~flagged & ref["fitted"]
    for name, got in (("device", nd), ("twin", nt)):
        ang = ns.angle(got, ref["normal"])
        print(f"{scene} R{R} {name}: worst angle / bound {(ang[rest] / ref['bound'][rest]).max():.4f}")
        assert (ang[rest] <= ref["bound"][rest]).all(), name
    fell = ~flagged & ~ref["fitted"]
    assert within_one_ulp(nd[fell], ref["fallback"][fell].astype(np.float32)).all()


@pytest.mark.parametrize("n", [0, 1, 257])
def test_pack_ply_normals_gives_numpy_s_records(dens, n):
    g = torch.Generator().manual_seed(n)
    xyz = (torch.rand((n, 3), generator=g) * 8.0 - 4.0).to(DEV)
    nrm = torch.nn.functional.normalize(torch.rand((n, 3), generator=g) - 0.5, dim=1).to(DEV) if n else torch.zeros((0, 3), device=DEV)
    rgb = (torch.rand((n, 3), generator=g) * 1.2 - 0.1).to(DEV)
    got = dens.pack_ply_normals(xyz, nrm, rgb)
    assert got.dtype == torch.uint8 and got.numel() == 27 * n
    want = ply_records(xyz.cpu().numpy(), dens.quantise_rgb(rgb).cpu().numpy(), normals=nrm.cpu().numpy())
    assert got.cpu().numpy().tobytes() == want.tobytes()


def test_each_context_refuses_the_other_s_entry_point(dens, twin):
    refs_h = [ns.reference_inputs("plane", ref, K, 6, 8)[0] for ref in REFS]
    batch_d = hb.PreparedBatch([to_device(ri) for ri in refs_h], ns.W_MATCH, ns.H_MATCH)
    batch_h = hb.PreparedBatch(refs_h, ns.W_MATCH, ns.H_MATCH)
    src = dens.triangulate_dense(batch_d, ns.params())
    rc, _r, _s = hb._normals_call(dens._lib.lfd_estimate_normals_host, dens._ctx, batch_d, src, 1, STEP, ns.THR, False, None, DEV)
    assert rc == LFD_ERR_STATE
    rc, _r, _s = hb._normals_call(twin._lib.lfd_estimate_normals, twin._ctx, batch_h, on_host(src), 1, STEP, ns.THR, False, None, torch.device("cpu"))
    assert rc == LFD_ERR_STATE


@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_the_driver_gives_the_same_normals_whatever_the_grouping(tmp_path_factory, mode):
    """backend='device' through run_dense_pipeline: one reference per launch and the automatic grouping (several references per fused call or
    launch) emit the same points with the same normals, bit for bit; with the knob off the same points and no normals; the file the device
    packs is the host writer's."""
    import cycle_scene
    from lichtfeld_densification_plugin_amd import densify
    scene = cycle_scene.make_scene(str(tmp_path_factory.mktemp("normals_gpu")))
    kw = dict(noise_px=0.0, outlier_frac=0.0, cert_mode="tiefree")
    exp = {"estimate_normals": True, "normal_radius_cells": 2}
    run = lambda name, **cfg: cycle_scene.run(scene, cycle_scene.matcher_for(scene, device=DEV, **kw), name, backend="device", device=DEV,
                                              triangulation_mode=mode, **cfg)
    one = run("one.ply", refs_per_launch=1, experimental=exp)
    auto = run("auto.ply", experimental=exp)
    off = run("off.ply")
    assert cycle_scene.same_cloud(one, auto) and cycle_scene.same_cloud(one, off) and one.xyz.shape[0] > 500
    assert off.normals is None and off.device_normals is None
    assert one.device_normals.is_cuda and one.normals.shape == one.xyz.shape
    assert np.array_equal(ns.bits(one.normals), ns.bits(auto.normals))
    length = np.linalg.norm(one.normals.astype(np.float64), axis=1)
    assert (np.abs(length - 1.0) <= 2.0 ** -22).all()
    # the 27-byte file, packed where the points are, against the host writer
    path, ref = str(tmp_path_factory.mktemp("normals_out") / "dev.ply"), str(tmp_path_factory.mktemp("normals_out") / "host.ply")
    assert densify._finish_on_device(auto, path, 0, 0) == auto.xyz.shape[0]
    densify._write_output(ref, auto.xyz, auto.rgb, auto.err, None, normals=auto.normals)
    assert open(path, "rb").read() == open(ref, "rb").read()
