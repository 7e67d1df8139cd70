"""The image undistortion on the device (lfd_undistort_image through HipDensifier.undistort_image) against the CPU twin and the NumPy reference
(tests/undistort_ref.py), byte for byte, on the shapes and cases of tests/test_undistort_host.py - 1 x 1 up to 320 x 240, every model, both
channel counts, bilinear and nearest, the pincushion camera's invalid corners, the denominator that crosses zero - plus one 640 x 480 FULL_OPENCV
image; the invalid count the call reports; two calls on one context and a smaller image after a larger one in the context's workspace; the
refusals of a device context; and, through the driver, dense_init on the SIMPLE_RADIAL scene with the images prepared on the device against the
run with them prepared on the host."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import undistort_ref as ur
import undistort_scene as us
from lichtfeld_densification_plugin_amd import densify
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from test_undistort_host import PINCUSHION, PINCUSHION_INTR, SIZES, image, intrinsics

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LFD_ERR_INVALID, LFD_ERR_STATE = 1, 4


@pytest.fixture(scope="module")
def dens():
    d = hb.HipDensifier(DEV)
    yield d
    d.close()


def three_ways(dens, src, params, nearest=False, with_valid=True, workspace=None):
    """device == twin == reference for one image; returns the reference's invalid count"""
    intr, d = tuple(params[:4]), tuple(params[4:])
    ref = ur.undistort(src, intr, d, nearest=nearest)
    host = hb.host_undistort_image(src, params, nearest=nearest, with_valid=with_valid)
    dev = dens.undistort_image(torch.from_numpy(src).to(DEV), params, nearest=nearest, with_valid=with_valid, count=True, workspace=workspace)
    assert np.array_equal(dev[0].cpu().numpy(), host[0]) and np.array_equal(host[0], ref[0])
    assert dev[2] == host[2] == ref[2]
    if with_valid:
        assert np.array_equal(dev[1].cpu().numpy(), host[1]) and np.array_equal(host[1], ref[1])
    else:
        assert dev[1] is None and host[1] is None
    return ref[2]


@pytest.mark.parametrize("model", list(ur.MODEL_CASES))
def test_device_equals_twin_equals_reference(dens, model):
    d = ur.MODEL_CASES[model]
    for w, h in SIZES:
        for channels in (1, 3):
            src = image(w, h, channels, seed=w * 7 + channels)
            for nearest in (False, True):
                three_ways(dens, src, intrinsics(w, h) + d, nearest=nearest, with_valid=not (nearest and channels == 3))
                if not any(d):
                    out = dens.undistort_image(torch.from_numpy(src).to(DEV), intrinsics(w, h) + d, nearest=nearest)[0]
                    assert np.array_equal(out.cpu().numpy(), src)                # zero coefficients: the input


def test_invalid_pixels_and_their_count(dens):
    w, h = 320, 240
    n = three_ways(dens, image(w, h, 3, seed=5), PINCUSHION_INTR + PINCUSHION)
    assert 0.02 * w * h < n < 0.10 * w * h                                       # the pincushion camera's frame of uncovered pixels
    intr = (300.0, 300.0, 160.0, 120.0)
    x, y = ((208.0 + 0.5) - 160.0) / 300.0, ((120.0 + 0.5) - 120.0) / 300.0
    k4 = -1.0 / (x * x + y * y)                                                  # the denominator is exactly zero on pixel (120, 208)
    src = torch.from_numpy(image(w, h, 3, seed=9)).to(DEV)
    n = three_ways(dens, src.cpu().numpy(), intr + (0.0, 0, 0, 0, 0, k4, 0, 0))
    out, valid, _ = dens.undistort_image(src, intr + (0.0, 0, 0, 0, 0, k4, 0, 0), with_valid=True)        # asynchronous: no count
    assert n > 0 and int(valid[120, 208]) == 0 and not bool(out[120, 208].any()) and int((valid == 0).sum()) == n


def test_one_larger_image_every_coefficient(dens):
    w, h = 640, 480
    params = (610.0, 608.5, 322.1, 237.9) + ur.MODEL_CASES["FULL_OPENCV"]
    three_ways(dens, image(w, h, 3, seed=11), params)


def test_two_calls_on_one_context_and_a_smaller_image_after_a_larger_one(dens):
    big, small = image(320, 240, 3, seed=21), image(67, 41, 3, seed=22)
    p_big, p_small = PINCUSHION_INTR + PINCUSHION, intrinsics(67, 41) + ur.MODEL_CASES["OPENCV"]
    n1 = three_ways(dens, big, p_big, workspace="w")
    n2 = three_ways(dens, big, p_big, workspace="w")                               # the counter starts from zero again
    assert n1 == n2 > 0
    three_ways(dens, small, p_small, workspace="w")                               # views of the larger image's buffers
    three_ways(dens, image(67, 41, 1, seed=23), p_small, nearest=True, workspace="w")
    assert three_ways(dens, big, p_big, workspace="w") == n1


def test_what_a_device_context_refuses(dens):
    lib = hb.load_library()
    src, dst = torch.zeros((4, 4, 3), dtype=torch.uint8, device=DEV), torch.zeros((4, 4, 3), dtype=torch.uint8, device=DEV)
    intr, dist = (C.c_double * 4)(10.0, 10.0, 2.0, 2.0), (C.c_double * 8)()
    call = lambda **kw: lib.lfd_undistort_image(dens._ctx, *[{**dict(src=src.data_ptr(), w=4, h=4, ch=3, nearest=0, intr=intr, dist=dist,      # noqa: E731
                                                                  dst=dst.data_ptr(), valid=None, n=None), **kw}[k]
                                                             for k in ("src", "w", "h", "ch", "nearest", "intr", "dist", "dst", "valid", "n")])
    assert call() == 0
    bad_f, bad_d = (C.c_double * 4)(0.0, 10.0, 2.0, 2.0), (C.c_double * 8)(float("nan"))
    for kw in (dict(src=None), dict(dst=None), dict(intr=None), dict(dist=None), dict(w=0), dict(h=-1), dict(w=1 << 16, h=1 << 15), dict(ch=2),
               dict(intr=bad_f), dict(dist=bad_d), dict(dst=src.data_ptr()), dict(dst=src.data_ptr() + 3), dict(valid=dst.data_ptr() + 40)):
        assert call(**kw) == LFD_ERR_INVALID, kw
        assert lib.lfd_last_error(dens._ctx).startswith(b"lfd_undistort_image: "), kw
    torch.cuda.synchronize()
    ctx = C.c_void_p()
    assert lib.lfd_create_host(1, C.byref(ctx)) == 0
    try:
        assert lib.lfd_undistort_image(ctx, src.data_ptr(), 4, 4, 3, 0, intr, dist, dst.data_ptr(), None, None) == LFD_ERR_STATE
    finally:
        lib.lfd_destroy(ctx)
    with pytest.raises(ValueError, match="uint8 tensor"):
        dens.undistort_image(torch.zeros((4, 4, 3), dtype=torch.uint8), (10.0, 10.0, 2.0, 2.0) + (0.0,) * 8)          # a CPU tensor


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    return us.make_scene(str(tmp_path_factory.mktemp("gpu_undistort_scene")), "SIMPLE_RADIAL", masks=False)


def cli(scene, out_name, mode, extra, device="cuda:0"):
    args = densify.build_argparser().parse_args(["--scene_root", scene["root"], "--images_subdir", "images_4", "--num_refs", "0.75", "--nns_per_ref", "3",
                                                 "--matches_per_ref", "2500", "--seed", "3", "--pack_workers", "1", "--triangulation_mode", mode,
                                                 "--out_name", out_name, "--undistort_images"] + extra)
    # distinct certainties: with tied sampling weights (the default field saturates at the sampler's cap) the coverage pass of the sampled mode
    # is decided by the order in which an unstable sort leaves the ties - NumPy's on the host backend, the device's own rule in the kernels -
    # and the two backends draw different cells whatever images they are given; a comparison of the backends needs a field
    # without ties, as tests/test_host_backend.py uses for its device / host comparison
    matcher = us.matcher_for(scene, device=device, cert_mode="tiefree")
    assert densify.dense_init(args, matcher=matcher) == 0
    return open(os.path.join(scene["root"], "sparse", "0", out_name), "rb").read(), matcher


def differing_bytes(a, b):
    return sum(x != y for x, y in zip(a, b)) + abs(len(a) - len(b))


def vertices(ply):
    return int(ply.split(b"element vertex ")[1].split(b"\n")[0])


@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_dense_init_with_the_images_prepared_on_the_device(scene, mode):
    """One run with device_image_prep on the device, one with backend='host'; the matcher is handed the same images - the reference-undistorted
    decode through Pillow's resize - byte for byte, and the two files are equal byte for byte."""
    on_device, m_dev = cli(scene, f"dev_{mode}.ply", mode, ["--device_image_prep"])
    on_host, m_host = cli(scene, f"host_{mode}.ply", mode, ["--backend", "host"], device="cpu")
    assert sorted(m_dev.seen) == sorted(m_host.seen) == list(range(len(scene["cams"])))
    for cam_index, seen in m_dev.seen.items():
        assert np.array_equal(seen, us.expected_view(scene["cams"][cam_index], (320, 320), undistort=True)[0])
        assert np.array_equal(seen, m_host.seen[cam_index])
    print(f"{mode}: {vertices(on_device)} points from the device run, {vertices(on_host)} from the host run, "
          f"{differing_bytes(on_device, on_host)} differing bytes of {len(on_host)}")
    assert vertices(on_host) > 1000
    assert on_device == on_host


@pytest.fixture(scope="module")
def masked_scene(tmp_path_factory):
    return us.make_scene(str(tmp_path_factory.mktemp("gpu_undistort_masked")), "OPENCV", masks=True)


def prepared_both_ways(scene, mode):
    """experimental['undistort_images'] with device_image_prep on and off on the device backend: the images the matcher is handed (masked pixels
    black) are the reference's, every camera has a mask that keeps some pixels and drops some, and the two runs - the same kernels on images
    prepared on the device and on the host - give the same arrays bit for bit."""
    import lichtfeld_densification_plugin_amd as lfd
    from lichtfeld_densification_plugin_amd.core import pipeline as pl
    files = []
    for prep in (True, False):
        out = os.path.join(scene["root"], f"prep{int(prep)}_{mode}.ply")
        cfg = lfd.DensePipelineConfig(output_path=out, nns_per_ref=3, seed=3, viz_interval=0, matches_per_ref=2500, pack_workers=1,
                                      triangulation_mode=mode, device_image_prep=prep, experimental={"undistort_images": True})
        matcher = us.matcher_for(scene, device="cuda:0")
        res = pl.run_dense_pipeline(scene["cams"], scene["refs"], scene["nn"], cfg, matcher=matcher)
        assert res.xyz.shape[0] > 0
        for cam_index, seen in matcher.seen.items():
            img, mask = us.expected_view(scene["cams"][cam_index], (320, 320), undistort=True)
            assert mask is not None and 0 < int(mask.sum()) < mask.size and np.array_equal(seen, img)
        files.append((res.xyz.copy(), res.rgb.copy(), res.err.copy(), np.asarray(res.points_per_reference).copy()))
    for a, b in zip(*files):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_device_preparation_with_mask_files_and_uncovered_pixels(masked_scene, mode):
    """The pincushion scene with mask files: the undistorted mask plane and the validity plane are thresholded and ANDed on the device."""
    prepared_both_ways(masked_scene, mode)


@pytest.fixture(scope="module")
def pincushion_scene(tmp_path_factory):
    return us.make_scene(str(tmp_path_factory.mktemp("gpu_undistort_pincushion")), "OPENCV", masks=False)


@pytest.mark.parametrize("mode", ["sampled", "dense"])
def test_device_preparation_without_mask_files_the_validity_plane_is_the_mask(pincushion_scene, mode):
    """The pincushion scene without mask files: the frame of uncovered pixels becomes the camera's only mask, on the device as on the host."""
    assert all(not c.mask_path for c in pincushion_scene["cams"])
    prepared_both_ways(pincushion_scene, mode)
