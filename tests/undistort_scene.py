"""What the driver tests of the image undistortion share (tests/test_undistort_driver.py on the host backend, tests/test_gpu_undistort.py on the
device): small COLMAP scenes on disk whose cameras carry a distortion model, optional mask files, a matcher that records the images it is handed,
and what the NumPy reference (tests/undistort_ref.py) says those images and the cameras' masks have to be."""
import os

import numpy as np
from PIL import Image

import undistort_ref as ur
from lichtfeld_densification_plugin_amd import densify, synthetic

W, H = 320, 208
# strong coefficients: the scene's focal length is three image widths, so r2 stays below 0.04.  The SIMPLE_RADIAL camera is a barrel camera (every
# pixel of the pinhole image lies inside the photograph: no mask of its own), the OPENCV one a pincushion camera with a frame of uncovered pixels.
MODELS = {"SIMPLE_RADIAL": (-1.5,), "OPENCV": (2.0, -3.0, 0.02, -0.015), "SIMPLE_PINHOLE": (), "PINHOLE": (),
          "OPENCV_FISHEYE": (0.01, 0.0, 0.0, 0.0), "SIMPLE_RADIAL_FISHEYE": (0.01,)}
PINHOLE_OF = {"SIMPLE_RADIAL": "SIMPLE_PINHOLE", "OPENCV": "PINHOLE"}


def make_scene(root: str, model: str, n_cams: int = 4, masks: bool = False):
    synthetic.write_colmap_scene(root, n_cams=n_cams, width=W, height=H, fmt="png", camera_model=model, distortion=MODELS[model])
    args = densify.build_argparser().parse_args(["--scene_root", root, "--images_subdir", "images_4", "--num_refs", "0.75", "--nns_per_ref", "3"])
    records, refs, nn, _ = densify.plan_scene(args)
    if masks:
        os.makedirs(os.path.join(root, "masks"), exist_ok=True)
        yy, xx = np.mgrid[0:H, 0:W]
        for i, rec in enumerate(records):
            # a grey-level mask file: a bright disc off the centre with a soft edge, different for every camera
            r = np.hypot(xx - (150 + 9 * i), yy - (100 - 5 * i))
            plane = np.clip(255.0 - 3.0 * np.maximum(r - 80.0, 0.0), 0, 255).astype(np.uint8)
            rec.mask_path = os.path.join(root, "masks", f"mask_{i:04d}.png")
            Image.fromarray(plane).save(rec.mask_path)
    return dict(cams=records, refs=[int(r) for r in refs], nn=nn, root=root, model=model)


class RecordingMatcher(synthetic.SyntheticMatcher):
    """The analytic matcher (it never looks at pixels), keeping the image every camera was matched with."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.seen = {}

    def match_grids_batch(self, imA, imB_list, keys=None):
        for cam, im in zip([int(keys[0])] + [int(k) for k in keys[1]], [imA] + list(imB_list)):
            arr = im.cpu().numpy() if hasattr(im, "cpu") else np.asarray(im)
            if cam in self.seen:
                assert np.array_equal(self.seen[cam], arr), f"camera {cam} was prepared in two different ways"
            self.seen[cam] = arr.copy()
        return super().match_grids_batch(imA, imB_list, keys=keys)


def matcher_for(scene, device="cpu", cert_mode="smooth"):
    return RecordingMatcher(scene["cams"], setting="turbo", device=device, channels=2, cert_mode=cert_mode)


def expected_view(cam, size_wh, undistort: bool):
    """(match-size image, {0,1} mask or None) of one camera as the contract prescribes them, through NumPy and PIL alone."""
    dec = np.asarray(Image.open(cam.image_path).convert("RGB"), dtype=np.uint8)
    d = cam.distortion
    on = undistort and d is not None and any(v != 0.0 for v in d[4:])
    valid01 = None
    if on:
        dec, valid255, n_invalid = ur.undistort(dec, d[:4], d[4:])
        if n_invalid:
            valid01 = _plane01(Image.fromarray(valid255), size_wh)
    img = np.asarray(Image.fromarray(dec).resize(tuple(size_wh), Image.BILINEAR), dtype=np.uint8)
    mask = None
    if cam.mask_path:
        plane = np.asarray(Image.open(cam.mask_path).convert("L"), dtype=np.uint8)
        if on:
            plane = ur.undistort(plane, d[:4], d[4:], nearest=True)[0]
        mask = _plane01(Image.fromarray(plane), size_wh)
    if valid01 is not None:
        mask = valid01 if mask is None else (mask & valid01)
    if mask is not None:
        img = img.copy()
        img[mask == 0] = 0
    return img, mask


def _plane01(im, size_wh):
    if im.size != tuple(size_wh):
        im = im.resize(tuple(size_wh), Image.NEAREST)
    return ((np.asarray(im, dtype=np.uint8).astype(np.float32) / 255.0) > 0.5).astype(np.uint8)
