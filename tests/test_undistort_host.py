"""The CPU twin of the image undistortion (lfd_host_undistort_image) against the independent NumPy reference
(tests/undistort_ref.py), byte for byte: every supported model, both channel counts, bilinear and nearest, with and without the validity plane,
at sizes from 1 x 1 up; the identity of zero coefficients; a pincushion camera whose corners the photograph does not cover; a rational model
whose denominator crosses zero inside the image; and the render round trip, which shows what the feature is for: the undistorted photograph of
an analytic texture is the texture at the pinhole pixel centres to within 2 grey levels, the photograph itself is off by more than 50."""
import numpy as np
import pytest

import undistort_ref as ur
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

SIZES = [(1, 1), (2, 2), (67, 41), (257, 3), (320, 240)]
PINCUSHION = (0.10, 0, 0, 0, 0, 0, 0, 0)
PINCUSHION_INTR = (260.0, 260.0, 160.0, 120.0)


def intrinsics(w, h):
    return (300.0, 301.5, w / 2.0 + 1.3, h / 2.0 - 0.7)


def image(w, h, channels, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w) if channels == 1 else (h, w, 3), dtype=np.uint8)


def same(got, ref, with_valid):
    assert np.array_equal(got[0], ref[0])
    assert got[2] == ref[2]
    if with_valid:
        assert np.array_equal(got[1], ref[1]) and set(np.unique(got[1])) <= {0, 255}
    else:
        assert got[1] is None


@pytest.mark.parametrize("model", list(ur.MODEL_CASES))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_twin_equals_reference(model, size):
    w, h = size
    d, intr = ur.MODEL_CASES[model], intrinsics(w, h)
    for channels in (1, 3):
        src = image(w, h, channels, seed=w * 7 + channels)
        for nearest in (False, True):
            ref = ur.undistort(src, intr, d, nearest=nearest)
            for with_valid in (False, True):
                same(hb.host_undistort_image(src, intr + d, nearest=nearest, with_valid=with_valid), ref, with_valid)


@pytest.mark.parametrize("size", SIZES + [(640, 480)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_zero_coefficients_return_the_input(size):
    w, h = size
    for intr in (intrinsics(w, h), (1234.5678, 987.654321, 0.1 * w, 0.9 * h), (0.3, 7e5, -40.0, 3.0 * h)):
        for channels in (1, 3):
            src = image(w, h, channels, seed=3)
            for nearest in (False, True):
                dst, valid, n_invalid = hb.host_undistort_image(src, intr + (0.0,) * 8, nearest=nearest, with_valid=True)
                assert np.array_equal(dst, src) and n_invalid == 0 and valid.min() == 255
                ref = ur.undistort(src, intr, (0.0,) * 8, nearest=nearest)                 # (the contract's own claim, in NumPy)
                assert np.array_equal(ref[0], src) and ref[2] == 0


def test_pincushion_corners_are_invalid():
    w, h = 320, 240
    src = image(w, h, 3, seed=5)
    ref = ur.undistort(src, PINCUSHION_INTR, PINCUSHION)
    got = hb.host_undistort_image(src, PINCUSHION_INTR + PINCUSHION, with_valid=True)
    same(got, ref, True)
    n_invalid = got[2]
    print(f"pincushion k1 = +0.10, fx = 260, 320 x 240: {n_invalid} invalid pixels")
    # the exact count is the NumPy reference's: a frame around the image, widest at the corners (a few per cent of the pixels)
    assert n_invalid == ref[2] == int((got[1] == 0).sum()) and 0.02 * w * h < n_invalid < 0.10 * w * h
    for i, j in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        assert got[1][i, j] == 0 and not got[0][i, j].any()
    assert got[1][h // 2, w // 2] == 255 and got[1][20, w // 2] == 255 and got[1][h // 2, 20] == 255


def test_a_denominator_that_crosses_zero_invalidates_those_pixels_only():
    w, h = 320, 240
    intr = (300.0, 300.0, 160.0, 120.0)
    # den = 1 + k4 r2 with r2 = x x + y y evaluated in f64; k4 = -1 / r2 of pixel (120, 208): 48.5^2 / 300^2 = 2352.25 / 90000
    x = ((208.0 + 0.5) - 160.0) / 300.0
    y = ((120.0 + 0.5) - 120.0) / 300.0
    r2 = x * x + y * y
    k4 = -1.0 / r2
    assert 1.0 + k4 * r2 == 0.0                                       # the denominator is exactly zero on that pixel (and its mirror images)
    d = (0.0, 0, 0, 0, 0, k4, 0, 0)
    src = image(w, h, 3, seed=9)
    ref = ur.undistort(src, intr, d)
    got = hb.host_undistort_image(src, intr + d, with_valid=True)
    same(got, ref, True)
    assert got[1][120, 208] == 0 and not got[0][120, 208].any()
    # nothing else changes: a pixel is invalid exactly where the reference's source coordinates leave the image or are not numbers
    su, sv, valid = ur.source_coordinates(w, h, intr, d)
    assert not np.isfinite(su[120, 208]) and np.array_equal(got[1] == 255, valid) and 0 < got[2] < w * h


ROUND_TRIP = {"pincushion": PINCUSHION, "barrel": ur.MODEL_CASES["SIMPLE_RADIAL"], "radial": ur.MODEL_CASES["RADIAL"],
              "tangential": ur.MODEL_CASES["OPENCV"], "rational": ur.MODEL_CASES["FULL_OPENCV"]}


@pytest.mark.parametrize("case", list(ROUND_TRIP))
def test_render_round_trip(case):
    """Bound 2 grey levels: bilinear error (M_u + M_v) / 8 < 0.3 for the texture's second derivatives under the local stretch, + 0.5 for the
    quantisation of the photograph, + 0.5 for the output's.  Measured with the twin: 0.97 - 1.01 in the five cases; the photograph itself is off
    by 55 - 87 levels; the pincushion case leaves out 7.5 % of the pixels (invalid corners, clamped taps), the other four none."""
    w, h = 320, 240
    d, intr = ROUND_TRIP[case], PINCUSHION_INTR
    photo = ur.render_distorted(w, h, intr, d)
    want = ur.pinhole_texture(w, h)
    got, _valid, _n = hb.host_undistort_image(photo, intr + d, with_valid=True)
    inside = ur.unclamped(w, h, intr, d)
    left_out = 1.0 - float(inside.mean())
    err = float(np.abs(got[inside].astype(np.float64) - want[inside]).max())
    raw = float(np.abs(photo.astype(np.float64) - want).max())
    print(f"{case}: undistorted within {err:.3f} levels of the texture on {100.0 * (1.0 - left_out):.1f} % of the pixels; the photograph is off by {raw:.1f}")
    assert left_out <= 0.10
    assert err <= 2.0
    assert raw > 50.0


def test_the_binding_refuses_what_the_library_refuses():
    src = image(8, 6, 3, seed=1)
    with pytest.raises(ValueError, match="twelve"):
        hb.host_undistort_image(src, (1.0, 1.0, 0.0, 0.0))
    with pytest.raises(ValueError, match="uint8 array"):
        hb.host_undistort_image(np.zeros((4, 4, 2), np.uint8), intrinsics(4, 4) + (0.0,) * 8)
    with pytest.raises(hb.HipBackendError, match="lfd_host_undistort_image"):
        hb.host_undistort_image(src, (0.0, 1.0, 0.0, 0.0) + (0.0,) * 8)
    with pytest.raises(hb.HipBackendError, match="lfd_host_undistort_image"):
        hb.host_undistort_image(src, intrinsics(8, 6) + (float("nan"),) + (0.0,) * 7)
