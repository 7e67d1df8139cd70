"""NumPy reference of the image undistortion (lfd_undistort_image), written from the contract and independent of the library:
the camera model with its eight coefficients in f64, the validity test, the clamped bilinear / nearest sampling, and - for the render round
trip - the inverse of the model by fixed-point iteration.  NumPy evaluates every + - * / and floor in IEEE f64 without contraction, so the
library is compared with ``==``."""
import numpy as np

# coefficient order of the contract: k1 k2 p1 p2 k3 k4 k5 k6
MODEL_CASES = {
    "SIMPLE_PINHOLE": (0.0,) * 8,
    "PINHOLE": (0.0,) * 8,
    "SIMPLE_RADIAL": (-0.12, 0, 0, 0, 0, 0, 0, 0),
    "RADIAL": (-0.10, 0.03, 0, 0, 0, 0, 0, 0),
    "OPENCV": (-0.09, 0.02, 0.004, -0.003, 0, 0, 0, 0),
    "FULL_OPENCV": (-0.11, 0.04, 0.002, 0.003, -0.01, 0.05, -0.02, 0.004),
}


def distort(x, y, d):
    """The model on normalised coordinates (f64 arrays): every rounding in the order of the contract."""
    k1, k2, p1, p2, k3, k4, k5, k6 = (np.float64(v) for v in d)
    xx, yy = x * x, y * y
    r2 = xx + yy
    r4 = r2 * r2
    r6 = r4 * r2
    xy = x * y
    num = ((1.0 + k1 * r2) + k2 * r4) + k3 * r6
    den = ((1.0 + k4 * r2) + k5 * r4) + k6 * r6
    with np.errstate(all="ignore"):
        rad = num / den
        xd = (x * rad + (2.0 * p1) * xy) + p2 * (r2 + 2.0 * xx)
        yd = (y * rad + (2.0 * p2) * xy) + p1 * (r2 + 2.0 * yy)
    return xd, yd


def source_coordinates(w, h, intr, d):
    """(su, sv, valid) of every output pixel: where the photograph shows it, in pixel-index coordinates."""
    fx, fy, cx, cy = (np.float64(v) for v in intr)
    j = np.arange(w, dtype=np.float64)[None, :]
    i = np.arange(h, dtype=np.float64)[:, None]
    x = np.broadcast_to(((j + 0.5) - cx) / fx, (h, w))
    y = np.broadcast_to(((i + 0.5) - cy) / fy, (h, w))
    xd, yd = distort(x, y, d)
    with np.errstate(all="ignore"):
        su = (fx * xd + cx) - 0.5
        sv = (fy * yd + cy) - 0.5
        valid = (su >= -0.5) & (su <= w - 0.5) & (sv >= -0.5) & (sv <= h - 0.5)
    return su, sv, valid


def undistort(src, intr, d, nearest=False):
    """(dst, valid255, n_invalid) of the contract for a (h, w) or (h, w, 3) u8 image."""
    src = np.asarray(src, np.uint8)
    h, w = src.shape[:2]
    planes = src.reshape(h, w, -1)
    su, sv, valid = source_coordinates(w, h, intr, d)
    su = np.where(valid, su, 0.0)                       # (no conversion of a value that failed the test)
    sv = np.where(valid, sv, 0.0)
    if nearest:
        xs = np.clip(np.floor(su + 0.5).astype(np.int64), 0, w - 1)
        ys = np.clip(np.floor(sv + 0.5).astype(np.int64), 0, h - 1)
        out = planes[ys, xs]
    else:
        x0f, y0f = np.floor(su), np.floor(sv)
        ax, ay = (su - x0f)[..., None], (sv - y0f)[..., None]
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        xa, xb = np.clip(x0, 0, w - 1), np.clip(x0 + 1, 0, w - 1)
        ya, yb = np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1)
        p00, p01 = planes[ya, xa].astype(np.float64), planes[ya, xb].astype(np.float64)
        p10, p11 = planes[yb, xa].astype(np.float64), planes[yb, xb].astype(np.float64)
        top = p00 + ax * (p01 - p00)
        bot = p10 + ax * (p11 - p10)
        val = top + ay * (bot - top)
        out = np.floor(val + 0.5).astype(np.uint8)
    out = np.where(valid[..., None], out, 0).astype(np.uint8).reshape(src.shape)
    return out, np.where(valid, 255, 0).astype(np.uint8), int((~valid).sum())


def unclamped(w, h, intr, d):
    """The valid pixels whose four bilinear taps all lie inside the image: no edge replication took part in them."""
    su, sv, valid = source_coordinates(w, h, intr, d)
    with np.errstate(invalid="ignore"):
        return valid & (su >= 0.0) & (np.floor(su) + 1.0 <= w - 1) & (sv >= 0.0) & (np.floor(sv) + 1.0 <= h - 1)


def undistort_points(xd, yd, d, rounds=60):
    """The inverse of ``distort`` by the fixed-point iteration x <- x - (distort(x) - xd); the residual is asserted below 1e-12."""
    x, y = np.array(xd, np.float64), np.array(yd, np.float64)
    for _ in range(rounds):
        ex, ey = distort(x, y, d)
        x, y = x - (ex - xd), y - (ey - yd)
    ex, ey = distort(x, y, d)
    assert float(np.max(np.abs(ex - xd))) < 1e-12 and float(np.max(np.abs(ey - yd))) < 1e-12
    return x, y


def texture(u, v):
    """An analytic grey texture over pinhole pixel coordinates (pixel centres at +0.5): mean 128, amplitude 100, shortest period 64 px."""
    return 128.0 + 50.0 * np.sin(2.0 * np.pi * u / 64.0) * np.cos(2.0 * np.pi * v / 97.0) + 50.0 * np.cos(2.0 * np.pi * (u + 2.0 * v) / 181.0)


def render_distorted(w, h, intr, d):
    """The photograph a camera with this distortion takes of ``texture`` laid out over its pinhole image plane: source pixel (i, j) looks
    along the distorted direction, which the inverse model turns into the pinhole pixel whose texture value it records (u8, round half up)."""
    fx, fy, cx, cy = (np.float64(v) for v in intr)
    j = np.arange(w, dtype=np.float64)[None, :]
    i = np.arange(h, dtype=np.float64)[:, None]
    xd = np.broadcast_to(((j + 0.5) - cx) / fx, (h, w))
    yd = np.broadcast_to(((i + 0.5) - cy) / fy, (h, w))
    x, y = undistort_points(xd, yd, d)
    return np.floor(np.clip(texture(fx * x + cx, fy * y + cy), 0.0, 255.0) + 0.5).astype(np.uint8)


def pinhole_texture(w, h):
    """``texture`` at the pinhole pixel centres: what the undistorted photograph should show."""
    j = np.arange(w, dtype=np.float64)[None, :] + 0.5
    i = np.arange(h, dtype=np.float64)[:, None] + 0.5
    return np.broadcast_to(texture(j, i), (h, w))
