"""CPU tier of the per-point normals (lfd_estimate_normals_host): the twin against the f64 reference of tests/normals_ref.py and
against the analytic normals of the scenes of tests/normals_scene.py, the window rules at a depth step, every documented fallback and the
effect of the window radius on a noisy plane."""
import dataclasses

import numpy as np
import pytest
import torch

import normals_ref as nr
import normals_scene as ns
import support_scene
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

REFS = (10, 20)
K = 3
PLANE_STEP = 0.5         # depth_step_rel of the plane tests: the steepest plane's depth varies by 0.38 of the nearer depth over the 6 x 8 grid
_cache = {}


@pytest.fixture(scope="module")
def twin():
    d = hb.HostDensifier(4)
    d.upload_cameras(ns.cameras())
    yield d
    d.close()


def probe(twin, kind, H, W, channels=2, tilt=0.0, noise=0.0, refs=REFS, edit=None):
    """References of one scene triangulated by the twin's dense call (``edit``: a function that changes the ReferenceInputs first; not cached)."""
    key = (kind, H, W, channels, tilt, noise, refs)
    if edit is None and key in _cache:
        return _cache[key]
    made = [ns.reference_inputs(kind, ref, K, H, W, channels=channels, tilt_deg=tilt, noise_px=noise) for ref in refs]
    ris, truth = [m[0] for m in made], [m[1] for m in made]
    if edit is not None:
        edit(ris)
    batch = hb.PreparedBatch(ris, ns.W_MATCH, ns.H_MATCH)
    src = twin.triangulate_dense(batch, ns.params())
    out = (ris, batch, src, truth)
    if edit is None:
        _cache[key] = out
    return out


def window_cells(cell, H, W, R, same_side_of=None):
    """In-grid cells of the (2R + 1)^2 window of every cell; ``same_side_of``: only those on the cell's side of that column."""
    y, x = cell // W, cell % W
    n = np.zeros(cell.shape, np.int64)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            ok = (y + dy >= 0) & (y + dy < H) & (x + dx >= 0) & (x + dx < W)
            if same_side_of is not None:
                ok &= ((x + dx) >= same_side_of) == (x >= same_side_of)
            n += ok
    return n


def truth_normals(src, truth, H, W):
    off = np.asarray(src.ref_offsets)
    cell = src.cell.numpy().astype(np.int64)
    return np.concatenate([truth[r]["normal"].reshape(H * W, 3)[cell[off[r]:off[r + 1]]] for r in range(len(truth))])


def view_dot(src, normals, ris):
    off = np.asarray(src.ref_offsets)
    C = np.concatenate([np.repeat(np.asarray(ns.cameras()[ri.ref_cam].C, np.float64)[None, :], off[r + 1] - off[r], axis=0) for r, ri in enumerate(ris)])
    return ((C - src.xyz.numpy().astype(np.float64)) * normals.astype(np.float64)).sum(axis=1)


@pytest.mark.parametrize("R", [1, 4])
@pytest.mark.parametrize("channels", [2, 4])
@pytest.mark.parametrize("H,W", [(20, 24), (6, 8)])
def test_noise_free_planes(twin, H, W, channels, R):
    for tilt in (0.0, 40.0, 75.0):
        ris, batch, src, truth = probe(twin, "plane", H, W, channels, tilt)
        assert src.count == len(REFS) * H * W                    # every cell of both references made a point
        counters = torch.zeros(2, dtype=torch.int64)
        res, status = twin.estimate_normals(batch, src, R, PLANE_STEP, ns.THR, with_status=True, counters=counters)
        nrm, st = res.normals.numpy(), status.numpy()
        cell = src.cell.numpy().astype(np.int64)
        # no exclusions: the status is the number of in-grid window cells, fitted
        assert np.array_equal(st, window_cells(cell, H, W, R) | 0x80)
        assert counters.tolist() == [src.count, 0]
        ref = nr.over_references(ns.cameras(), ris, src, ns.W_MATCH, ns.H_MATCH, R, PLANE_STEP, ns.THR)
        assert not ref["flagged"].any() and np.array_equal(ref["status"], st.astype(np.int64))
        want = truth_normals(src, truth, H, W)
        assert (ns.angle(ref["normal"], want) <= 0.1 * ref["bound"]).all()      # the scene itself: rounding the warps to f32 is small against the bound
        ang = ns.angle(nrm, want)
        print(f"{W}x{H} c{channels} R{R} tilt {tilt}: max angle to the analytic normal {ang.max():.3e} rad, bound {ref['bound'].min():.3e} .. "
              f"{ref['bound'].max():.3e}, worst ratio {(ang / ref['bound']).max():.4f}")
        assert (ang <= ref["bound"]).all()
        assert (ns.angle(nrm, ref["normal"]) <= ref["bound"]).all()
        assert (np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1.0) <= 2.0 ** -22).all()
        assert (view_dot(src, nrm, ris) > 0).all()
        # the points are not touched, a second call gives the same bits
        again = twin.estimate_normals(batch, src, R, PLANE_STEP, ns.THR)
        assert np.array_equal(ns.bits(again.normals), ns.bits(res.normals)) and again.xyz is src.xyz


@pytest.mark.parametrize("R", [1, 4])
def test_the_window_stops_at_a_depth_step(twin, R):
    H, W = 20, 24
    ris, batch, src, truth = probe(twin, "slab", H, W)
    assert src.count == len(REFS) * H * W
    res, status = twin.estimate_normals(batch, src, R, 0.05, ns.THR, with_status=True)
    cell = src.cell.numpy().astype(np.int64)
    own_side = window_cells(cell, H, W, R, same_side_of=W // 2)
    whole = window_cells(cell, H, W, R)
    st = status.numpy()
    assert np.array_equal(st & 0x7f, own_side) and ((st & 0x80) != 0).all()
    x = cell % W
    far = (x < W // 2 - R) | (x >= W // 2 + R)                   # at least R cells from the step: the whole window
    assert np.array_equal((st & 0x7f)[far], whole[far]) and ((st & 0x7f)[~far] < whole[~far]).all()
    ref = nr.over_references(ns.cameras(), ris, src, ns.W_MATCH, ns.H_MATCH, R, 0.05, ns.THR)
    assert not ref["flagged"].any() and np.array_equal(ref["status"], st.astype(np.int64))
    assert (ns.angle(res.normals.numpy(), truth_normals(src, truth, H, W)) <= ref["bound"]).all()


def test_the_crease_keeps_two_orientations(twin):
    """Away from the crease line every window lies on one plane: that plane's normal, within the bound."""
    H, W, R = 20, 24, 1
    ris, batch, src, truth = probe(twin, "crease", H, W, 4)
    res, status = twin.estimate_normals(batch, src, R, PLANE_STEP, ns.THR, with_status=True)
    ref = nr.over_references(ns.cameras(), ris, src, ns.W_MATCH, ns.H_MATCH, R, PLANE_STEP, ns.THR)
    assert np.array_equal(ref["status"], status.numpy().astype(np.int64))
    assert (ns.angle(res.normals.numpy(), ref["normal"]) <= ref["bound"]).all()
    x = src.cell.numpy().astype(np.int64) % W
    away = np.abs(x - (W - 1) / 2.0) > R + 1
    want = truth_normals(src, truth, H, W)
    assert away.sum() > 0.6 * src.count and (ns.angle(res.normals.numpy(), want)[away] <= ref["bound"][away]).all()


def _fallback_of(src, ris):
    off = np.asarray(src.ref_offsets)
    X = src.xyz.numpy().astype(np.float64)
    out = np.zeros_like(X)
    for r, ri in enumerate(ris):
        V = np.asarray(ns.cameras()[ri.ref_cam].C, np.float32).astype(np.float64)[None, :] - X[off[r]:off[r + 1]]
        with np.errstate(all="ignore"):
            l = np.linalg.norm(V, axis=1)
            out[off[r]:off[r + 1]] = np.where((np.isfinite(l) & (l > 0))[:, None], V / l[:, None], 0.0)
    return np.nan_to_num(out, nan=0.0, posinf=0.0, neginf=0.0)


def _is_fallback(nrm, want):
    """Components within one f32 ulp of the rounded f64 unit view vector."""
    w32 = want.astype(np.float32)
    return (np.abs(nrm.astype(np.float64) - w32) <= np.spacing(np.maximum(np.abs(w32), np.float32(1e-30)))).all(axis=1)


@pytest.mark.parametrize("how", ["mask_a", "zero_cert"])
def test_a_single_live_row_is_collinear(twin, how):
    H, W, R, y0 = 20, 24, 4, 7

    def edit(ris):
        for ri in ris:
            if how == "mask_a":
                m = torch.zeros((ns.H_MATCH, ns.W_MATCH), dtype=torch.uint8)
                m[(ns.H_MATCH // H) * y0:(ns.H_MATCH // H) * (y0 + 1), :] = 1
                ri.mask_a = m
            else:
                for c in ri.cert:
                    c[:y0] = 0.0
                    c[y0 + 1:] = 0.0

    ris, batch, src, _truth = probe(twin, "plane", H, W, 2, 40.0, edit=edit)
    cell = src.cell.numpy().astype(np.int64)
    if how == "mask_a":
        assert src.count == len(REFS) * W and (cell // W == y0).all()
    else:
        assert src.count == len(REFS) * H * W                   # the dense call floors the certainty: every cell makes a point, one row is live
    counters = torch.zeros(2, dtype=torch.int64)
    res, status = twin.estimate_normals(batch, src, R, PLANE_STEP, ns.THR, with_status=True, counters=counters)
    x = cell % W
    in_row = (np.minimum(x + R, W - 1) - np.maximum(x - R, 0) + 1) * (np.abs(cell // W - y0) <= R)
    assert np.array_equal(status.numpy().astype(np.int64), in_row)            # counted, not fitted
    assert _is_fallback(res.normals.numpy(), _fallback_of(src, ris)).all()
    assert counters.tolist() == [0, src.count]
    ref = nr.over_references(ns.cameras(), ris, src, ns.W_MATCH, ns.H_MATCH, R, PLANE_STEP, ns.THR)
    assert np.array_equal(ref["status"], status.numpy().astype(np.int64))


def test_points_the_guard_stops(twin):
    H, W, R = 20, 24, 1
    ris, batch, src, _truth = probe(twin, "plane", H, W, 2, 40.0)
    cell, slot, xyz = src.cell.clone(), src.slot.clone(), src.xyz.clone()
    cell[3], cell[4], cell[5] = -1, H * W, 2 ** 31 - 1
    slot[6], slot[7] = K, 255
    xyz[8, 1] = float("nan")
    xyz[9, 0] = float("inf")
    cam = ns.cameras()[ris[0].ref_cam]
    xyz[10] = torch.from_numpy(np.asarray(cam.C, np.float32) - 2.0 * (src.xyz[10].numpy() - np.asarray(cam.C, np.float32)))     # behind the reference
    xyz[11] = torch.from_numpy(np.asarray(cam.C, np.float32))                                                          # at its centre
    bad = dataclasses.replace(src, cell=cell, slot=slot, xyz=xyz, _packed=None)
    keep = [t.clone() for t in (bad.xyz, bad.rgb, bad.err, bad.cell, bad.slot)]
    res, status = twin.estimate_normals(batch, bad, R, PLANE_STEP, ns.THR, with_status=True)
    st, nrm = status.numpy(), res.normals.numpy()
    assert (st[3:12] == 0).all()
    want = _fallback_of(bad, ris)
    assert _is_fallback(nrm[3:8], want[3:8]).all() and _is_fallback(nrm[10:11], want[10:11]).all()
    assert (nrm[8:10] == 0).all() and (nrm[11] == 0).all()       # |Vw| not finite, or zero
    good, st_good = twin.estimate_normals(batch, src, R, PLANE_STEP, ns.THR, with_status=True)
    rest = np.ones(src.count, bool)
    rest[3:12] = False
    assert np.array_equal(ns.bits(res.normals)[rest], ns.bits(good.normals)[rest]) and np.array_equal(st[rest], st_good.numpy()[rest])
    for a, b in zip(keep, (bad.xyz, bad.rgb, bad.err, bad.cell, bad.slot)):
        assert np.array_equal(ns.bits(a), ns.bits(b))            # nothing of the input is written
    ref = nr.over_references(ns.cameras(), ris, bad, ns.W_MATCH, ns.H_MATCH, R, PLANE_STEP, ns.THR)
    assert np.array_equal(ref["status"], st.astype(np.int64))


def test_a_nan_warp_skips_its_cell_only(twin):
    H, W, R = 20, 24, 1
    hole = 9 * W + 11

    def edit(ris):
        for w in ris[0].warp:
            w.reshape(H * W, -1)[hole, -1] = float("nan")

    ris, batch, src, truth = probe(twin, "plane", H, W, 2, 40.0, edit=edit)
    assert src.count == len(REFS) * H * W - 1
    res, status = twin.estimate_normals(batch, src, R, PLANE_STEP, ns.THR, with_status=True)
    cell = src.cell.numpy().astype(np.int64)
    first = np.arange(src.count) < int(src.ref_offsets[1])
    near = first & (np.abs(cell // W - 9) <= R) & (np.abs(cell % W - 11) <= R)
    want = window_cells(cell, H, W, R) - near
    assert near.sum() == 8 and np.array_equal(status.numpy().astype(np.int64), want | 0x80)
    assert np.isfinite(res.normals.numpy()).all()
    ref = nr.over_references(ns.cameras(), ris, src, ns.W_MATCH, ns.H_MATCH, R, PLANE_STEP, ns.THR)
    assert np.array_equal(ref["status"], status.numpy().astype(np.int64))
    assert (ns.angle(res.normals.numpy(), truth_normals(src, truth, H, W)) <= ref["bound"]).all()


def test_an_empty_reference_and_an_empty_cloud(twin):
    H, W, R = 6, 8, 1

    def edit(ris):
        for w in ris[0].warp:                                   # no cell of the first reference passes the two-view test
            w.fill_(float("nan"))

    ris, batch, src, _truth = probe(twin, "plane", H, W, 2, 0.0, edit=edit)
    assert src.ref_offsets.tolist() == [0, 0, H * W]
    counters = torch.zeros(2, dtype=torch.int64)
    res, status = twin.estimate_normals(batch, src, R, PLANE_STEP, ns.THR, with_status=True, counters=counters)
    assert np.array_equal(status.numpy().astype(np.int64), window_cells(src.cell.numpy().astype(np.int64), H, W, R) | 0x80)
    assert counters.tolist() == [H * W, 0]
    none = dataclasses.replace(src, xyz=src.xyz[:0], rgb=src.rgb[:0], err=src.err[:0], cell=src.cell[:0], slot=src.slot[:0],
                               ref_offsets=np.zeros(3, np.int64), _packed=None)
    res, status = twin.estimate_normals(batch, none, R, PLANE_STEP, ns.THR, with_status=True, counters=counters)
    assert res.normals.shape == (0, 3) and status.numel() == 0 and counters.tolist() == [H * W, 0]


def test_a_wider_window_is_more_accurate_on_a_noisy_plane(twin):
    H = W = 128
    ris, batch, src, truth = probe(twin, "plane", H, W, 2, 40.0, noise=0.5, refs=(10,))
    want = truth_normals(src, truth, H, W)
    med = {}
    for R in (1, 3):
        res, status = twin.estimate_normals(batch, src, R, 0.05, ns.THR, with_status=True)
        fitted = (status.numpy() & 0x80) != 0
        assert fitted.mean() > 0.9
        med[R] = float(np.median(ns.angle(res.normals.numpy(), want)[fitted]))
    print(f"noisy plane 128x128, 0.5 px: median angular error R=1 {np.degrees(med[1]):.2f} deg, R=3 {np.degrees(med[3]):.2f} deg")
    assert med[3] < med[1]


def _noisy(twin, spec, R):
    spec = dict(spec)
    kind, H, W = spec.pop("kind"), spec.pop("H"), spec.pop("W")
    ris = [ns.reference_inputs(kind, ref, K, H, W, **spec)[0] for ref in REFS]
    batch = hb.PreparedBatch(ris, ns.W_MATCH, ns.H_MATCH)
    src = twin.triangulate_dense(batch, ns.params())
    res, status = twin.estimate_normals(batch, src, R, ns.NOISY_STEP, ns.THR, with_status=True)
    ref = nr.over_references(ns.cameras(), ris, src, ns.W_MATCH, ns.H_MATCH, R, ns.NOISY_STEP, ns.THR)
    return src, res.normals.numpy(), status.numpy().astype(np.int64), ref


@pytest.mark.parametrize("R", [1, 3])
def test_the_noisy_scene_of_the_device_comparison_stays_inside_the_band_cap(twin, R):
    """The scene and seed tests/test_gpu_normals.py compares device and twin on: the reference alone flags at most BAND_CAP of the points, so
    that comparison is one of decisions every implementation must take alike - and the twin takes them."""
    src, nrm, st, ref = _noisy(twin, ns.NOISY, R)
    print(f"R{R}: {src.count} points, {int(ref['flagged'].sum())} flagged, {int(((st & 0x7f) < (2 * R + 1) ** 2).sum())} windows lost a cell")
    assert src.count > 800 and ref["flagged"].mean() <= support_scene.BAND_CAP
    assert ((st & 0x7f) < (2 * R + 1) ** 2).sum() > 0.1 * src.count          # the outliers do leave windows with fewer cells
    assert not ((st != ref["status"]) & ~ref["flagged"]).any()
    rest = ~ref["flagged"] & ref["fitted"]
    assert (ns.angle(nrm, ref["normal"])[rest] <= ref["bound"][rest]).all()


@pytest.mark.parametrize("R", [1, 3])
def test_outside_the_band_the_twin_takes_the_reference_s_decisions(twin, R):
    """Outliers along the epipolar lines put reprojection errors on both sides of the threshold and some inside the band: the reference flags
    those points, the twin may differ from it there and nowhere else."""
    src, nrm, st, ref = _noisy(twin, ns.IN_BAND, R)
    flagged = ref["flagged"]
    print(f"R{R}: {src.count} points, {int(flagged.sum())} flagged, twin != reference on {int((st != ref['status']).sum())}")
    assert 0 < flagged.sum() < 0.1 * src.count                                 # the band rule has something to decide, and most points are outside it
    assert not ((st != ref["status"]) & ~flagged).any()
    rest = ~flagged & ref["fitted"]
    assert (ns.angle(nrm, ref["normal"])[rest] <= ref["bound"][rest]).all()
    fell = ~flagged & ~ref["fitted"]
    assert _is_fallback(nrm[fell], ref["fallback"][fell]).all()


def test_buffers_hand_out_only_normals_written_for_their_current_points(twin):
    """OutputBuffers keep their normals tensor when they are reused: collect() reports it only while it belongs to the points they hold."""
    import ctypes as C
    H, W = 6, 8
    ris = [ns.reference_inputs("plane", ref, K, H, W, tilt_deg=40.0)[0] for ref in REFS]
    batch = hb.PreparedBatch(ris, ns.W_MATCH, ns.H_MATCH)
    buf = hb.OutputBuffers(len(REFS) * H * W, len(REFS), K, torch.device("cpu"))
    fill = lambda: twin._lib.lfd_triangulate_dense_host(twin._ctx, C.byref(batch.c), C.byref(ns.params()), C.byref(buf.c), buf.ref_offsets.data_ptr(),
                                                        buf.seg_counts.data_ptr())
    assert fill() == 0 and buf.collect().normals is None
    assert twin.estimate_normals(batch, buf, 1, PLANE_STEP, ns.THR) is buf
    got = buf.collect()
    assert got.normals.shape == (got.count, 3) and buf.normals_valid
    twin.refine_multiview(batch, buf, 1.6, ns.THR)             # moves points in place: the normals belong to the old positions
    assert buf.collect().normals is None and buf.normals is not None
    twin.estimate_normals(batch, buf, 1, PLANE_STEP, ns.THR)
    assert buf.collect().normals is not None
    into = twin.support_filter(batch, buf, 1, 1.6, into=buf.__class__(buf.capacity, len(REFS), K, torch.device("cpu")))
    assert into.collect().normals is None                      # a filter's destination starts without
    twin.estimate_normals(batch, into, 1, PLANE_STEP, ns.THR)
    assert into.collect().normals is not None
    twin.support_filter(batch, buf, 1, 1.6, into=into)         # refilled
    assert into.collect().normals is None
