"""CPU tier of the multi-view colour (lfd_colour_multiview_host): the twin against the NumPy reference of tests/colour_ref.py
bit for bit on the rendered plane of tests/colour_scene.py - both modes, 2- and 4-channel warps, masks on and off, k = 3 and k = LFD_MAX_SLOTS,
in place against out of place - the view set against the support filter's, the guards, and what the stage is for: the colour of a point seen
under different exposures, and with an occluder in one view."""
import ctypes as C

import numpy as np
import pytest
import torch

import colour_ref
import colour_scene as cs
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

TAU = 1.6
MATCH = 96


@pytest.fixture(scope="module")
def twin():
    d = hb.HostDensifier(2)
    d.upload_cameras(cs.cameras())
    yield d
    d.close()


_made = {}


def case(k, channels, masks):
    """Two references of 12 x 16 cells with 0.6 px matching noise (so that the other neighbours confirm some points and not others), their
    batch and the twin's dense points - made once per shape."""
    key = (k, channels, masks)
    if key not in _made:
        scenes = [cs.make(r, k, 12, 16, match=MATCH, channels=channels, masks=masks, noise_px=0.6, gains=[1.0 + 0.03 * ((j * 7) % 5 - 2) for j in range(k + 1)])
                  for r in (5, 21)]
        _made[key] = scenes
    return _made[key]


def dense_points(twin, scenes):
    batch = hb.PreparedBatch([s.inputs for s in scenes], MATCH, MATCH)
    return batch, twin.triangulate_dense(batch, cs.params())


@pytest.mark.parametrize("mode", ["mean", "median"])
@pytest.mark.parametrize("k,channels,masks", [(3, 2, False), (3, 4, True), (16, 2, True), (16, 4, False)])
def test_twin_equals_the_reference_bit_for_bit(twin, k, channels, masks, mode):
    scenes = case(k, channels, masks)
    batch, res = dense_points(twin, scenes)
    assert res.count > 300
    counters = torch.zeros(2, dtype=torch.int64)
    out, status = twin.colour_multiview(batch, res, TAU, mode, with_status=True, counters=counters)
    want, want_status = colour_ref.batch_reference(cs.cameras(), [s.inputs for s in scenes], [s.images for s in scenes], MATCH, MATCH, res, TAU, mode)
    st = status.numpy()
    assert np.array_equal(st, want_status)
    assert np.array_equal(cs.bits(out.rgb), cs.bits(want))
    assert counters.tolist() == [int((st > 0).sum()), int(st.astype(np.int64).sum())]
    for name in ("xyz", "err", "cell", "slot"):                      # a column rewrite: everything else is the input's
        assert np.array_equal(cs.bits(getattr(out, name)), cs.bits(getattr(res, name)))
    assert np.array_equal(out.ref_offsets, res.ref_offsets)
    seen = set(st.tolist())
    assert any(n % 2 == 0 for n in seen) and any(n % 2 == 1 for n in seen) and 0 not in seen       # both parities of n
    if k == 16:
        assert max(seen) >= 12, seen                                 # many views per point (17 without noise and masks)
    # the view set is the support filter's: winner + reference + the slots it counts
    _kept, support = twin.support_filter(batch, res, 1, TAU, with_support=True)
    assert np.array_equal(st, support.numpy() + 2)


def test_all_seventeen_views(twin):
    """Without noise and masks every one of the 16 neighbours confirms every point: n = LFD_MAX_SLOTS + 1, the last entry of the 1 / n table."""
    scenes = [cs.make(7, 16, 6, 8, match=MATCH)]
    batch, res = dense_points(twin, scenes)
    for mode in ("mean", "median"):
        out, status = twin.colour_multiview(batch, res, TAU, mode, with_status=True)
        want, want_status = colour_ref.batch_reference(cs.cameras(), [scenes[0].inputs], [scenes[0].images], MATCH, MATCH, res, TAU, mode)
        assert (status.numpy() == 17).all() and np.array_equal(status.numpy(), want_status)
        assert np.array_equal(cs.bits(out.rgb), cs.bits(want))


@pytest.mark.parametrize("mode", ["mean", "median"])
def test_in_place_equals_out_of_place(twin, mode):
    scenes = case(3, 2, False)
    batch = hb.PreparedBatch([s.inputs for s in scenes], MATCH, MATCH)
    cap = 2 * 12 * 16
    src = hb.OutputBuffers(cap, 2, 3, torch.device("cpu"))
    assert twin._lib.lfd_triangulate_dense_host(twin._ctx, C.byref(batch.c), C.byref(cs.params()), C.byref(src.c), src.ref_offsets.data_ptr(),
                                                src.seg_counts.data_ptr()) == 0
    res = src.collect()
    apart = twin.colour_multiview(batch, res, TAU, mode)                     # a collected result: a copy with a new rgb tensor
    assert apart.rgb.data_ptr() != res.rgb.data_ptr()
    xyz = src.xyz.clone()
    same = twin.colour_multiview(batch, src, TAU, mode)                      # the buffers: rewritten where they are
    assert same is src
    n = res.count
    assert np.array_equal(cs.bits(src.rgb[:n]), cs.bits(apart.rgb)) and np.array_equal(cs.bits(src.xyz), cs.bits(xyz))


@pytest.mark.parametrize("mode", ["mean", "median"])
def test_guarded_points_keep_their_bits(twin, mode):
    scenes = case(3, 2, False)
    batch, res = dense_points(twin, scenes)
    n0 = int(res.ref_offsets[1])
    HW = 12 * 16
    xyz, rgb, cell, slot = res.xyz.clone(), res.rgb.clone(), res.cell.clone(), res.slot.clone()
    xyz[3, 1] = float("nan")
    xyz[4, 0] = float("inf")
    rgb.view(torch.int32)[5, 2] = 0x7fc01234                                 # a NaN with a payload: it must come back bit for bit
    rgb[6, 0] = float("-inf")
    cell[7] = -1
    cell[8] = HW
    cell[n0 + 1] = 2 ** 31 - 1
    slot[9] = 3                                                              # n_slots of every reference is 3
    slot[n0 + 2] = 255
    bad = [3, 4, 5, 6, 7, 8, 9, n0 + 1, n0 + 2]
    import dataclasses
    hurt = dataclasses.replace(res, xyz=xyz, rgb=rgb, cell=cell, slot=slot, _packed=None)
    counters = torch.zeros(2, dtype=torch.int64)
    out, status = twin.colour_multiview(batch, hurt, TAU, mode, with_status=True, counters=counters)
    clean, clean_status = twin.colour_multiview(batch, res, TAU, mode, with_status=True)
    st = status.numpy()
    assert (st[bad] == 0).all()
    assert np.array_equal(cs.bits(out.rgb)[bad], cs.bits(rgb)[bad])
    good = np.setdiff1d(np.arange(res.count), bad)
    assert np.array_equal(st[good], clean_status.numpy()[good]) and np.array_equal(cs.bits(out.rgb)[good], cs.bits(clean.rgb)[good])
    assert counters.tolist() == [len(good), int(st.astype(np.int64).sum())]
    want, want_status = colour_ref.batch_reference(cs.cameras(), [s.inputs for s in scenes], [s.images for s in scenes], MATCH, MATCH, hurt, TAU, mode)
    assert np.array_equal(st, want_status) and np.array_equal(cs.bits(out.rgb), cs.bits(want))


def test_winner_with_a_non_finite_observation_is_left_out(twin):
    scenes = [cs.make(5, 3, 12, 16, match=MATCH)]
    batch, res = dense_points(twin, scenes)
    i = 20
    s, c = int(res.slot[i]), int(res.cell[i])
    ri = scenes[0].inputs
    hurt = cs.to_device(ri, "cpu")
    hurt.warp[s] = ri.warp[s].clone()
    hurt.warp[s].view(-1, 2)[c, 0] = float("nan")
    b2 = hb.PreparedBatch([hurt], MATCH, MATCH)
    out, status = twin.colour_multiview(b2, res, TAU, "mean", with_status=True)
    ref, ref_status = twin.colour_multiview(batch, res, TAU, "mean", with_status=True)
    assert int(ref_status[i]) == 4 and int(status[i]) == 3
    want, want_status = colour_ref.batch_reference(cs.cameras(), [hurt], [scenes[0].images], MATCH, MATCH, res, TAU, "mean")
    assert np.array_equal(status.numpy(), want_status) and np.array_equal(cs.bits(out.rgb), cs.bits(want))


def inside_all(sc, res, H, W):
    """Points whose observation lies inside the image in every neighbour (the support test does not ask for that: a view whose observation
    lies off its image takes part with the clamped border colour, as the reference's own sample does at its border)."""
    cell = res.cell.numpy().astype(np.int64)
    ok = np.ones(cell.shape, bool)
    for w in sc.inputs.warp:
        wj = w.numpy().reshape(H * W, -1)[cell]
        ok &= (np.abs(wj[:, -2]) <= 1.0) & (np.abs(wj[:, -1]) <= 1.0)
    return ok


def test_effect():
    """What the stage buys, on a 256^2 rendering of the plane seen by a reference and three neighbours, no matching noise.

    The albedo a(X) has |grad a| <= G = ALBEDO_GRAD per scene unit (amplitude times the norm of the two frequencies).  A view with gain g
    stores round(255 g a) / 255 per pixel: the stored value differs from g a at the pixel's plane point by at most 0.5 / 255.  The four taps of
    a bilinear sample lie within one pixel of the sample position in x and in y, i.e. within d on the plane, d the largest distance between the
    plane points of diagonal pixel neighbours of that view (colour_scene.pixel_footprint, from the scene's geometry); the blend is a convex
    combination of them, so a view's sample differs from g a(X) by at most

        e = g_max G d + 0.5 / 255 (+ 1e-5 for the f32 arithmetic of position and blend)

    The reference's colour is such a sample too.  Asserted over the points that all four views blend and that lie inside all four images.  With gains whose mean over the four views is exactly 1 - (1.15, 0.85, 1, 1) - the mean of the
    samples is a(X) + mean of the errors: within e of the albedo.  The reference's own colour is 1.15 a(X) + error, at least 0.15 a_min - e
    away, a_min = 0.4.  With every gain 1 and an occluder of constant colour painted into one neighbour's image, three of the four values lie
    within e of a(X); the median - the mean of the two middle ones - lies between two of those three, hence within e, while the mean is
    dragged by a quarter of the occluder's distance from the albedo: at least 0.2 / 4 in the channel where the occluder is farthest.

    Measured: d = 0.0714, e = 0.0136; largest error of the mean 0.0016, smallest error of the reference's colour 0.0583; with
    the occluder: median at most 0.0018 anywhere, mean at least 0.1407 off in some channel at every point behind the patch."""
    match, H, W, k = 256, 40, 48, 3
    cams = cs.cameras()
    twin = hb.HostDensifier(2)
    twin.upload_cameras(cams)
    try:
        gains = (1.15, 0.85, 1.0, 1.0)
        assert sum(gains) / 4 == 1.0
        sc = cs.make(12, k, H, W, match=match, gains=gains)
        d = max(cs.pixel_footprint(cams[c], match) for c in [sc.ref] + sc.nbrs)
        e = max(gains) * cs.ALBEDO_GRAD * d + 0.5 / 255 + 1e-5
        batch = hb.PreparedBatch([sc.inputs], match, match)
        res = twin.triangulate_dense(batch, cs.params())
        truth = sc.truth.reshape(-1, 3)[res.cell.numpy().astype(np.int64)]
        out, status = twin.colour_multiview(batch, res, TAU, "mean", with_status=True)
        full = (status.numpy() == k + 1) & inside_all(sc, res, H, W)
        assert full.sum() > 0.75 * H * W
        err_mean = np.abs(out.rgb.numpy().astype(np.float64) - truth)[full]
        err_single = np.abs(res.rgb.numpy().astype(np.float64) - truth)[full]
        print(f"bound e = {e:.4f} (d = {d:.4f}); mean mode: largest error {err_mean.max():.4f}; single view: smallest error {err_single.min():.4f}")
        assert e < 0.15 * 0.4 - e                                         # the bound separates the two
        assert err_mean.max() <= e
        assert err_single.min() > e
        # an occluder in neighbour 1's image, every gain 1
        patch = (60, 200, 60, 200)
        sc = cs.make(12, k, H, W, match=match, patch_in=1, patch=patch)
        batch = hb.PreparedBatch([sc.inputs], match, match)
        res = twin.triangulate_dense(batch, cs.params())
        truth = sc.truth.reshape(-1, 3)[res.cell.numpy().astype(np.int64)]
        mean, status = twin.colour_multiview(batch, res, TAU, "mean", with_status=True)
        median = twin.colour_multiview(batch, res, TAU, "median")
        wj = sc.inputs.warp[1].numpy().reshape(H * W, -1)[res.cell.numpy().astype(np.int64)]
        px, py = (wj[:, -2] + 1.0) * 0.5 * (match - 1), (wj[:, -1] + 1.0) * 0.5 * (match - 1)
        seen = (status.numpy() == k + 1) & inside_all(sc, res, H, W)
        behind = seen & (px > patch[2] + 1) & (px < patch[3] - 2) & (py > patch[0] + 1) & (py < patch[1] - 2)
        assert behind.sum() > 100
        err_median = np.abs(median.rgb.numpy().astype(np.float64) - truth)
        err_mean = np.abs(mean.rgb.numpy().astype(np.float64) - truth)
        print(f"occluder: median largest error {err_median[seen].max():.4f}; mean behind the patch: smallest of the per-point "
              f"largest channel error {err_mean[behind].max(axis=1).min():.4f}")
        assert err_median[seen].max() <= e              # everywhere, behind the patch included
        assert err_mean[behind].max(axis=1).min() > e                      # where the mean does not
    finally:
        twin.close()
