"""CPU tier of the far-field shell: the twins (lfd_far_accumulate_host, lfd_far_emit_host) against the NumPy reference of
tests/far_ref.py - tables equal element for element, records bit for bit - on the analytic outdoor scene of tests/far_scene.py, and what the
feature is for: the sky the triangulation drops comes out as a shell, the ground does not, one neighbour that sees parallax vetoes."""
import numpy as np
import pytest
import torch

import colour_scene as cs
import far_ref
import far_scene as fs
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

TAU, CERT, VIEWS, S, MIN_SAMPLES = 0.8, 0.5, 2, 256, 2          # the knobs' defaults (core/types.py; reproj_thresh = 0.8)
MATCH = 64


@pytest.fixture(scope="module")
def twin():
    d = hb.HostDensifier(2)
    d.upload_cameras(fs.cameras())
    yield d
    d.close()


def u64(t):
    return t.cpu().numpy().view(np.uint64)


_made = {}


def case(channels, masks, H=24, W=40):
    """Three references with 1, 3 and 2 neighbours."""
    key = (channels, masks, H, W)
    if key not in _made:
        _made[key] = [fs.make(r, fs.others(r, n), H, W, match=MATCH, channels=channels, masks=masks) for r, n in ((0, 1), (1, 3), (2, 2))]
    return _made[key]


@pytest.mark.parametrize("channels,masks,S_", [(2, False, 256), (4, True, 32), (2, True, 8), (4, False, 256)])
def test_twin_equals_the_reference_element_for_element(twin, channels, masks, S_):
    scenes = case(channels, masks)
    refs = [s.inputs for s in scenes]
    batch = hb.PreparedBatch(refs, MATCH, MATCH)
    counters = torch.zeros(3, dtype=torch.int64)
    table = twin.far_accumulate(batch, TAU, CERT, VIEWS, S_, counters=counters)
    want, want_counters, per = far_ref.accumulate(fs.cameras(), refs, MATCH, MATCH, TAU, CERT, VIEWS, S_)
    assert table.dtype == torch.int64 and tuple(table.shape) == (6 * S_ * S_, 7)
    assert np.array_equal(u64(table), want)
    assert np.array_equal(counters.numpy(), want_counters) and want_counters.min() > 50
    assert all((~c["far"]).sum() > 50 for c in per)
    # accumulating twice equals the doubled table (two's complement: the direction columns double as integers)
    again = twin.far_accumulate(batch, TAU, CERT, VIEWS, S_, table=table, counters=counters)
    assert again is table and np.array_equal(table.numpy(), 2 * want.view(np.int64)) and np.array_equal(counters.numpy(), 2 * want_counters)


def test_nan_entries_and_targets_outside_are_not_confident(twin):
    scenes = case(2, False)
    refs = []
    for s in scenes:
        ri = s.inputs
        cert, warp = [c.clone() for c in ri.cert], [w.clone() for w in ri.warp]
        cert[0][2, 3:9] = float("nan")
        warp[0][3, 5:11, 0] = float("nan")
        warp[-1][4, 7:13, 1] = float("inf")
        warp[0][5, 2:8, 0] = 1.5                                       # outside the neighbour's grid
        refs.append(hb.ReferenceInputs(ref_cam=ri.ref_cam, nbr_cams=ri.nbr_cams, cert=cert, warp=warp, image=ri.image))
    batch = hb.PreparedBatch(refs, MATCH, MATCH)
    table = twin.far_accumulate(batch, TAU, CERT, VIEWS, 32)
    want, _c, per = far_ref.accumulate(fs.cameras(), refs, MATCH, MATCH, TAU, CERT, VIEWS, 32)
    assert np.array_equal(u64(table), want)
    plain, _c2, per_plain = far_ref.accumulate(fs.cameras(), [s.inputs for s in scenes], MATCH, MATCH, TAU, CERT, VIEWS, 32)
    assert not np.array_equal(plain, want)
    far0, was0 = per[0]["far"].reshape(24, 40), per_plain[0]["far"].reshape(24, 40)
    assert was0[2, 3:9].all() and not far0[2, 3:9].any()               # reference 0 has one neighbour: without it nothing is confident
    assert was0[5, 2:8].all() and not far0[5, 2:8].any()


@pytest.mark.parametrize("S_,min_samples", [(32, 1), (32, 3), (256, 1)])
def test_emit_equals_the_reference_bit_for_bit(twin, S_, min_samples):
    refs = [s.inputs for s in case(2, False)]
    table = twin.far_accumulate(hb.PreparedBatch(refs, MATCH, MATCH), TAU, CERT, VIEWS, S_)
    centre, radius = np.array([0.3, -0.2, 0.1]), 12.5
    keys, xyz, rgb, nrm, smp = far_ref.emit(u64(table), S_, min_samples, centre, radius)
    assert keys.size > 10
    for with_normals in (False, True):
        got = twin.far_emit(table, S_, min_samples, centre, radius, with_normals=with_normals)
        assert np.array_equal(cs.bits(got[0]), cs.bits(xyz)) and np.array_equal(cs.bits(got[1]), cs.bits(rgb))
        assert np.array_equal(got[3].numpy(), smp)
        assert (got[2] is None) if not with_normals else np.array_equal(cs.bits(got[2]), cs.bits(nrm))
    # the records lie on the sphere and look inwards
    assert np.allclose(np.linalg.norm(xyz.astype(np.float64) - centre, axis=1), radius, rtol=1e-6)
    assert np.allclose((xyz.astype(np.float64) - centre) / radius, -nrm.astype(np.float64), atol=1e-6)


def test_emit_of_an_empty_table_and_of_too_large_a_threshold_is_empty(twin):
    table = hb.far_table(8, torch.device("cpu"))
    assert twin.far_emit(table, 8, 1, (0.0, 0.0, 0.0), 1.0)[0].shape[0] == 0
    refs = [s.inputs for s in case(2, False)]
    table = twin.far_accumulate(hb.PreparedBatch(refs, MATCH, MATCH), TAU, CERT, VIEWS, 8)
    assert int(table[:, 6].max()) > 0
    assert twin.far_emit(table, 8, int(table[:, 6].max()) + 1, (0.0, 0.0, 0.0), 1.0)[0].shape[0] == 0


# ---- what the feature is for -----------------------------------------------------------------------------------------------------------------
def test_effect(twin):
    """Four references of 48 x 64 cells with three neighbours each, every knob at its default.

    The knob-off cloud has no point from the upper half; no ground cell is far; every upper-half cell that is confident in at least
    far_min_views slots is far; the shell covers every direction cell the backdrop's cells give at least far_min_samples samples; its colour
    is the backdrop's.  The colour comparison takes the direction cells all of whose samples blend backdrop pixels only: the cells of the grid
    row at the horizon blend the ground's pixels in by the four-tap sampling itself.  Observed: largest difference between a direction cell's
    mean colour and the backdrop's texture averaged over the cell 0.70 grey levels (asserted: 1)."""
    H, W = 48, 64
    cams = fs.cameras()
    scenes = [fs.make(r, fs.others(r, 3), H, W, match=MATCH) for r in range(4)]
    refs = [s.inputs for s in scenes]
    batch = hb.PreparedBatch(refs, MATCH, MATCH)
    # the gap this closes: the triangulation emits nothing for the upper half
    res = twin.triangulate_dense(batch, cs.params())
    off = np.asarray(res.ref_offsets)
    assert res.count > 2000
    for r, s in enumerate(scenes):
        cell = res.cell.numpy()[off[r]:off[r + 1]]
        assert cell.size > 500 and not s.upper.reshape(-1)[cell].any()
    # ground: its disparity f b / depth against every neighbour is far above the threshold (depth <= 3.2 along the axis, b >= BASELINE)
    assert cams[0].K[0, 0] * fs.BASELINE / 3.2 > 20 * TAU
    table = twin.far_accumulate(batch, TAU, CERT, VIEWS, S)
    want, _counters, per = far_ref.accumulate(cams, refs, MATCH, MATCH, TAU, CERT, VIEWS, S)
    assert np.array_equal(u64(table), want)
    n_upper_far = 0
    for s, c in zip(scenes, per):
        upper, far = s.upper.reshape(-1), c["far"]
        assert not far[~upper].any()
        confident = upper & (c["n_conf"] >= VIEWS)
        assert far[confident].all() and not far[upper & ~confident].any()
        assert confident.sum() > 0.5 * upper.sum() and (upper & ~confident).sum() > 0
        n_upper_far += int(far.sum())
    assert n_upper_far > 4000
    # the shell covers the direction cells the backdrop subtends with enough samples
    centre = np.mean([np.asarray(c.C, np.float64) for c in cams], axis=0)
    xyz, rgb, _n, samples = twin.far_emit(table, S, MIN_SAMPLES, centre, 100.0)
    key_all = np.concatenate([c["key"][c["far"]] for c in per])
    kk, cnt = np.unique(key_all, return_counts=True)
    expect = kk[cnt >= MIN_SAMPLES]
    got_keys = far_ref.emit(want, S, MIN_SAMPLES, centre, 100.0)[0]
    assert np.array_equal(got_keys, expect) and xyz.shape[0] == expect.size > 300
    assert np.array_equal(samples.numpy(), cnt[cnt >= MIN_SAMPLES])
    # every shell point lies in front of the rig, above the horizon, in the direction of its cells
    dirs = (xyz.numpy().astype(np.float64) - centre) / 100.0
    assert (dirs[:, 1] > 0.5).all() and (dirs[:, 2] > -0.02).all()
    # colour: the backdrop's texture averaged over the direction cell (a 4 x 4 lattice of directions inside it)
    clean = {}
    for s, c in zip(scenes, per):
        cam = cams[s.ref]
        idx = np.nonzero(c["far"])[0]
        yy, xx = np.divmod(idx, W)
        ax, ay = far_ref.axis(W).astype(np.float64), far_ref.axis(H).astype(np.float64)
        x_px, y_px = (ax[xx] + 1.0) * 0.5 * (MATCH - 1), (ay[yy] + 1.0) * 0.5 * (MATCH - 1)
        taps_up = np.ones(idx.size, bool)
        for dx in (0, 1):
            for dy in (0, 1):
                tx, ty = np.minimum(np.floor(x_px) + dx, MATCH - 1), np.minimum(np.floor(y_px) + dy, MATCH - 1)
                taps_up &= fs.surface(cam, tx, ty, MATCH, MATCH)[1]
        for kx, ok in zip(c["key"][idx].tolist(), taps_up):
            clean[kx] = clean.get(kx, True) and bool(ok)
    tex = 255.0 * fs.backdrop_texture(far_ref.cell_directions(expect, S)).mean(axis=1)
    worst, compared = 0.0, 0
    for kx, col, t in zip(expect.tolist(), rgb.numpy().astype(np.float64), tex):
        if clean[kx]:
            worst = max(worst, float(np.abs(255.0 * col - t).max()))
            compared += 1
    print("direction cells compared:", compared, "of", expect.size, "largest colour difference [grey levels]:", worst)
    assert compared > 0.8 * expect.size
    assert worst <= 1.0


def test_one_confident_neighbour_that_sees_parallax_vetoes_its_cells(twin):
    """An occluder 3 units away, seen confidently by slot 0 of three; slots 1 and 2 see the backdrop there.  Its cells are not far; with slot
    0's certainty below far_certainty there, they are."""
    H, W = 24, 40
    occ = (0, 2, 8, 10, 24)
    s = fs.make(1, fs.others(1, 3), H, W, match=MATCH, occluder=occ)
    cams = fs.cameras()
    per = far_ref.cells(cams, s.inputs, MATCH, MATCH, TAU, CERT, VIEWS, 32)
    inside = s.occluded.reshape(-1)
    assert s.upper[2:8, 10:24].all() and per["conf"][inside].all()
    assert per["agree"][inside, 1].all() and per["agree"][inside, 2].all() and not per["agree"][inside, 0].any()
    table = twin.far_accumulate(hb.PreparedBatch([s.inputs], MATCH, MATCH), TAU, CERT, VIEWS, 32)
    want, _c, (c,) = far_ref.accumulate(cams, [s.inputs], MATCH, MATCH, TAU, CERT, VIEWS, 32)
    assert np.array_equal(u64(table), want) and not c["far"][inside].any() and c["far"][~inside & s.upper.reshape(-1)].any()
    ri = s.inputs
    cert = [x.clone() for x in ri.cert]
    cert[0][2:8, 10:24] = 0.3
    quiet = hb.ReferenceInputs(ref_cam=ri.ref_cam, nbr_cams=ri.nbr_cams, cert=cert, warp=ri.warp, image=ri.image)
    table2 = twin.far_accumulate(hb.PreparedBatch([quiet], MATCH, MATCH), TAU, CERT, VIEWS, 32)
    want2, _c, (c2,) = far_ref.accumulate(cams, [quiet], MATCH, MATCH, TAU, CERT, VIEWS, 32)
    assert np.array_equal(u64(table2), want2) and c2["far"][inside].all()
