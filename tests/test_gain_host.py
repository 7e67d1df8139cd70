"""CPU tier of the per-image exposure gains: the statistics twin (lfd_gain_accumulate_host) against the brute-force NumPy
reference of tests/gain_ref.py, uint64 tables equal element for element, on the rendered plane of tests/colour_scene.py; the apply twin
(lfd_gain_apply_host) against the NumPy rule, bit for bit; the solver (core/gains.py) on tables built from known factors; and what the
feature is for: four cameras at different exposures come out at one."""
import dataclasses
import math

import numpy as np
import pytest
import torch

import colour_scene as cs
import gain_ref
import gain_scene
from lichtfeld_densification_plugin_amd.core import gains
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
    """Two references of 12 x 16 cells with 0.6 px matching noise (other neighbours confirm some points and not others) and gains between 0.8
    and 1.35: 1.35 x albedo (up to 0.8) passes 0.95 - and clips at 1 - in part of the image, so some samples count and some do not."""
    key = (k, channels, masks)
    if key not in _made:
        g = [1.0] + [(0.8, 1.35, 1.0, 1.2)[j % 4] for j in range(k)]
        _made[key] = [cs.make(r, k, 12, 16, match=MATCH, channels=channels, masks=masks, noise_px=0.6, gains=g) for r in (5, 21)]
    return _made[key]


def dense_points(twin, scenes, match=MATCH):
    batch = hb.PreparedBatch([s.inputs for s in scenes], match, match)
    return batch, twin.triangulate_dense(batch, cs.params())


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def reference_table(scenes, res, k, match=MATCH):
    return gain_ref.batch_reference(cs.cameras(), [s.inputs for s in scenes], [s.images for s in scenes], match, match, res, TAU, k)


@pytest.mark.parametrize("k,channels,masks", [(3, 2, False), (3, 4, True), (16, 2, True), (16, 4, False)])
def test_twin_equals_the_reference_element_for_element(twin, k, channels, masks):
    scenes = case(k, channels, masks)
    batch, res = dense_points(twin, scenes)
    assert res.count > 300
    before = [cs.bits(getattr(res, n)).copy() for n in ("xyz", "rgb", "err", "cell", "slot")]
    table = twin.gain_accumulate(batch, res, TAU)
    want, part, counted = reference_table(scenes, res, k)
    assert table.dtype == torch.int64 and tuple(table.shape) == (2 * k, 7)
    assert np.array_equal(u64(table), want)
    assert counted.any() and (part & ~counted).any() and (~part).any()          # samples that count, samples out of range, views that do not confirm
    assert (want[:, 0] > 0).sum() >= k                                          # rows of both references
    for n, b in zip(("xyz", "rgb", "err", "cell", "slot"), before):             # reads only
        assert np.array_equal(cs.bits(getattr(res, n)), b)
    # the views are the multi-view colour's: reference + the slots that took part
    _out, status = twin.colour_multiview(batch, res, TAU, "mean", with_status=True)
    assert np.array_equal(status.numpy(), 1 + part.sum(axis=1))
    # a second call adds exactly the same again
    again = twin.gain_accumulate(batch, res, TAU, table=table)
    assert again is table and np.array_equal(u64(table), 2 * want)


def test_buffers_and_collected_result_give_the_same_table(twin):
    import ctypes as C
    scenes = case(3, 2, False)
    batch = hb.PreparedBatch([s.inputs for s in scenes], MATCH, MATCH)
    src = hb.OutputBuffers(2 * 12 * 16, 2, 3, torch.device("cpu"))
    assert twin._lib.lfd_triangulate_dense_host(twin._ctx, C.byref(batch.c), C.byref(cs.params()), C.byref(src.c), src.ref_offsets.data_ptr(),
                                                src.seg_counts.data_ptr()) == 0
    a = twin.gain_accumulate(batch, src, TAU)
    b = twin.gain_accumulate(batch, src.collect(), TAU)
    assert np.array_equal(u64(a), u64(b)) and int(a[:, 0].sum()) > 0


def test_guarded_points_have_no_samples(twin):
    scenes = case(3, 2, False)
    batch, res = dense_points(twin, scenes)
    n0 = int(res.ref_offsets[1])
    xyz, rgb, cell, slot = res.xyz.clone(), res.rgb.clone(), res.cell.clone(), res.slot.clone()
    xyz[3, 1] = float("nan")
    xyz[4, 0] = float("inf")
    rgb.view(torch.int32)[5, 2] = 0x7fc01234
    rgb[6, 0] = float("-inf")
    cell[7] = -1
    cell[8] = 12 * 16
    cell[n0 + 1] = 2 ** 31 - 1
    slot[9] = 3                                                              # n_slots of every reference is 3
    slot[n0 + 2] = 255
    rgb[10, 1] = 0.04                                                        # not guarded: the reference's colour is out of range
    rgb[11, 0] = 0.96
    hurt = dataclasses.replace(res, xyz=xyz, rgb=rgb, cell=cell, slot=slot, _packed=None)
    table = twin.gain_accumulate(batch, hurt, TAU)
    want, part, counted = reference_table(scenes, hurt, 3)
    assert np.array_equal(u64(table), want)
    bad = [3, 4, 5, 6, 7, 8, 9, n0 + 1, n0 + 2]
    assert not part[bad].any() and part[[10, 11]].any() and not counted[[10, 11]].any()
    clean = twin.gain_accumulate(batch, res, TAU)
    assert int(clean[:, 0].sum()) > int(table[:, 0].sum())


def test_apply_bits_equal_the_rule(twin):
    rng = np.random.default_rng(3)
    counts = np.array([5, 0, 700, 1, 4500], np.int64)                        # an empty reference, one of a single point, more than a chunk
    n = int(counts.sum())
    rgb = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
    rgb[2, 1] = np.float32(0.9)                                              # 0.9 x 1.5 clamps
    rgb[7] = [np.nan, np.inf, -np.inf]
    rgb.view(np.uint32)[8, 0] = 0x7fc01234                                   # a NaN with a payload: copied bit for bit
    rgb[9, 2] = -0.25                                                        # (a negative value is multiplied like any other)
    factors = np.array([[1.5, 1.5, 1.5], [9.0, 9.0, 9.0], [0.8, 1.0, 1.25], [0.25, 4.0, 1.0], [1.0 / 3.0, 1.1, 0.97]], np.float32)
    out = twin.gain_apply(torch.from_numpy(rgb), counts, factors).numpy()
    want = gains.apply_rule(rgb, np.repeat(factors, counts, axis=0))
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    assert want[2, 1] == 1.0 and (want[:5] == 1.0).any() and out.view(np.uint32)[8, 0] == 0x7fc01234
    assert np.isnan(out[7, 0]) and out[7, 1] == np.inf and out[7, 2] == -np.inf
    # the rule itself, spelled out for one value: one f32 product, then the clamp
    assert out[5, 0] == np.float32(rgb[5, 0] * np.float32(0.8)) and out[5, 2] == min(np.float32(rgb[5, 2] * np.float32(1.25)), np.float32(1.0))


# ---- the solver -------------------------------------------------------------------------------------------------------------------------------
def rows_from(pairs, lam):
    """A table for (reference uid, neighbour uid, N) ``pairs`` under log-gains ``lam`` (uid -> scalar or (3,)): Sref = base exp(lam_a),
    Snbr = base exp(lam_b) per channel, rounded to integers - with base = 2^44 x (0.3, 0.5, 0.4) the rounding changes ln(B / A) by less
    than 2^-41, far inside the 1e-12 the tests ask for."""
    ref, nbr, tab = [], [], []
    for (a, b, n) in pairs:
        la, lb = np.broadcast_to(np.asarray(lam[a], np.float64), (3,)), np.broadcast_to(np.asarray(lam[b], np.float64), (3,))
        base = np.array([0.3, 0.5, 0.4]) * 2.0 ** 44
        ref.append(a)
        nbr.append(b)
        tab.append([n] + list(np.rint(base * np.exp(la)).astype(np.uint64)) + list(np.rint(base * np.exp(lb)).astype(np.uint64)))
    return gains.GainRows(np.array(ref, np.int64), np.array(nbr, np.int64), np.array(tab, np.uint64))


def test_solver_recovers_known_factors_over_a_connected_graph():
    rng = np.random.default_rng(0)
    uids = [10, 11, 12, 13, 14, 15]
    lam = {u: v for u, v in zip(uids, rng.uniform(-0.4, 0.4, len(uids)))}
    pairs = [(10, 11, 500), (11, 10, 64), (11, 12, 90000), (12, 13, 700), (13, 14, 64), (14, 15, 3000), (15, 10, 100), (12, 15, 4000)]
    sol = gains.solve_gains(rows_from(pairs, lam), uids, "luma")
    mean = np.mean([lam[u] for u in uids])
    for i, u in enumerate(uids):
        assert abs(sol.log_gain[i, 0] - (lam[u] - mean)) <= 1e-12 and (sol.log_gain[i] == sol.log_gain[i, 0]).all()
        assert sol.factors[i, 0] == np.float32(math.exp(-sol.log_gain[i, 0]))
    assert sol.n_components == 1 and sol.rows_ignored == 0 and not sol.clamped and abs(sol.log_gain[:, 0].sum()) <= 1e-12
    # per channel
    lam3 = {u: rng.uniform(-0.3, 0.3, 3) for u in uids}
    sol = gains.solve_gains(rows_from(pairs, lam3), uids, "rgb")
    mean3 = np.mean([lam3[u] for u in uids], axis=0)
    for i, u in enumerate(uids):
        assert np.abs(sol.log_gain[i] - (lam3[u] - mean3)).max() <= 1e-12


def test_solver_components_small_rows_and_isolated_images():
    uids = [1, 2, 3, 4, 5, 6, 7]
    lam = {1: 0.3, 2: -0.1, 3: 0.2, 4: 0.5, 5: 0.1, 6: 0.9, 7: -0.7}
    pairs = [(1, 2, 100), (2, 3, 200), (3, 1, 64),             # one component
             (4, 5, 1000),                                    # another
             (5, 6, 63), (1, 4, 1), (6, 7, 0)]                # ignored: fewer than 64 samples - 6 and 7 are in no usable row
    sol = gains.solve_gains(rows_from(pairs, lam), uids, "luma")
    lg = sol.log_gain[:, 0]
    assert sol.n_components == 2 and sol.rows_ignored == 3
    assert abs(lg[0] + lg[1] + lg[2]) <= 1e-12 and abs(lg[3] + lg[4]) <= 1e-12            # zero mean per component
    assert abs((lg[1] - lg[0]) - (lam[2] - lam[1])) <= 1e-12 and abs((lg[4] - lg[3]) - (lam[5] - lam[4])) <= 1e-12
    assert (sol.factors[5:] == 1.0).all() and (lg[5:] == 0.0).all()                      # images in no usable row get 1
    assert sol.pairs.tolist() == [2, 2, 2, 1, 1, 0, 0] and sol.samples.tolist() == [164, 300, 264, 1000, 1000, 0, 0]
    js = sol.to_json({u: f"im{u}.png" for u in uids})
    assert js["mode"] == "luma" and js["components"] == 2 and js["rows_ignored"] == 3 and js["images"][3]["name"] == "im4.png"
    assert gains.MIN_SAMPLES == 64 and gains.MAX_GAIN == 4.0


def test_solver_clamps_and_warns():
    said = []
    sol = gains.solve_gains(rows_from([(1, 2, 100)], {1: 0.0, 2: 4.0}), [1, 2], "luma", warn=said.append)
    assert sol.factors[:, 0].tolist() == [4.0, 0.25] and sorted(sol.clamped) == [1, 2] and len(said) == 2 and "clamped" in said[0]


# ---- what it is for ---------------------------------------------------------------------------------------------------------------------------
SOLVED_MEASURED = 0.00031       # the worst |ln(f_a / f_b) + ln(g_a / g_b)| measured on this scene
SOLVED_BOUND = 4.0 * SOLVED_MEASURED       # asserted: four times that - other seeds and shapes - and it must stay below 0.03


def test_effect():
    """Four cameras, each a reference with the other three as neighbours, exposures (1.15, 0.85, 1, 1), exact warps, 256^2 renderings.

    Row level, derived: a sample of a view with gain g differs from g a(X) by at most e, the per-sample bound of the multi-view colour's
    test (tests/test_multiview_colour_host.py::test_effect: e = g_max G d + 0.5 / 255 + 1e-5 from the scene's geometry; the truncation to
    2^-24 is inside the 1e-5).  Every value is at least m = 0.85 x 0.4, so a sum of samples of view b over a sum of samples of view a at the
    same points lies within a factor (1 + e / m) / (1 - e / m) of g_b / g_a.

    Solved level, measured: the worst |ln(f_a / f_b) + ln(g_a / g_b)| over the six pairs is SOLVED_MEASURED; asserted is
    four times that, which must stay below 0.03 - a tenth of ln(1.15 / 0.85).

    Cloud level: per reference the mean of colour / albedo over its points; without compensation two references differ by their gains,
    with it by no more than the asserted bound."""
    match, H, W = 256, 40, 48
    cam_ids, g = [11, 12, 13, 14], (1.15, 0.85, 1.0, 1.0)
    cams = cs.cameras()
    twin = hb.HostDensifier(2)
    twin.upload_cameras(cams)
    try:
        scenes = gain_scene.make_group(cam_ids, g, H, W, match)
        d = max(cs.pixel_footprint(cams[c], match) for c in cam_ids)
        e = max(g) * cs.ALBEDO_GRAD * d + 0.5 / 255 + 1e-5
        m = 0.85 * 0.4
        row_bound = math.log((1 + e / m) / (1 - e / m))
        ref_uid, nbr_uid, tables, results = [], [], [], []
        for sc in scenes:
            batch = hb.PreparedBatch([sc.inputs], match, match)
            res = twin.triangulate_dense(batch, cs.params())
            results.append(res)
            tables.append(u64(twin.gain_accumulate(batch, res, TAU)))
            ref_uid += [sc.ref] * 3
            nbr_uid += sc.nbrs
        rows = gains.GainRows(np.array(ref_uid, np.int64), np.array(nbr_uid, np.int64), np.concatenate(tables, axis=0))
        assert rows.table.shape == (12, 7) and (rows.table[:, 0] >= gains.MIN_SAMPLES).all(), rows.table[:, 0]
        gain_of = dict(zip(cam_ids, g))
        worst_row = 0.0
        for a, b, t in zip(rows.ref_uid, rows.nbr_uid, rows.table.astype(np.float64)):
            dev = abs(math.log(t[4:7].sum() / t[1:4].sum()) - math.log(gain_of[int(b)] / gain_of[int(a)]))
            worst_row = max(worst_row, dev)
            assert dev <= row_bound, (a, b, dev, row_bound)
        sol = gains.solve_gains(rows, cam_ids, "luma")
        f = {c: float(sol.factors[i, 0]) for i, c in enumerate(cam_ids)}
        worst = max(abs(math.log(f[a] / f[b]) + math.log(gain_of[a] / gain_of[b])) for a in cam_ids for b in cam_ids if a < b)
        print(f"e = {e:.4f} (d = {d:.4f}), row bound {row_bound:.4f}, worst row {worst_row:.5f}; samples per row {rows.table[:, 0].min()} .. "
              f"{rows.table[:, 0].max()}; solved: worst pair {worst:.5f}, asserted {SOLVED_BOUND:.5f}; factors {f}")
        assert SOLVED_BOUND < 0.03 and SOLVED_BOUND < 0.1 * math.log(1.15 / 0.85) + 1e-3
        assert worst <= SOLVED_BOUND
        assert sol.n_components == 1 and not sol.clamped and sol.rows_ignored == 0
        # per channel the same exposures come out (the scene has no colour cast)
        sol3 = gains.solve_gains(rows, cam_ids, "rgb")
        for ch in range(3):
            f3 = {c: float(sol3.factors[i, ch]) for i, c in enumerate(cam_ids)}
            assert max(abs(math.log(f3[a] / f3[b]) + math.log(gain_of[a] / gain_of[b])) for a in cam_ids for b in cam_ids if a < b) <= row_bound
        # cloud level
        off, on = {}, {}
        for sc, res in zip(scenes, results):
            truth = sc.truth.reshape(-1, 3)[res.cell.numpy().astype(np.int64)]
            new = twin.gain_apply(res.rgb, [res.count], sol.factors[cam_ids.index(sc.ref)][None, :]).numpy()
            assert np.array_equal(new.view(np.uint32), gains.apply_rule(res.rgb.numpy(), sol.factors[cam_ids.index(sc.ref)]).view(np.uint32))
            off[sc.ref] = float((res.rgb.numpy().astype(np.float64) / truth).mean())
            on[sc.ref] = float((new.astype(np.float64) / truth).mean())
        spread_on = max(abs(math.log(on[a] / on[b])) for a in cam_ids for b in cam_ids if a < b)
        print(f"cloud: colour / albedo per reference without {off}, with {on}: worst pair {spread_on:.5f}")
        for a in cam_ids:
            for b in cam_ids:
                if a < b:
                    assert abs(math.log(off[a] / off[b]) - math.log(gain_of[a] / gain_of[b])) <= row_bound
                    assert abs(math.log(on[a] / on[b])) <= SOLVED_BOUND
        assert abs(math.log(off[11] / off[12])) > 0.29
    finally:
        twin.close()
