"""CPU tier of the connected-component filter (lfd_component_filter_host): the twin - keys, sort, the walk over the cells below a
point and a sequential union-find through csrc/lfd_component.hpp - against the brute-force reference of tests/component_ref.py, which knows
neither grid nor sort.  Every comparison is exact: size and label of every point, the kept rows bit for bit, the offsets and the summary."""
import numpy as np
import pytest
import torch

import component_cases as cases
import component_ref as cr
import consensus_ref
from lichtfeld_densification_plugin_amd.core import hip_backend as hb


@pytest.fixture(scope="module")
def twin():
    t = hb.HostDensifier(4)
    yield t
    t.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def call(dens, xyz, counts, radius, min_points, with_sizes=True, with_labels=True, rgb=None, err=None):
    """component_filter over NumPy arrays (moved to the densifier's device and back): (xyz, rgb, err, kept, size u32, label u32, summary)"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dens.device) if a is not None else None      # noqa: E731
    back = lambda v: v.cpu().numpy() if v is not None else None      # noqa: E731
    x, c, e, kept, size, label, summ = dens.component_filter(t(xyz), t(rgb), t(err), counts, radius, min_points, with_sizes, with_labels)
    u32 = lambda v: back(v).view(np.uint32) if v is not None else None      # noqa: E731
    return back(x), back(c), back(e), np.asarray(kept), u32(size), u32(label), np.asarray(summ)


def check_against_reference(twin, xyz, counts, radius, min_points_list, want=None):
    """the twin against component_ref on every output, at every min_points; returns (size, label) of the reference"""
    xyz = np.ascontiguousarray(xyz, np.float32)
    n = xyz.shape[0]
    rng = np.random.default_rng(n + 29)
    rgb = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
    err = rng.uniform(0.0, 2.0, (n,)).astype(np.float32)
    if n > 2:
        rgb[1, 1], err[2] = np.nan, np.inf                                 # whatever travels along is copied, not looked at
    with np.errstate(all="ignore"):
        size_ref, label_ref = cr.components(xyz, radius) if want is None else want
    summ_ref = cr.summary(size_ref, label_ref)
    ids = cr.ref_ids(counts)
    for m in min_points_list:
        keep = size_ref >= m
        x, c, e, kept, size, label, summ = call(twin, xyz, counts, radius, m, True, True, rgb, err)
        assert np.array_equal(size, size_ref), (m, np.flatnonzero(size != size_ref)[:10])
        assert np.array_equal(label, label_ref), (m, np.flatnonzero(label != label_ref)[:10])
        assert np.array_equal(summ, summ_ref)
        assert np.array_equal(kept, np.bincount(ids[keep], minlength=len(counts)))
        assert np.array_equal(bits(x), bits(xyz[keep])) and np.array_equal(bits(c), bits(rgb[keep])) and np.array_equal(bits(e), bits(err[keep]))
        # without the optional outputs: the same kept set, nothing else written
        x2, c2, e2, kept2, size2, label2, summ2 = call(twin, xyz, counts, radius, m, False, False)
        assert size2 is None and label2 is None and c2 is None and e2 is None
        assert np.array_equal(bits(x2), bits(xyz[keep])) and np.array_equal(kept2, kept) and np.array_equal(summ2, summ_ref)
    return size_ref, label_ref


def test_the_summary_words_of_a_cloud_counted_by_hand(twin):
    # components of 3, 1, 2 and 1 points along a line, written down by hand: neither the reference nor the twin is asked what they should be
    xyz = np.zeros((7, 3), np.float32)
    xyz[:, 0] = [0.0, 0.1, 0.2, 10.0, 20.0, 20.1, 30.0]
    want = np.zeros(66, np.int64)
    want[0], want[1] = 4, 3                                                # four components, the largest of three points
    want[2], want[3] = 2, 2                                                # two of size 1; two with 2 <= size < 4
    want[34], want[35] = 2, 5                                              # ... holding 2 and 5 points
    size, label = np.array([3, 3, 3, 1, 2, 2, 1], np.uint32), np.array([0, 0, 0, 3, 4, 4, 6], np.uint32)
    assert np.array_equal(cr.summary(size, label), want)
    x, _c, _e, kept, size_t, label_t, summ_t = call(twin, xyz, [4, 3], 0.15, 2)
    assert np.array_equal(size_t, size) and np.array_equal(label_t, label) and np.array_equal(summ_t, want)
    assert kept.tolist() == [3, 2] and np.array_equal(bits(x), bits(xyz[size >= 2]))
    check_against_reference(twin, xyz, [4, 3], 0.15, [2, 3, 4])


@pytest.mark.parametrize("gap_at", [None, 1237])
def test_a_long_chain_is_one_component_and_one_gap_makes_two(twin, gap_at):
    line, radius = cases.chain(2000, gap_at)
    rng = np.random.default_rng(3)
    perm = rng.permutation(2000)
    xyz = line[perm]
    sizes = [2000] if gap_at is None else [gap_at, 2000 - gap_at]
    # min_points exactly at, one above and one below a component's size
    mins = sorted({max(2, s + d) for s in sizes for d in (-1, 0, 1)})
    size, label = check_against_reference(twin, xyz, [700, 0, 1300], radius, mins)
    want = np.full(2000, 2000) if gap_at is None else np.where(perm < gap_at, gap_at, 2000 - gap_at)
    assert np.array_equal(size, want)
    assert len(set(label.tolist())) == len(sizes)
    for m in mins:
        kept = call(twin, xyz, [2000], radius, m)[3]
        assert int(kept[0]) == sum(s for s in sizes if s >= m)
    # in line order too: the sorted positions then follow the input, and the trees are the deepest
    check_against_reference(twin, line, [2000], radius, [2])


def test_the_boundary_of_the_link_test_is_the_f32_expression(twin):
    radius = 0.5
    just_over = np.nextafter(np.float32(0.5), np.float32(1.0))
    on = np.array([[0, 0, 0], [0.5, 0, 0]], np.float32)
    over = np.array([[0, 0, 0], [just_over, 0, 0]], np.float32)
    assert cr.edges(on, radius).tolist() == [[0, 1]] and cr.edges(over, radius).tolist() == []      # the reference's own f32 expression decides
    assert check_against_reference(twin, on, [2], radius, [2, 3])[0].tolist() == [2, 2]
    assert check_against_reference(twin, over, [1, 1], radius, [2])[0].tolist() == [1, 1]
    # 3-4-5: d2 = 25 exactly
    tri = np.array([[0, 0, 0], [3, 4, 0], [3, 4, 12]], np.float32)
    assert check_against_reference(twin, tri, [3], 5.0, [2])[0].tolist() == [2, 2, 1]
    assert check_against_reference(twin, tri, [3], 12.0, [2])[0].tolist() == [3, 3, 3]


def test_pairs_across_a_cell_border_in_each_of_the_26_directions(twin):
    radius = 1.0
    n = 0
    for d in np.stack(np.meshgrid([-1, 0, 1], [-1, 0, 1], [-1, 0, 1], indexing="ij"), -1).reshape(-1, 3):
        if not d.any():
            continue
        base = np.array([10.3, -4.2, 0.9])
        b = base + d * 0.55 / np.linalg.norm(d) * radius
        anchor = base - 3.0                                                # fixes the grid's origin; far from both
        for off in np.linspace(0.0, 1.0, 7):                               # slide the pair through the cells: it straddles a face for some offsets
            xyz = np.array([anchor, base + off * d, b + off * d], np.float32)
            for order in ([0, 1, 2], [2, 1, 0]):                           # whichever of the two sorts first
                size, label = check_against_reference(twin, xyz[order], [1, 2], radius, [2])
                assert sorted(size.tolist()) == [1, 2, 2], (d, off)
            n += 1
    assert n == 26 * 7


def test_two_points_of_one_cell_further_apart_than_the_radius_stay_separate(twin):
    radius = 1.0
    xyz = np.array([[0, 0, 0], [0.9, 0.9, 0.9], [0.05, 0, 0], [0.9, 0.9, 0.95]], np.float32)      # one cell; its diagonal is 1.56 radius
    size, label = check_against_reference(twin, xyz, [4], radius, [2, 3])
    assert size.tolist() == [2, 2, 2, 2] and label.tolist() == [0, 1, 0, 1]


def test_the_lattice_with_singletons_and_clumps(twin):
    xyz, counts, radius, want = cases.lattice_with_clumps()
    assert xyz.shape[0] == 4096 + 200 + 820
    size, label = check_against_reference(twin, xyz, counts, radius, [2, 20, 40, 41, 4096, 4097])
    assert np.array_equal(size, want)                                      # the construction, the reference and the twin agree
    summ = cr.summary(size, label)
    assert summ[0] == 1 + 200 + 40 and summ[1] == 4096 and summ[2] == 201 and summ[2 + 12] == 1 and summ[34 + 12] == 4096


def test_three_hundred_identical_points(twin):
    xyz = np.tile(np.array([[1.5, -2.0, 0.25]], np.float32), (300, 1))
    size, label = check_against_reference(twin, xyz, [100, 200], 1e-3, [2, 300, 301])
    assert (size == 300).all() and (label == 0).all()


def test_five_thousand_points_in_one_cell(twin):
    xyz, counts, radius = cases.one_cell(5000)
    size, label = check_against_reference(twin, xyz, counts, radius, [2, 2500, 2501])
    assert (size == 2500).all() and len(set(label.tolist())) == 2


@pytest.mark.parametrize("radius", [1e-4, 0.004, 0.01, 0.05, 20.0])           # from "all singletons" to "one component"
def test_seeded_clustered_cloud_equals_the_reference(twin, radius):
    xyz, counts = cases.clustered(3000, 5, 4)
    size, _label = check_against_reference(twin, xyz, counts, radius, [2, 5, 100])
    if radius == 1e-4:
        assert (size == 1).all()
    if radius == 20.0:
        assert (size == 3000).all()


def test_degenerate_inputs(twin):
    z3, z1 = np.zeros((0, 3), np.float32), np.zeros((0,), np.float32)
    x, c, e, kept, size, label, summ = call(twin, z3, [0, 0, 0], 1.0, 2, True, True, z3, z1)
    assert x.shape == (0, 3) and c.shape == (0, 3) and e.shape == (0,) and kept.tolist() == [0, 0, 0] and size.shape == (0,) and not summ.any()
    x, _c, _e, kept, size, label, summ = call(twin, np.ones((1, 3), np.float32), [0, 1], 1.0, 2)
    assert x.shape[0] == 0 and kept.tolist() == [0, 0] and size.tolist() == [1] and label.tolist() == [0]
    assert summ[:3].tolist() == [1, 1, 1] and summ[34] == 1 and summ.sum() == 4
    # empty references at the start, in the middle and at the end; one reference
    xyz, _ = cases.clustered(900, 2, 6)
    a = check_against_reference(twin, xyz, [0, 0, 300, 0, 600, 0], 0.02, [2, 4])
    check_against_reference(twin, xyz, [900], 0.02, [2, 4], want=a)        # the references do not enter the partition
    assert 1 < a[0].max() < 900


def test_non_finite_points_are_singletons_and_change_nothing_else(twin):
    xyz, counts = cases.clustered(1200, 6, 9)
    rng = np.random.default_rng(9)
    bad = rng.choice(1200, 60, replace=False)
    dirty = xyz.copy()
    dirty[bad[:20], 0] = np.nan
    dirty[bad[20:40], 2] = np.inf
    dirty[bad[40:], 1] = -np.inf
    size, label = check_against_reference(twin, dirty, counts, 0.02, [2, 3])
    assert (size[bad] == 1).all() and np.array_equal(label[bad], bad)
    # against the same cloud with those points REMOVED: the others form the same components
    mask = np.ones(1200, bool)
    mask[bad] = False
    ids = cr.ref_ids(counts)
    removed = call(twin, dirty[mask], np.bincount(ids[mask], minlength=6), 0.02, 2)
    assert np.array_equal(removed[4], size[mask])
    assert np.array_equal(np.flatnonzero(mask)[removed[5]], label[mask])
    allbad = np.full((5, 3), np.nan, np.float32)
    allbad[3] = np.inf
    size, label = check_against_reference(twin, allbad, [2, 3], 1.0, [2])
    assert size.tolist() == [1] * 5 and label.tolist() == [0, 1, 2, 3, 4]


def test_a_permutation_of_the_input_gives_the_same_partition(twin):
    xyz, counts = cases.clustered(2500, 7, 12)
    rng = np.random.default_rng(12)
    perm = rng.permutation(2500)
    a = call(twin, xyz, counts, 0.015, 4)
    b = call(twin, xyz[perm], [2500], 0.015, 4)
    assert 1 < a[4].max() < 2500
    assert np.array_equal(b[4], a[4][perm])                                # the sizes are permuted
    # the labels are mapped through the permutation: two points share a label after it iff they did before, and a label is the smallest NEW index
    inv = np.empty(2500, np.int64)
    inv[perm] = np.arange(2500)
    want = np.full(2500, 2500, np.int64)
    np.minimum.at(want, a[5], inv)                                         # per old label: the smallest new index of its members
    assert np.array_equal(b[5], want[a[5][perm]])
    assert np.array_equal(b[6], a[6])


def sheets_and_clumps():
    """A sheet owned by ONE reference, a second sheet owned by three, and clumps of at most 30 points each further than the radius from
    everything - all on a lattice of dyadic coordinates, so every distance that matters is exact."""
    radius, step = 0.25, 0.125
    a = np.arange(24) * step
    uv = np.stack(np.meshgrid(a, a, indexing="ij"), -1).reshape(-1, 2)
    sheet1 = np.column_stack([uv, np.zeros(576)])                          # reference 0 alone
    sheet2 = np.column_stack([uv, np.full(576, 8.0)])                      # references 1, 2, 3 in turn
    parts, flags = {g: [] for g in range(5)}, {g: [] for g in range(5)}
    parts[0].append(sheet1), flags[0].append(np.zeros(576, bool))
    for g in (1, 2, 3):
        parts[g].append(sheet2[g - 1::3]), flags[g].append(np.zeros(sheet2[g - 1::3].shape[0], bool))
    rng = np.random.default_rng(41)
    for k in range(12):                                                    # clumps of 5 .. 30 points on a fine lattice inside a cube of side 0.125
        m = 5 + (25 * k) // 11
        cells = rng.choice(5 ** 3, m, replace=False)
        pts = np.stack([cells // 25, (cells // 5) % 5, cells % 5], 1) * (step / 4.0) + np.array([k * 1.0, -2.0, 4.0])
        owner = k % 5
        parts[owner].append(pts), flags[owner].append(np.ones(m, bool))
    xyz = np.concatenate([np.concatenate(parts[g]) for g in range(5)]).astype(np.float32)
    counts = np.array([sum(p.shape[0] for p in parts[g]) for g in range(5)], np.int64)
    return xyz, counts, np.concatenate([np.concatenate(flags[g]) for g in range(5)]), radius


def test_it_keeps_the_one_witness_sheet_that_the_consensus_filter_erases(twin):
    xyz, counts, clump, radius = sheets_and_clumps()
    keep, size, label, kept, summ = cr.filter_cloud(xyz, counts, radius, 31)
    assert size[clump].max() == 30 and size[clump].min() == 5 and (size[~clump] == 576).all()
    x, _c, _e, kept_t, size_t, _l, summ_t = call(twin, xyz, counts, radius, 31)
    assert np.array_equal(size_t, size) and np.array_equal(summ_t, summ) and np.array_equal(kept_t, kept)
    assert np.array_equal(bits(x), bits(xyz[~clump]))                      # every clump point goes, every sheet point stays
    # the consensus filter at min_refs = 1 and the same radius drops the whole one-reference sheet (and keeps the three-reference one)
    t = torch.from_numpy
    xc, _rc, _ec, kept_c, _cons = twin.consensus_filter(t(xyz), None, None, counts, radius, 1)
    ids = consensus_ref.ref_ids(counts)
    on_sheet1 = (~clump) & (ids == 0)
    assert on_sheet1.sum() == 576
    assert np.array_equal(bits(xc.numpy()), bits(xyz[(~clump) & (ids != 0)]))
