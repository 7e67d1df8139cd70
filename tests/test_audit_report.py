"""The epipolar audit's report (core/audit.py) on hand-made histograms: the rank rule of the quantiles, the open last bin, the
sample floor, the lower median of a camera's pairs, the two-pair floor of the verdict, the majority warning, the JSON round trip."""
import pytest

from lichtfeld_densification_plugin_amd.core import audit


def row(bins, degenerate=0):
    """{bin: count} -> the pair's 66 integers."""
    h = [0] * 64
    for b, c in bins.items():
        h[b] = c
    return [sum(h), degenerate] + h


@pytest.mark.parametrize("n,samples,median_bin,p90_bin", [
    (1, [5], 5, 5),                                          # ranks 1 and 1
    (2, [3, 9], 3, 9),                                       # ranks 1 (the lower of two) and 2
    (3, [2, 4, 6], 4, 6),                                    # ranks 2 and 3
    (10, [0, 1, 2, 3, 4, 5, 6, 7, 8, 40], 4, 8),             # ranks 5 and (90 + 9) // 10 = 9
])
def test_the_rank_rule(n, samples, median_bin, p90_bin):
    bins = {}
    for s in samples:
        bins[s] = bins.get(s, 0) + 1
    st = audit.pair_stats(row(bins), 1)
    assert st["n"] == n and st["usable"] and st["median_bin"] == median_bin and st["p90_bin"] == p90_bin
    assert st["median_px"] == (median_bin + 1) / 8.0 and st["p90_px"] == (p90_bin + 1) / 8.0
    assert st["median_text"] == f"{(median_bin + 1) / 8.0:.3f}"
    assert st["share_below_1px"] == sum(1 for s in samples if s < 8) / n


def test_everything_in_the_last_bin_and_an_empty_row():
    st = audit.pair_stats(row({63: 500}, degenerate=3), 256)
    assert st["usable"] and st["median_bin"] == 63 and st["median_px"] is None and st["p90_px"] is None
    assert st["median_text"] == ">= 7.875" == st["p90_text"] and st["share_below_1px"] == 0.0 and st["degenerate"] == 3
    empty = audit.pair_stats(row({}), 1)
    assert empty["n"] == 0 and not empty["usable"] and empty["median_bin"] is None and empty["share_below_1px"] is None
    with pytest.raises(ValueError, match="66 entries"):
        audit.pair_stats([0] * 65, 1)
    with pytest.raises(ValueError, match="sum to its usable count"):
        audit.pair_stats([5, 0] + [0] * 64, 1)
    # a camera all of whose pairs sit in the last bin is suspect whatever the threshold; bin 63 sorts last
    rep = audit.build_report({(1, 2): row({63: 300}), (2, 1): row({63: 300}), (1, 3): row({0: 300}), (3, 1): row({0: 300}), (3, 4): row({0: 300})},
                             None, 256, 100.0)
    assert rep["scene"]["suspects"] == [2] and [c["score_text"] for c in rep["cameras"]] == ["0.125", ">= 7.875", "0.125", "0.125"]
    assert audit.lower_median([63, 0, 63, 0]) == 0 and audit.lower_median([63, 0, 63]) == 63


def test_the_sample_floor():
    rows = {(1, 2): row({0: 255}), (2, 1): row({0: 256}), (1, 3): row({40: 10})}
    rep = audit.build_report(rows, {1: "a.png", 2: "b.png"}, 256, 0.8)
    assert [p["usable"] for p in rep["pairs"]] == [False, False, True]            # sorted by (reference, neighbour): (1, 2), (1, 3), (2, 1)
    assert rep["scene"]["pairs_ignored"] == [[1, 2], [1, 3]] and rep["scene"]["usable_pairs"] == 1
    assert [c["usable_pairs"] for c in rep["cameras"]] == [1, 1, 0] and rep["scene"]["suspects"] == []
    assert [c["name"] for c in rep["cameras"]] == ["a.png", "b.png", "3"]
    assert audit.build_report(rows, None, 1, 0.8)["scene"]["usable_pairs"] == 3
    with pytest.raises(ValueError, match="audit_warn_px must be > 0"):
        audit.build_report(rows, None, 1, 0.0)


def test_the_lower_median_and_the_two_pair_floor():
    good, bad = row({0: 400}), row({17: 400})                                         # 0.125 px and 2.25 px
    # camera 1: four usable pairs, two bad - the LOWER median of [0, 0, 17, 17] is 0: not suspect.  Camera 2: both of its pairs bad: suspect.
    rows = {(1, 2): bad, (2, 1): bad, (1, 3): good, (3, 1): good}
    rep = audit.build_report(rows, None, 256, 0.8)
    by = {c["uid"]: c for c in rep["cameras"]}
    assert by[1]["usable_pairs"] == 4 and by[1]["score_px"] == 0.125 and not by[1]["suspect"]
    assert by[2]["usable_pairs"] == 2 and by[2]["score_px"] == 2.25 and by[2]["suspect"]
    assert not by[3]["suspect"] and rep["scene"]["suspects"] == [2] and rep["scene"]["median_px"] == 0.125
    # a score exactly at the threshold does not exceed it
    assert audit.build_report(rows, None, 256, 2.25)["scene"]["suspects"] == []
    # a camera with a single usable pair is never suspect, however bad the pair
    one = audit.build_report({(1, 2): bad, (1, 3): good, (3, 1): good, (3, 4): good, (4, 3): good}, None, 256, 0.8)
    by = {c["uid"]: c for c in one["cameras"]}
    assert by[2]["usable_pairs"] == 1 and by[2]["score_px"] == 2.25 and not by[2]["suspect"] and one["scene"]["suspects"] == []
    assert audit.warnings(one) == []


def test_the_warnings():
    good, bad = row({0: 400}), row({30: 400})
    rows = {(1, 2): bad, (2, 1): bad, (1, 3): good, (3, 1): good, (3, 4): good, (4, 3): good}
    rep = audit.build_report(rows, {2: "IMG_2.jpg"}, 256, 0.8)
    w = audit.warnings(rep)
    assert len(w) == 1 and "IMG_2.jpg" in w[0] and "uid 2" in w[0] and "3.875" in w[0] and not rep["scene"]["poses_do_not_fit"]
    assert "1 of 4 cameras suspect" in audit.summary_line(rep) and "6 usable pairs (0 ignored)" in audit.summary_line(rep)
    # more than half of the cameras: ONE warning about the poses as a whole, none per camera
    allbad = audit.build_report({k: bad for k in rows}, None, 256, 0.8)
    assert allbad["scene"]["suspects"] == [1, 2, 3, 4] and allbad["scene"]["poses_do_not_fit"]
    w = audit.warnings(allbad)
    assert len(w) == 1 and "as a whole do not fit the photographs" in w[0] and "4 of 4" in w[0]
    # exactly half is not a majority
    half = audit.build_report({(1, 2): bad, (2, 1): bad, (3, 4): good, (4, 3): good}, None, 256, 0.8)
    assert half["scene"]["suspects"] == [1, 2] and not half["scene"]["poses_do_not_fit"] and len(audit.warnings(half)) == 2


def test_the_json_round_trip():
    rows = {(1, 2): row({0: 300, 5: 10}, degenerate=2), (2, 1): row({63: 300})}
    rep = audit.build_report(rows, {1: "a.png", 2: "b.png"}, 256, 0.8, 0.5)
    text = audit.to_json(rep)
    assert audit.from_json(text) == rep and audit.to_json(audit.from_json(text)) == text
    assert rep["knobs"] == {"audit_certainty": 0.5, "audit_min_samples": 256, "audit_warn_px": 0.8}
    assert rep["pairs"][0]["histogram"][:6] == [300, 0, 0, 0, 0, 10] and rep["pairs"][1]["median_px"] is None
    assert "elapsed" not in text and "seconds" not in text
