"""Epipolar audit, the report: what the histograms of lfd_epipolar_audit say about the camera poses.

Pure Python on integers: a histogram row is [usable, degenerate, bin 0 .. bin 63], bin b < 63 a distance of [b / 8, (b + 1) / 8) px of the
neighbour's camera image between a confident match and its epipolar line, bin 63 anything from 7.875 px on.  Quantiles are bin edges, found
by rank, so a device run and a host run - which agree on every integer - write the same report.

    pair      n, degenerate, median_px, p90_px (the upper edge of the bin the rank falls in; bin 63: None and ">= 7.875"), share_below_1px;
              USABLE with n >= audit_min_samples
    camera    its usable pairs, as reference or as neighbour ((a, b) and (b, a) are two rows); score = the LOWER median of their medians;
              SUSPECT iff it has at least two usable pairs and its score exceeds audit_warn_px.  A camera with a bad pose has all its pairs
              bad; a good camera with one bad neighbour keeps most of its pairs good.
    scene     the lower median of all usable pair medians, the pairs ignored, the suspects
"""
from __future__ import annotations

import json
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

BINS = 64
QUANTITIES = 66
LAST = BINS - 1
LAST_TEXT = ">= 7.875"


def bin_px(b: int) -> Optional[float]:
    """The upper edge of bin ``b`` in px (exact in binary), None for the open last bin."""
    return None if b >= LAST else (b + 1) / 8.0


def bin_text(b: int) -> str:
    return LAST_TEXT if b >= LAST else f"{(b + 1) / 8.0:.3f}"


def quantile_bin(hist: Sequence[int], rank: int) -> int:
    """The smallest bin whose cumulative count reaches ``rank`` (1-based).  ``hist``: the 64 bins; rank <= sum(hist)."""
    acc = 0
    for b, c in enumerate(hist):
        acc += int(c)
        if acc >= rank:
            return b
    return LAST


def lower_median(bins: Sequence[int]) -> int:
    """The lower median of bin indices (bin 63 sorts last by being the largest)."""
    s = sorted(int(b) for b in bins)
    return s[(len(s) - 1) // 2]


def exceeds(b: int, warn_px: float) -> bool:
    """A quantile in bin ``b`` exceeds ``warn_px``: its upper edge does; the open last bin always does."""
    return b >= LAST or (b + 1) / 8.0 > warn_px


def pair_stats(row: Sequence[int], min_samples: int) -> dict:
    row = [int(v) for v in row]
    if len(row) != QUANTITIES:
        raise ValueError(f"an audit row has {QUANTITIES} entries")
    n, hist = row[0], row[2:]
    if sum(hist) != n:
        raise ValueError("an audit row's bins must sum to its usable count")
    out = {"n": n, "degenerate": row[1], "usable": n >= int(min_samples), "median_bin": None, "p90_bin": None, "median_px": None,
           "p90_px": None, "median_text": None, "p90_text": None, "share_below_1px": None, "histogram": hist}
    if n > 0:
        mb, pb = quantile_bin(hist, (n + 1) // 2), quantile_bin(hist, (9 * n + 9) // 10)
        out.update(median_bin=mb, p90_bin=pb, median_px=bin_px(mb), p90_px=bin_px(pb), median_text=bin_text(mb), p90_text=bin_text(pb),
                   share_below_1px=sum(hist[:8]) / n)
    return out


def build_report(rows: Mapping[Tuple[int, int], Sequence[int]], names: Optional[Mapping[int, str]] = None, audit_min_samples: int = 256,
                 audit_warn_px: float = 0.8, audit_certainty: float = 0.5) -> dict:
    """``rows``: {(reference uid, neighbour uid): the pair's 66 integers summed over the run}.  Returns the report as plain JSON-able data."""
    if not (audit_warn_px > 0):
        raise ValueError("audit_warn_px must be > 0")
    names = dict(names or {})
    name = lambda uid: names.get(uid, str(uid))
    pairs: List[dict] = []
    per_cam: Dict[int, List[int]] = {}
    cams = set()
    for (a, b) in sorted(rows):
        st = pair_stats(rows[(a, b)], audit_min_samples)
        pairs.append({"reference_uid": int(a), "reference": name(a), "neighbour_uid": int(b), "neighbour": name(b), **st})
        cams.update((int(a), int(b)))
        if st["usable"]:
            per_cam.setdefault(int(a), []).append(st["median_bin"])
            per_cam.setdefault(int(b), []).append(st["median_bin"])
    cameras = []
    for uid in sorted(cams):
        meds = per_cam.get(uid, [])
        score = lower_median(meds) if meds else None
        cameras.append({"uid": uid, "name": name(uid), "usable_pairs": len(meds), "score_bin": score,
                        "score_px": bin_px(score) if score is not None else None, "score_text": bin_text(score) if score is not None else None,
                        "suspect": len(meds) >= 2 and exceeds(score, audit_warn_px)})
    usable = [p["median_bin"] for p in pairs if p["usable"]]
    scene_bin = lower_median(usable) if usable else None
    suspects = [c["uid"] for c in cameras if c["suspect"]]
    return {"knobs": {"audit_certainty": float(audit_certainty), "audit_min_samples": int(audit_min_samples), "audit_warn_px": float(audit_warn_px)},
            "bin_px": 0.125, "pairs": pairs, "cameras": cameras,
            "scene": {"usable_pairs": len(usable), "median_bin": scene_bin, "median_px": bin_px(scene_bin) if scene_bin is not None else None,
                      "median_text": bin_text(scene_bin) if scene_bin is not None else None,
                      "pairs_ignored": [[p["reference_uid"], p["neighbour_uid"]] for p in pairs if not p["usable"]],
                      "suspects": suspects, "n_cameras": len(cameras), "poses_do_not_fit": 2 * len(suspects) > len(cameras)}}


def summary_line(report: dict) -> str:
    s = report["scene"]
    return (f"epipolar audit: {s['usable_pairs']} usable pairs ({len(s['pairs_ignored'])} ignored), median distance from the epipolar line "
            f"{s['median_text'] if s['median_text'] is not None else 'n/a'} px, {len(s['suspects'])} of {s['n_cameras']} cameras suspect")


def warnings(report: dict) -> List[str]:
    """One warning per suspect camera - or, when more than half of the cameras are suspect, ONE warning about the poses as a whole."""
    s = report["scene"]
    if not s["suspects"]:
        return []
    warn = report["knobs"]["audit_warn_px"]
    if s["poses_do_not_fit"]:
        return [f"epipolar audit: {len(s['suspects'])} of {s['n_cameras']} cameras are more than {warn:g} px off their epipolar lines: the poses as "
                "a whole do not fit the photographs (wrong image association, scale or convention?)"]
    by_uid = {c["uid"]: c for c in report["cameras"]}
    return [f"epipolar audit: camera {by_uid[u]['name']} (uid {u}) is suspect: the median over its {by_uid[u]['usable_pairs']} pairs is "
            f"{by_uid[u]['score_text']} px off the epipolar lines (audit_warn_px {warn:g}); its pose, intrinsics or distortion may be wrong"
            for u in s["suspects"]]


def to_json(report: dict) -> str:
    return json.dumps(report, indent=1, sort_keys=True) + "\n"


def from_json(text: str) -> dict:
    return json.loads(text)
