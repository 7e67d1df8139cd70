"""Per-image exposure gains solved from the run's statistics: the host half of experimental['gain_compensation'].

The input is the table lfd_gain_accumulate[_host] summed while each reference was resident - per (reference, neighbour slot) the number of
samples N and the integer sums of the reference's and the neighbour's colour at the same surface points - with the camera uid of every
row's reference and neighbour.  Both backends hand in identical integers, so both get identical factors; everything here is NumPy f64.

Model: image value = exposure x albedo.  A row's observation is m = ln(B / A), A the sum of the reference's channel means and B the
neighbour's ("luma": over the three channels; "rgb": per channel), an estimate of lambda_nbr - lambda_ref with lambda = ln(exposure).
Rows below MIN_SAMPLES are ignored (and counted).  The lambdas minimise sum N (lambda_b - lambda_a - m)^2 over the rows; of the solutions -
every connected component of the pair graph may be shifted freely - the minimum-norm one is taken (np.linalg.lstsq), which has zero mean per
component: no ridge, no shrinking of the ratios.  The factor of image c is RN_f32(exp(-lambda_c)), clamped to [1 / MAX_GAIN, MAX_GAIN];
an image in no usable row gets 1."""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional, Sequence

import numpy as np

MIN_SAMPLES = 64             # a row needs this many samples to take part in the solve
MAX_GAIN = 4.0               # factors are clamped to [1 / MAX_GAIN, MAX_GAIN]
GAIN_MODES = ("off", "luma", "rgb")


@dataclasses.dataclass
class GainRows:
    """The run's statistics: row i is the pair (ref_uid[i] -> nbr_uid[i]) with table[i] = (N, Sref r g b, Snbr r g b) as uint64."""
    ref_uid: np.ndarray
    nbr_uid: np.ndarray
    table: np.ndarray

    @staticmethod
    def empty() -> "GainRows":
        return GainRows(np.zeros((0,), np.int64), np.zeros((0,), np.int64), np.zeros((0, 7), np.uint64))

    @staticmethod
    def concat(parts: Sequence["GainRows"]) -> "GainRows":
        if not parts:
            return GainRows.empty()
        return GainRows(np.concatenate([p.ref_uid for p in parts]), np.concatenate([p.nbr_uid for p in parts]),
                        np.concatenate([p.table for p in parts], axis=0))


@dataclasses.dataclass
class GainSolution:
    mode: str
    uids: List[int]
    log_gain: np.ndarray         # (n_images, 3) f64: lambda per image and channel (luma: three equal columns)
    factors: np.ndarray          # (n_images, 3) f32: the compensation factors, clamped
    pairs: np.ndarray            # (n_images,) i64: usable rows the image takes part in
    samples: np.ndarray          # (n_images,) i64: their samples
    rows_ignored: int            # rows with N < MIN_SAMPLES (those without any sample included)
    n_components: int            # connected components of the graph of usable rows (images in no usable row are not counted)
    clamped: List[int]           # uids whose factor was clamped

    def factor_of(self) -> Dict[int, np.ndarray]:
        return {uid: self.factors[i] for i, uid in enumerate(self.uids)}

    def to_json(self, names: Optional[Dict[int, str]] = None) -> dict:
        images = []
        for i, uid in enumerate(self.uids):
            f = [float(v) for v in self.factors[i]]
            images.append({"name": (names or {}).get(uid, ""), "uid": int(uid), "factor": f[0] if self.mode == "luma" else f,
                           "pairs": int(self.pairs[i]), "samples": int(self.samples[i])})
        return {"mode": self.mode, "min_samples": MIN_SAMPLES, "max_gain": MAX_GAIN, "images": images, "rows_ignored": int(self.rows_ignored),
                "components": int(self.n_components), "clamped": [int(u) for u in self.clamped]}


def _components(n: int, a: np.ndarray, b: np.ndarray) -> int:
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for x, y in zip(a.tolist(), b.tolist()):
        parent[find(x)] = find(y)
    return len({find(x) for x in set(a.tolist()) | set(b.tolist())})


def solve_gains(rows: GainRows, uids: Sequence[int], mode: str, warn=None) -> GainSolution:
    """The factors of the images ``uids`` (every uid a row names must be among them) from the run's ``rows``; ``mode``: "luma" or "rgb".
    ``warn``: called with a message for every clamped image."""
    if mode not in ("luma", "rgb"):
        raise ValueError("solve_gains: mode must be 'luma' or 'rgb'")
    uids = [int(u) for u in uids]
    index = {u: i for i, u in enumerate(uids)}
    if len(index) != len(uids):
        raise ValueError("solve_gains: the image uids must be distinct")
    n = len(uids)
    table = np.asarray(rows.table, np.uint64).reshape(-1, 7)
    N = table[:, 0].astype(np.int64)
    use = N >= MIN_SAMPLES
    a = np.array([index[int(u)] for u in np.asarray(rows.ref_uid)[use]], np.int64)
    b = np.array([index[int(u)] for u in np.asarray(rows.nbr_uid)[use]], np.int64)
    w = N[use].astype(np.float64)
    sref, snbr = table[use, 1:4].astype(np.float64), table[use, 4:7].astype(np.float64)
    lam = np.zeros((n, 3), np.float64)
    m_rows = int(use.sum())
    if m_rows:
        D = np.zeros((m_rows, n), np.float64)
        D[np.arange(m_rows), b] += 1.0
        D[np.arange(m_rows), a] -= 1.0               # (a pair of an image with itself: a zero row, no information)
        sw = np.sqrt(w)
        if mode == "luma":
            m = np.log(snbr.sum(axis=1) / sref.sum(axis=1))
            lam[:] = np.linalg.lstsq(D * sw[:, None], m * sw, rcond=None)[0][:, None]
        else:
            m = np.log(snbr / sref)
            lam[:] = np.linalg.lstsq(D * sw[:, None], m * sw[:, None], rcond=None)[0]
    raw = np.exp(-lam).astype(np.float32)
    lo, hi = np.float32(1.0 / MAX_GAIN), np.float32(MAX_GAIN)
    factors = np.minimum(np.maximum(raw, lo), hi)
    clamped = [uids[i] for i in range(n) if (factors[i] != raw[i]).any()]
    for u in clamped:
        if warn is not None:
            i = index[u]
            warn(f"gain compensation: the factor of image uid {u} ({', '.join(f'{v:.4g}' for v in raw[i])}) was clamped to "
                 f"[{1.0 / MAX_GAIN:g}, {MAX_GAIN:g}]")
    pairs, samples = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for x in (a, b):
        np.add.at(pairs, x, 1)
        np.add.at(samples, x, N[use])
    return GainSolution(mode=mode, uids=uids, log_gain=lam, factors=factors, pairs=pairs, samples=samples,
                        rows_ignored=int((~use).sum()), n_components=_components(n, a, b) if m_rows else 0, clamped=clamped)


def apply_rule(rgb: np.ndarray, f: np.ndarray) -> np.ndarray:
    """lfd_gain_apply's rule in NumPy: min(c * f, 1) in f32, one rounding; a value that is not finite keeps its bits.  rgb (n, 3) f32, f (n, 3)
    or (3,) f32."""
    rgb = np.ascontiguousarray(rgb, np.float32)
    with np.errstate(all="ignore"):
        out = np.minimum(rgb * np.asarray(f, np.float32), np.float32(1.0)).astype(np.float32)
    bad = ~np.isfinite(rgb)
    out.view(np.uint32)[bad] = rgb.view(np.uint32)[bad]
    return out


__all__ = ["MIN_SAMPLES", "MAX_GAIN", "GAIN_MODES", "GainRows", "GainSolution", "solve_gains", "apply_rule"]
