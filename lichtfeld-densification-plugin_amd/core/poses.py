"""Pose corrections from the matches, the solve: one Gauss-Newton step on the epipolar error from the integer tables of
lfd_pose_accumulate.

NumPy f64 on integers that a device run and a host run agree on, no timing fields: both write the same report.  A row is [inliers, outliers,
degenerate, sum rq rq, sum Jq_i rq (6), sum Jq_i Jq_j (i <= j, 21), unused] with Jq = rint(8 J), rq = rint(1024 r): r the signed distance of a
match from its epipolar line in px of the neighbour's camera image, J its derivative with respect to a LEFT twist (omega, tau / tn) of the
pair's relative pose T_B T_A^-1, taken at the foot of the observation on the line.

    pair      USABLE with inliers >= pose_min_samples.  H = sums / 64, g = sums / 8192; the translation rows and columns times 1 / tn; expanded
              to the two cameras' left twists by delta_rel = delta_B - Ad(R, t) delta_A, Ad(omega, tau) = (R omega, [t]x R omega + R tau)
    gauge     the epipolar error does not see a rotation, a translation or a scaling of the world: seven directions, written down analytically
              per camera (R_i, t_i) - omega = -R_i e_a, tau = -omega x t_i; tau = -R_i e_a; tau = t_i - and the system is solved in their
              orthogonal complement.  Eigen-directions of the reduced matrix below EIG_CUT (a design default) of its largest eigenvalue are
              dropped and counted.
    camera    R_i <- exp([omega_i]x) R_i,  t_i <- exp([omega_i]x) t_i + tau_i.  A camera without a usable pair is left out, unchanged.

One LINEAR step: a step above WARN_STEP_DEG (a design default) is reported with a warning that it cannot be trusted.
"""
from __future__ import annotations

import dataclasses
import json
from typing import List, Mapping, Optional, Sequence, Tuple

import numpy as np

from . import colmap_io
from .types import CameraRecord

QUANTITIES = 32
# Relative eigenvalue below which a direction of the reduced matrix counts as undetermined.  A design default, and it has to sit ABOVE the floor
# the quantisation itself leaves: Jq = rint(8 J) is off by 1 / 8 / sqrt(12) px per radian on entries of a few hundred, so a direction the
# matches do not determine at all (two groups of cameras joined by a single pair: their relative scale) comes out of the integer sums at
# about (0.036 / 300)^2 ~ 1e-8 .. 1e-7 of the largest eigenvalue, not at 0 (measured: 5.4e-8).  A cut of 1e-9 keeps that direction and the
# step along it is noise times 1e7.  On a well-posed rig the smallest real eigenvalue is about 1e-5 (tests/pose_scene.py: 9.6e-6).
EIG_CUT = 1e-6
WARN_STEP_DEG = 2.0
F32_POSE_TOL = 1e-5        # apply_corrections: |difference| a pose may show against the file's input_* (f32 rounding of entries of size O(1) .. O(10))


def skew(v) -> np.ndarray:
    x, y, z = (float(a) for a in v)
    return np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])


def exp_so3(w) -> np.ndarray:
    """Rodrigues' formula."""
    w = np.asarray(w, np.float64).reshape(3)
    th = float(np.linalg.norm(w))
    K = skew(w)
    if th < 1e-12:
        return np.eye(3) + K + 0.5 * (K @ K)
    return np.eye(3) + (np.sin(th) / th) * K + ((1.0 - np.cos(th)) / (th * th)) * (K @ K)


def pose_of(rec) -> Tuple[np.ndarray, np.ndarray]:
    """(R, t) of a record as the library holds them: the f32 values, in f64."""
    return (np.asarray(rec.R, np.float32).astype(np.float64).reshape(3, 3), np.asarray(rec.t, np.float32).astype(np.float64).reshape(3))


def relative(pa, pb) -> Tuple[np.ndarray, np.ndarray]:
    R = pb[0] @ pa[0].T
    return R, pb[1] - R @ pa[1]


def adjoint(R, t) -> np.ndarray:
    A = np.zeros((6, 6))
    A[:3, :3] = R
    A[3:, :3] = skew(t) @ R
    A[3:, 3:] = R
    return A


def pair_system(row: Sequence[int]) -> Tuple[np.ndarray, np.ndarray, float]:
    """(H (6, 6), g (6,), sum r^2) of one row, dequantised; the translation part still in units of tn."""
    row = [int(v) for v in row]
    if len(row) != QUANTITIES:
        raise ValueError(f"a pose row has {QUANTITIES} entries")
    H = np.zeros((6, 6))
    e = 10
    for i in range(6):
        for j in range(i, 6):
            H[i, j] = H[j, i] = row[e] / 64.0
            e += 1
    g = np.array([row[4 + i] / 8192.0 for i in range(6)])
    return H, g, row[3] / 1048576.0


def gauge_columns(poses: Sequence[Tuple[np.ndarray, np.ndarray]]) -> np.ndarray:
    """(6 N, 7): what a rotation about and a translation along each world axis and a scaling of the world do to every camera's left twist."""
    G = np.zeros((6 * len(poses), 7))
    for i, (R, t) in enumerate(poses):
        for a in range(3):
            om = -R[:, a]
            G[6 * i:6 * i + 3, a] = om
            G[6 * i + 3:6 * i + 6, a] = -np.cross(om, t)
            G[6 * i + 3:6 * i + 6, 3 + a] = -R[:, a]
        G[6 * i + 3:6 * i + 6, 6] = t
    return G


def assemble(rows: Mapping[Tuple[int, int], Sequence[int]], poses: Mapping[int, Tuple[np.ndarray, np.ndarray]], pose_min_samples: int):
    """The 6 N x 6 N normal equations over the cameras that have a usable pair.  Returns (uids in system order, H, g, [per usable pair: (a, b,
    M (6, 12), H6, g6, rr, tn)])."""
    usable = [(a, b) for (a, b) in sorted(rows) if int(rows[(a, b)][0]) >= int(pose_min_samples) and a in poses and b in poses]
    uids = sorted({u for ab in usable for u in ab})
    at = {u: i for i, u in enumerate(uids)}
    H = np.zeros((6 * len(uids), 6 * len(uids)))
    g = np.zeros(6 * len(uids))
    parts = []
    for (a, b) in usable:
        R, t = relative(poses[a], poses[b])
        tn = float(np.linalg.norm(t))
        if not (np.isfinite(tn) and tn > 0.0):
            continue                                                    # (such a pair has no inlier: every sample is degenerate)
        H6, g6, rr = pair_system(rows[(a, b)])
        S = np.diag([1.0, 1.0, 1.0, 1.0 / tn, 1.0 / tn, 1.0 / tn])
        H6, g6 = S @ H6 @ S, S @ g6
        M = np.concatenate([-adjoint(R, t), np.eye(6)], axis=1)        # delta_rel = M (delta_A, delta_B)
        idx = np.r_[6 * at[a]:6 * at[a] + 6, 6 * at[b]:6 * at[b] + 6]
        H[np.ix_(idx, idx)] += M.T @ H6 @ M
        g[idx] += M.T @ g6
        parts.append((a, b, M, H6, g6, rr, tn))
    return uids, H, g, parts


def reduced(H: np.ndarray, G: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(Q2, Q2^T H Q2): an orthonormal basis of the gauge columns' orthogonal complement and the matrix there."""
    Q, _ = np.linalg.qr(G, mode="complete")
    rank = int(np.linalg.matrix_rank(G))
    Q2 = Q[:, rank:]
    return Q2, Q2.T @ H @ Q2


def solve(rows, poses, pose_min_samples: int = 256) -> dict:
    """One Gauss-Newton step.  ``poses``: {uid: (R, t)} f64.  Returns dict(uids, delta {uid: (6,)}, dropped, eig_min_rel, parts)."""
    uids, H, g, parts = assemble(rows, poses, pose_min_samples)
    if not uids:
        return dict(uids=[], delta={}, dropped=0, eig_min_rel=None, parts=[])
    Q2, Hr = reduced(H, gauge_columns([poses[u] for u in uids]))
    lam, V = np.linalg.eigh(0.5 * (Hr + Hr.T))
    top = float(lam[-1]) if lam.size else 0.0
    keep = lam > EIG_CUT * top if top > 0.0 else np.zeros(lam.shape, bool)
    gr = Q2.T @ g
    y = V[:, keep] @ ((V[:, keep].T @ gr) / lam[keep])
    delta = -(Q2 @ y)
    kept = lam[keep]
    return dict(uids=uids, delta={u: delta[6 * i:6 * i + 6] for i, u in enumerate(uids)}, dropped=int((~keep).sum()),
                eig_min_rel=float(kept[0] / top) if kept.size else None, parts=parts)


def corrected(pose, delta) -> Tuple[np.ndarray, np.ndarray]:
    E = exp_so3(delta[:3])
    return E @ pose[0], E @ pose[1] + np.asarray(delta[3:], np.float64)


def build_report(rows: Mapping[Tuple[int, int], Sequence[int]], records: Sequence[CameraRecord], pose_min_samples: int = 256,
                 pose_certainty: float = 0.5, pose_inlier_px: float = 8.0, names: Optional[Mapping[int, str]] = None) -> dict:
    """``rows``: {(reference uid, neighbour uid): the pair's 32 integers summed over the run}; ``records``: the cameras the run was given.
    Returns the report as plain JSON-able data: the corrected world-to-camera pose of every camera."""
    names = dict(names or {})
    name = lambda uid: names.get(uid, str(uid))
    poses = {int(r.uid): pose_of(r) for r in records}
    sol = solve(rows, poses, pose_min_samples)
    baselines = sorted(p[6] for p in sol["parts"])
    base = baselines[(len(baselines) - 1) // 2] if baselines else None                                  # (the lower median)
    n_pairs = {}
    for (a, b, *_rest) in sol["parts"]:
        n_pairs[a] = n_pairs.get(a, 0) + 1
        n_pairs[b] = n_pairs.get(b, 0) + 1
    cameras = []
    for rec in sorted(records, key=lambda r: int(r.uid)):
        uid = int(rec.uid)
        R, t = poses[uid]
        d = sol["delta"].get(uid)
        R1, t1 = corrected((R, t), d) if d is not None else (R, t)
        cameras.append({"uid": uid, "name": name(uid), "usable_pairs": n_pairs.get(uid, 0), "corrected": d is not None,
                        "input_qvec": [float(v) for v in colmap_io.quaternion_from_rotation(R)], "input_tvec": [float(v) for v in t],
                        "qvec": [float(v) for v in colmap_io.quaternion_from_rotation(R1)], "tvec": [float(v) for v in t1],
                        "rotation_step_deg": float(np.degrees(np.linalg.norm(d[:3]))) if d is not None else 0.0,
                        "translation_step_rel": float(np.linalg.norm(d[3:]) / base) if d is not None and base else 0.0})
    used = {(p[0], p[1]): p for p in sol["parts"]}
    pairs = []
    tot_before = tot_after = 0.0
    tot_n = 0
    for (a, b) in sorted(rows):
        row = [int(v) for v in rows[(a, b)]]
        n = row[0]
        entry = {"reference_uid": int(a), "reference": name(a), "neighbour_uid": int(b), "neighbour": name(b), "inliers": n, "outliers": row[1],
                 "degenerate": row[2], "usable": (a, b) in used, "rms_px": float(np.sqrt(row[3] / 1048576.0 / n)) if n > 0 else None,
                 "predicted_rms_px": None}
        if (a, b) in used:
            _a, _b, M, H6, g6, rr, _tn = used[(a, b)]
            d_rel = M @ np.concatenate([sol["delta"][a], sol["delta"][b]])
            after = max(0.0, float(rr + 2.0 * g6 @ d_rel + d_rel @ H6 @ d_rel))
            entry["predicted_rms_px"] = float(np.sqrt(after / n))
            tot_before, tot_after, tot_n = tot_before + rr, tot_after + after, tot_n + n
        pairs.append(entry)
    return {"knobs": {"pose_certainty": float(pose_certainty), "pose_inlier_px": float(pose_inlier_px), "pose_min_samples": int(pose_min_samples)},
            "convention": "world-to-camera, qvec = (w, x, y, z); one Gauss-Newton step on the epipolar error, fixed up to the projected gauge",
            "cameras": cameras, "pairs": pairs,
            "scene": {"usable_pairs": len(used), "pairs_ignored": [[p["reference_uid"], p["neighbour_uid"]] for p in pairs if not p["usable"]],
                      "cameras_corrected": len(sol["delta"]), "cameras_left_out": [c["uid"] for c in cameras if not c["corrected"]],
                      "dropped_directions": sol["dropped"], "eig_min_rel": sol["eig_min_rel"], "median_baseline": base, "inliers": tot_n,
                      "rms_px": float(np.sqrt(tot_before / tot_n)) if tot_n else None,
                      "predicted_rms_px": float(np.sqrt(tot_after / tot_n)) if tot_n else None,
                      "max_rotation_step_deg": max([c["rotation_step_deg"] for c in cameras], default=0.0)}}


def summary_line(report: dict) -> str:
    s = report["scene"]
    fmt = lambda v: "n/a" if v is None else f"{v:.3f}"
    return (f"pose refinement: {s['cameras_corrected']} cameras corrected from {s['usable_pairs']} usable pairs ({len(s['pairs_ignored'])} ignored, "
            f"{len(s['cameras_left_out'])} cameras left out, {s['dropped_directions']} directions dropped): rms distance from the epipolar lines "
            f"{fmt(s['rms_px'])} px, {fmt(s['predicted_rms_px'])} px predicted after the step; largest rotation step {s['max_rotation_step_deg']:.3f} deg")


def warnings(report: dict) -> List[str]:
    """One warning per camera whose rotation step exceeds WARN_STEP_DEG."""
    return [f"pose refinement: camera {c['name']} (uid {c['uid']}) moves by {c['rotation_step_deg']:.2f} degrees: one linear step cannot be trusted "
            f"that far from the input pose (above {WARN_STEP_DEG:g} degrees); re-estimate the poses" for c in report["cameras"]
            if c["rotation_step_deg"] > WARN_STEP_DEG]


def to_json(report: dict) -> str:
    return json.dumps(report, indent=1, sort_keys=True) + "\n"


def from_json(text: str) -> dict:
    rep = json.loads(text)
    if not isinstance(rep, dict) or "cameras" not in rep:
        raise ValueError("not a poses.json: no 'cameras'")
    return rep


def apply_corrections(records: Sequence[CameraRecord], report: dict, log=None) -> List[CameraRecord]:
    """The records with the file's poses: a camera the file names (by uid) is rebuilt with CameraRecord.from_krt from its absolute qvec / tvec;
    one whose current pose is not the file's input_* (beyond f32 rounding) is refused - the corrections were computed for other poses; cameras
    the file does not name stay as they are, and one line counts them."""
    by_uid = {int(c["uid"]): c for c in report["cameras"]}
    out, unnamed = [], 0
    for rec in records:
        c = by_uid.get(int(rec.uid))
        if c is None:
            unnamed += 1
            out.append(rec)
            continue
        R, t = pose_of(rec)
        R_in = colmap_io._Rotation(c["input_qvec"]).matrix()
        if np.abs(R - R_in).max() > F32_POSE_TOL or np.abs(t - np.asarray(c["input_tvec"], np.float64)).max() > F32_POSE_TOL * max(1.0, float(np.abs(t).max())):
            raise ValueError(f"pose_corrections: camera {c.get('name', rec.uid)} (uid {int(rec.uid)}) has another pose than the file's input: the "
                             "corrections were computed for other poses")
        new = CameraRecord.from_krt(rec.uid, rec.K, colmap_io._Rotation(c["qvec"]).matrix(), np.asarray(c["tvec"], np.float64), rec.width, rec.height,
                                    image_path=rec.image_path, mask_path=rec.mask_path)
        out.append(dataclasses.replace(new, distortion=rec.distortion, distortion_model=rec.distortion_model))
    if unnamed and log is not None:
        log.info(f"pose_corrections: {unnamed} of {len(out)} cameras are not named by the file and keep their poses")
    return out
