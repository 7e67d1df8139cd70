#!/usr/bin/env python3
"""Entry points of the dense-initialisation pass (upstream densify.py:148-420).

``dense_init`` (COLMAP scene on disk / CLI), ``dense_init_from_lfs`` (camera nodes handed over by
LichtFeld Studio's GUI job) and ``build_argparser`` keep upstream's signatures, flags, return codes
and progress milestones; the body is host glue around ``core.pipeline.run_dense_pipeline`` whose
per-reference hot path runs on the GPU.
"""
from __future__ import annotations

import argparse
import json
import math
import os
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np

from .core.hostlog import log
from .core.image_io import find_image, image_dir, to_uint8_rgb
from .core.pipeline import PipelineCancelled, run_dense_pipeline
from .core.selection import nearest_neighbors, select_cameras_by_visibility, select_cameras_kcenters
from .core.types import CameraRecord, DensePipelineConfig, TRIANGULATION_MODES
from .core.writers import write_ply, write_points3D_bin


# ---- COLMAP -> CameraRecord (upstream core/geometry.py:10-50, densify.py:53-88) ----------------------
def K_from_camera(cam) -> np.ndarray:
    """3x3 f32 intrinsics from a pycolmap camera: (fx, fy, cx, cy) by model family; distortion
    parameters are ignored exactly as upstream ignores them."""
    model = str(cam.model.name).upper()
    p = np.asarray(cam.params, dtype=np.float32)
    # upstream's chain IN ITS ORDER (core/geometry.py:15-30): SIMPLE_RADIAL_FISHEYE is a SIMPLE_RADIAL before it is a FISHEYE
    # (found by tests/golden/check_oracle_fuzz.py: the two 4-parameter tests had been merged in front of the 3-parameter ones)
    if "PINHOLE" in model and "SIMPLE" not in model:
        fx, fy, cx, cy = p[0], p[1], p[2], p[3]
    elif "SIMPLE_PINHOLE" in model or "SIMPLE_RADIAL" in model or model == "RADIAL":
        fx = fy = p[0]
        cx, cy = p[1], p[2]
    elif "OPENCV" in model or "FISHEYE" in model:
        fx, fy, cx, cy = p[0], p[1], p[2], p[3]
    else:
        fx = fy = p[0]
        cx = p[1] if len(p) > 1 else cam.width / 2
        cy = p[2] if len(p) > 2 else cam.height / 2
    K = np.eye(3, dtype=np.float32)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = fx, fy, cx, cy
    return K


def distortion_from_camera(cam) -> Optional[Tuple[float, ...]]:
    """``(fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6)`` of a COLMAP camera (pycolmap's or core/colmap_io.Camera) in f64, exactly as the
    model stores them - what experimental['undistort_images'] resamples the image through - or None for a model the
    undistortion does not support: the fisheye family, FOV, anything unknown.  The name is tested as ``K_from_camera`` tests it, with the
    fisheye models taken out first: SIMPLE_RADIAL_FISHEYE contains SIMPLE_RADIAL but is a fisheye model."""
    model = str(cam.model.name).upper()
    p = [float(v) for v in np.asarray(cam.params, dtype=np.float64).reshape(-1)]
    zero = [0.0] * 8
    if "FISHEYE" in model:
        return None
    if model == "PINHOLE" and len(p) == 4:
        return tuple(p + zero)
    if model == "SIMPLE_PINHOLE" and len(p) == 3:
        return (p[0], p[0], p[1], p[2], *zero)
    if model == "SIMPLE_RADIAL" and len(p) == 4:
        return (p[0], p[0], p[1], p[2], p[3], *zero[1:])
    if model == "RADIAL" and len(p) == 5:
        return (p[0], p[0], p[1], p[2], p[3], p[4], *zero[2:])
    if model == "OPENCV" and len(p) == 8:
        return tuple(p + zero[4:])
    if model == "FULL_OPENCV" and len(p) == 12:
        return tuple(p)
    return None


def pose_world2cam(im) -> Tuple[np.ndarray, np.ndarray]:
    if hasattr(im, "cam_from_world"):
        cfw = im.cam_from_world
        cfw = cfw() if callable(cfw) else cfw
        R = np.asarray(cfw.rotation.matrix(), dtype=np.float32)
        t = np.asarray(cfw.translation, dtype=np.float32).reshape(3, 1)
    else:
        R = im.qvec.to_rotation_matrix()
        t = np.asarray(im.tvec, dtype=np.float32).reshape(3, 1)
    return R, t


def load_reconstruction(sparse_dir: str):
    """``pycolmap.Reconstruction`` like upstream (densify.py:54-56) when pycolmap is installed; otherwise the same three files read by
    core/colmap_io.py (cameras / images / points3D, .bin or .txt), which offers the attributes upstream touches."""
    try:
        import pycolmap
    except ImportError:
        from .core.colmap_io import Reconstruction
        rec = Reconstruction(sparse_dir)
        log.info(f"pycolmap is not installed: read {len(rec.images)} images / {len(rec.cameras)} cameras from {sparse_dir} with the built-in reader")
        return rec, rec.cameras, rec.images
    rec = pycolmap.Reconstruction(sparse_dir)
    return rec, rec.cameras, rec.images


def camera_records_from_colmap(cams: Dict, imgs: Dict, images_dir: str) -> Tuple[List[CameraRecord], List[int]]:
    records: List[CameraRecord] = []
    img_ids = sorted(imgs.keys())
    for iid in img_ids:
        im = imgs[iid]
        cam = cams[im.camera_id]
        R, t = pose_world2cam(im)
        rec = CameraRecord.from_krt(iid, K_from_camera(cam), R, t, cam.width, cam.height,
                                    image_path=find_image(images_dir, im.name))
        rec.distortion, rec.distortion_model = distortion_from_camera(cam), str(cam.model.name).upper()
        records.append(rec)
    return records, img_ids


def extract_cameras_from_lfs(camera_nodes) -> List[CameraRecord]:
    """Scene camera nodes -> records; the principal point is assumed at the image centre
    (upstream densify.py:215-245)."""
    records: List[CameraRecord] = []
    for node in camera_nodes:
        if not getattr(node, "has_camera", False):
            continue
        w, h = node.camera_width, node.camera_height
        K = np.array([[node.camera_focal_x, 0.0, w / 2.0], [0.0, node.camera_focal_y, h / 2.0], [0.0, 0.0, 1.0]],
                     dtype=np.float32)
        rec = CameraRecord.from_krt(node.camera_uid, K, node.camera_R, node.camera_T, w, h, image_path=node.image_path,
                                    mask_path=(node.mask_path if getattr(node, "has_mask", False) else None))
        records.append(rec)
    return records


# ---- post-processing ------------------------------------------------------------------------------
def _flat_pose_stack(records: List[CameraRecord]) -> np.ndarray:
    return np.stack([c.flat_pose() for c in records], axis=0)


def _num_refs(fraction_or_count: float, n: int) -> int:
    return int(round(fraction_or_count * n)) if fraction_or_count <= 1.0 else int(fraction_or_count)


def _effective_neighbor_count(requested: int, camera_count: int) -> int:
    if camera_count <= 1:
        return 0
    return max(1, min(int(requested), camera_count - 1))


def _cap_index(n_before: int, max_points: int, seed: int) -> Optional[np.ndarray]:
    """The rows the point cap keeps (upstream densify.py's draw), or None when the cap does not act: the ONE place the choice is made - the
    host arrays, the device tensors and the normals all index with it."""
    if max_points > 0 and n_before > max_points:
        return np.random.default_rng(seed).choice(n_before, size=max_points, replace=False)
    return None


class SpatialCapRefused(RuntimeError):
    """experimental['cap_mode'] = 'spatial': the library refused the cloud (a non-finite coordinate).  No draw stands in for it."""


def _cap_keep(xyz, err, max_points: int, seed: int, cap_mode: str = "random", host_threads: int = 0, progress_callback=None):
    """The rows the point cap keeps of this cloud, or None when the cap does not act - beside ``_cap_index``, the one place the choice is made:
    the points, the normals and the GPU copy all index with what this returns.  ``cap_mode`` 'random': ``_cap_index``, a NumPy index.
    'spatial' (DESIGN.md 4.19): lfd_cap_spatial where ``xyz`` / ``err`` are - device tensors through the device call, an int64 tensor that
    stays on the GPU; host arrays or CPU tensors through the twin, a NumPy index.  Ascending: the kept cloud is the input under a mask."""
    n_before = int(xyz.shape[0])
    if cap_mode != "spatial":
        return _cap_index(n_before, max_points, seed)
    if not (max_points > 0 and n_before > max_points):
        return None
    from .core import hip_backend as hb
    import torch
    as_tensor = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))      # noqa: E731
    t_xyz, t_err = as_tensor(xyz), (None if err is None else as_tensor(err))
    on_gpu = bool(t_xyz.is_cuda)
    if progress_callback:
        progress_callback(95.0, "Choosing points (spatial cap)...")
    dens = hb.HipDensifier(t_xyz.device) if on_gpu else hb.HostDensifier(int(host_threads))
    try:
        keep = dens.cap_spatial(t_xyz, t_err, int(max_points))
        lev, cells, _above, _side = dens.cap_stats
    except hb.CapInputRefused as exc:
        raise SpatialCapRefused(f"experimental['cap_mode'] = 'spatial' cannot be applied to this cloud of {n_before:,} points: {exc}") from exc
    finally:
        dens.close()
    log.info(f"Spatial cap: {n_before:,} points in, {int(keep.shape[0]):,} kept, level {lev}, {cells:,} cells")
    return keep if on_gpu else keep.numpy()


def _take_rows(a, keep):
    """``a`` (a NumPy array, a tensor wherever it lives, or None) under the cap's index (a NumPy index, or a tensor wherever it lives)."""
    if a is None or keep is None:
        return a
    if isinstance(a, np.ndarray):
        return a[keep if isinstance(keep, np.ndarray) else keep.cpu().numpy()]
    import torch
    return a[(torch.from_numpy(keep) if isinstance(keep, np.ndarray) else keep).to(a.device)]


def _apply_point_cap(xyz, rgb, err, max_points: int, seed: int, cap_mode: str = "random", host_threads: int = 0):
    keep = _cap_keep(xyz, err, max_points, seed, cap_mode, host_threads)
    return _take_rows(xyz, keep), _take_rows(rgb, keep), _take_rows(err, keep)


def _cap_args(config) -> dict:
    """``_cap_keep``'s mode arguments of a configuration (None: upstream's draw)."""
    return {} if config is None else {"cap_mode": str(config.exp("cap_mode")), "host_threads": int(config.exp("host_threads"))}


def _finish_on_device(result, path: str, max_points: int, seed: int, clock=None, config=None, progress_callback=None, shell=None) -> Optional[int]:
    """Point cap + output file for a result whose points are still on the GPU, without ever bringing the f32 cloud to the host: the same subset
    ``_apply_point_cap`` picks (the same generator, the same call), applied to the device tensors, then the file payload packed on the device
    (``_write_output``).  Returns the number of points written, or None when the result is not on a GPU (the host path applies)."""
    pts = result.device_points
    if pts is None or not pts[0].is_cuda:
        return None
    keep = _cap_keep(pts[0], pts[2] if len(pts) > 2 else None, max_points, seed, progress_callback=progress_callback, **_cap_args(config))
    normals = _take_rows(result.device_normals, keep)           # (the index of a spatial cap is a device tensor: it never leaves the GPU)
    pts = _cap_device_points(pts, keep)
    if config is not None and float(config.exp("fuse_voxel_size")) > 0.0:      # (behind the cap, in front of packing)
        xyz, normals, rgb = _apply_oriented_fusion(config, pts[0], normals, pts[1], progress_callback)
        pts = (xyz, rgb)
    n = int(pts[0].shape[0])
    if config is not None and bool(config.exp("gaussian_init")):              # (the last stage: it replaces the 27-byte packing)
        _write_gaussians(config, path, pts[0], normals, pts[1], clock=clock, progress_callback=progress_callback)
        if shell is not None:
            shell.write_file(pts[0], normals is not None, clock)
        return n
    _write_final(shell, path, np.empty((n, 0), np.float32), None, None, pts, clock=clock, normals=normals)
    return n


def _voxel_downsample(xyz: np.ndarray, rgb: np.ndarray, voxel_size: float) -> Tuple[np.ndarray, np.ndarray]:
    """One averaged point (and colour) per occupied voxel.  Uses Open3D when installed (upstream
    densify.py:29-50); otherwise an equivalent NumPy voxel-grid average (voxel order then follows the
    sorted voxel index instead of Open3D's hash order)."""
    col = rgb[:, :3].astype(np.float64) / (255.0 if rgb.size and rgb.max() > 1.0 else 1.0)
    try:
        import open3d as o3d
        pcd = o3d.geometry.PointCloud()
        pcd.points = o3d.utility.Vector3dVector(xyz.astype(np.float64))
        pcd.colors = o3d.utility.Vector3dVector(col)
        down = pcd.voxel_down_sample(voxel_size=float(voxel_size))
        return np.asarray(down.points, dtype=np.float32), np.asarray(down.colors, dtype=np.float32)
    except ImportError:
        pts = xyz.astype(np.float64)
        origin = pts.min(axis=0) - 0.5 * voxel_size
        key = np.floor((pts - origin) / float(voxel_size)).astype(np.int64)
        _, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
        inv = inv.reshape(-1)
        p = np.zeros((cnt.size, 3))
        c = np.zeros((cnt.size, 3))
        np.add.at(p, inv, pts)
        np.add.at(c, inv, col)
        return (p / cnt[:, None]).astype(np.float32), (c / cnt[:, None]).astype(np.float32)


def _voxel_filter_on_device(device_points, voxel_size: float):
    """``_voxel_downsample`` where the points are (lfd_voxel_downsample): ``(xyz, rgb)`` device tensors, bit for bit and in the order of its
    NumPy branch.  None when the library refuses the cloud (a non-finite coordinate, a voxel key range beyond 63 bits): the host filters it."""
    from .core import hip_backend as hb
    dens = hb.HipDensifier(device_points[0].device)
    try:
        return dens.voxel_downsample(device_points[0], device_points[1], voxel_size)
    except hb.VoxelInputRefused as exc:
        log.warn(f"Distance filter: {exc}; filtering on the host")
        return None
    finally:
        dens.close()


def _apply_gain_compensation(result, config: DensePipelineConfig, camera_records, refs_local, progress_callback=None):
    """Per-image exposure gains (experimental['gain_compensation']) on the collected cloud, in front of every cloud stage
    while the per-reference counts are still the loop's: the factors are solved from the run's statistics (core/gains.py),
    ``<output file>.gains.json`` is written, and every point's colour is multiplied by its reference's factor where the points are - the
    device tensors of a GPU run through lfd_gain_apply, the host arrays of ``backend='host'`` through the twin.  Returns the result with the
    new rgb; points, counts, order, xyz and err are the input's.  Off: the result itself, nothing runs."""
    mode = str(config.exp("gain_compensation"))
    if mode == "off":
        return result
    import json
    import torch
    from .core import hip_backend as hb
    from .core.gains import solve_gains
    from .core.sinks import PipelineResult
    if result.streamed_path is not None or result.gain_rows is None:
        raise RuntimeError("experimental['gain_compensation'] needs the cloud held as arrays and the run's statistics: this result has neither")
    counts = np.asarray(result.points_per_reference, np.int64)
    pts = result.device_points
    if pts is None:
        pts = tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in (result.xyz, result.rgb, result.err))
    n_in = int(pts[0].shape[0])
    if counts.size != len(refs_local) or int(counts.sum()) != n_in:
        raise RuntimeError(f"experimental['gain_compensation'] needs the whole cloud with its per-reference counts: this result holds {n_in:,} "
                           f"points in {counts.size} counts that add up to {int(counts.sum()):,}, the run has {len(refs_local)} references")
    if progress_callback:
        progress_callback(91.0, "Applying gain compensation...")
    uids = [int(c.uid) for c in camera_records]
    sol = solve_gains(result.gain_rows, uids, mode, warn=log.warn)
    by_uid = sol.factor_of()
    factors = np.stack([by_uid[int(camera_records[int(ci)].uid)] for ci in refs_local]).astype(np.float32)
    names = {int(c.uid): os.path.basename(str(c.image_path)) for c in camera_records}
    with open(str(config.output_path) + ".gains.json", "w") as f:
        json.dump(sol.to_json(names), f, indent=1)
    on_gpu = bool(pts[0].is_cuda)
    dens = hb.HipDensifier(pts[0].device) if on_gpu else hb.HostDensifier(int(config.exp("host_threads")))
    try:
        rgb = dens.gain_apply(pts[1], counts, factors)
    finally:
        dens.close()
    used = factors[counts > 0] if (counts > 0).any() else np.ones((1, 3), np.float32)       # (an empty cloud: nothing was multiplied)
    log.info(f"Gain compensation ({mode}): {int(sol.pairs.sum()) // 2} pairs in {sol.n_components} component(s), {sol.rows_ignored} rows ignored, "
             f"factors of the references {float(used.min()):.4f} .. {float(used.max()):.4f}, {len(sol.clamped)} clamped")
    new_pts = (pts[0], rgb, pts[2])
    if on_gpu:
        clock = result._clock

        def loader(p=new_pts, clk=clock):
            if hasattr(clk, "stage"):
                with clk.stage("d2h"):
                    return tuple(t.cpu().numpy() for t in p)
            return tuple(t.cpu().numpy() for t in p)
        arrays = (None, None, None)
    else:
        loader, arrays = None, tuple(t.numpy() for t in new_pts)
    out = PipelineResult(xyz=arrays[0], rgb=arrays[1], err=arrays[2], elapsed_seconds=result.elapsed_seconds, pairs_processed=result.pairs_processed,
                         pairs_matched=result.pairs_matched, points_per_reference=result.points_per_reference, device_points=new_pts,
                         streamed_path=None, clock=result._clock, loader=loader, device_normals=result.device_normals, match_grid=result.match_grid)
    out.gain_rows = result.gain_rows
    return out


class FarShell:
    """The far-field shell of a run (experimental['far_shell']) between the pipeline and the writers: the run's direction
    table and what ``emit`` needs to place it around the final cloud - behind every filter, thinning, cap and fusion, in front of packing.
    Centre: the f64 mean of the loaded cameras' centres; automatic radius: max(10 x the largest distance of a camera from the centre,
    1.25 x the largest distance of a point of the final cloud), the cloud's taken where the cloud lives - squares and sums as separate f64
    operations, the same bits on either route."""

    def __init__(self, stats: dict, config: DensePipelineConfig, camera_records):
        self.config, self.stats, self.mode = config, stats, str(config.exp("far_shell"))
        self.table = stats["table"]
        self.names = {int(c.uid): os.path.basename(str(c.image_path)) for c in camera_records}
        centres = np.stack([np.asarray(c.C, np.float64).reshape(3) for c in camera_records])
        self.centre = centres.mean(axis=0)
        d = centres - self.centre
        sq = d * d
        self.r_cams = float(np.sqrt(((sq[:, 0] + sq[:, 1]) + sq[:, 2]).max()))
        self.shell_path = os.path.splitext(str(config.output_path))[0] + "_shell.ply"

    def radius(self, xyz) -> float:
        import torch
        fixed = float(self.config.exp("far_shell_radius"))
        if fixed > 0.0:
            return fixed
        r_cloud = 0.0
        if xyz is not None and int(xyz.shape[0]) > 0:
            t = xyz if isinstance(xyz, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(xyz))
            d = t.to(torch.float64) - torch.from_numpy(self.centre).to(t.device)
            sq = d * d
            r_cloud = float(torch.sqrt(((sq[:, 0] + sq[:, 1]) + sq[:, 2]).max()).item())
        r = max(10.0 * self.r_cams, 1.25 * r_cloud)
        return r if r > 0.0 else 1.0                    # (one camera and no cloud: any positive radius is as good as another)

    def emit(self, xyz, with_normals: bool):
        """The shell around the final cloud ``xyz`` (array or tensor, where it lives): (xyz, rgb, normals or None) tensors where the table
        lives, and ``<output file>.shell.json`` beside the output."""
        import json
        from .core import hip_backend as hb
        cfg = self.config
        S, min_samples = int(cfg.exp("far_shell_cells")), int(cfg.exp("far_min_samples"))
        radius = self.radius(xyz)
        dens = hb.HipDensifier(self.table.device) if self.table.is_cuda else hb.HostDensifier(int(cfg.exp("host_threads")))
        try:
            sx, srgb, snrm, samples = dens.far_emit(self.table, S, min_samples, self.centre, radius, with_normals=with_normals)
        finally:
            dens.close()
        count = self.table[:, 6]
        report = {"mode": self.mode, "far_thresh_px": float(cfg.far_threshold()), "far_certainty": float(cfg.exp("far_certainty")),
                  "far_min_views": int(cfg.exp("far_min_views")), "far_shell_cells": S, "far_min_samples": min_samples,
                  "far_shell_radius": float(cfg.exp("far_shell_radius")), "centre": [float(v) for v in self.centre], "radius": float(radius),
                  "direction_cells": 6 * S * S, "cells_occupied": int((count > 0).sum()), "cells_kept": int(sx.shape[0]),
                  "samples": int(count.sum()), "samples_kept": int(samples.sum()),
                  "far_cells": {self.names.get(uid, str(uid)): int(n) for uid, n in sorted(self.stats["far_cells"].items())},
                  "far_cells_with_a_point": int(self.stats["overlap"])}
        if _is_writer_rank():
            with open(str(cfg.output_path) + ".shell.json", "w") as f:
                json.dump(report, f, indent=1)
        log.info(f"Far-field shell ({self.mode}): {report['cells_kept']} points from {report['samples_kept']} samples in {report['cells_occupied']} "
                 f"occupied direction cells (S = {S}, at least {min_samples} samples), radius {radius:.4g} around the cameras' centre")
        return sx, srgb, snrm

    def write_file(self, xyz, with_normals: bool, clock=None) -> None:
        """'file' mode beside an output this module does not pack itself (the Gaussian file, a PLY under another name)."""
        sx, srgb, snrm = self.emit(xyz, with_normals)
        _write_shell_file(self.shell_path, sx, srgb, snrm, clock)


def _write_shell_file(path: str, sx, srgb, snrm, clock=None) -> None:
    n = int(sx.shape[0])
    if sx.is_cuda:
        _write_output(path, np.empty((n, 0), np.float32), None, None, (sx, srgb), clock=clock, as_ply=True, normals=snrm)
    else:
        _write_output(path, sx.numpy(), srgb.numpy(), None, None, as_ply=True, normals=snrm.numpy() if snrm is not None else None)


def _check_audit_maps(config: DensePipelineConfig, camera_records) -> None:
    """experimental['audit_maps_dir'] names a reference's map after its image file, as the depth maps do: refused before the run when two image
    files share a stem."""
    if str(config.exp("epipolar_audit")) == "off" or str(config.exp("audit_maps_dir")) == "":
        return
    stems = {}
    for rec in camera_records:
        stem = os.path.splitext(os.path.basename(str(rec.image_path)))[0]
        if stem == "" or stem in stems:
            raise RuntimeError(f"experimental['audit_maps_dir'] names a camera's maps after its image file: {stems.get(stem, rec).image_path!r} and "
                               f"{rec.image_path!r} both give {stem!r}")
        stems[stem] = rec


def _write_audit(result, config: DensePipelineConfig, camera_records) -> None:
    """The epipolar audit of a run (experimental['epipolar_audit']): ``<output file>.audit.json`` - the knobs, every pair's
    histogram and quantiles, every camera's score, the scene summary; no timing, so a device run and a host run write the same bytes - one
    summary line, and one warning per suspect camera (one in all when more than half of them are).  With experimental['audit_maps_dir'] every
    REFERENCE also gets ``<image stem>_epi.npy``: f32 (H, W), the smallest distance from the epipolar line any confident neighbour reports for
    the cell, in px of that neighbour's camera image (bin / 8), NaN where there is none.  A side output: ``result`` is not changed."""
    if str(config.exp("epipolar_audit")) == "off" or not _is_writer_rank():
        return
    from .core import audit as audit_report
    got = getattr(result, "epipolar_audit", None)
    if got is None:
        raise RuntimeError("experimental['epipolar_audit'] needs the run's histograms: this result has none")
    report = dict(got["report"])
    maps_dir = str(config.exp("audit_maps_dir"))
    if maps_dir != "":
        _check_audit_maps(config, camera_records)
        rel = maps_dir
        if not os.path.isabs(maps_dir):
            maps_dir = os.path.join(os.path.dirname(os.path.abspath(config.output_path)), maps_dir)
        os.makedirs(maps_dir, exist_ok=True)
        by_uid = {int(c.uid): c for c in camera_records}
        entries = []
        for uid in sorted(got["maps"] or {}):
            m = got["maps"][uid]
            stem = os.path.splitext(os.path.basename(str(by_uid[uid].image_path)))[0]
            px = np.where(m == 255, np.float32(np.nan), m.astype(np.float32) / np.float32(8.0)).astype(np.float32)
            np.save(os.path.join(maps_dir, stem + "_epi.npy"), px)
            entries.append({"uid": uid, "image": os.path.basename(str(by_uid[uid].image_path)), "map": stem + "_epi.npy",
                            "height": int(m.shape[0]), "width": int(m.shape[1]), "cells_with_data": int((m != 255).sum())})
        report["maps"] = {"dir": rel, "unit": "px of the winning neighbour's camera image, lower edge of the bin", "references": entries}
    with open(str(config.output_path) + ".audit.json", "w") as f:
        f.write(audit_report.to_json(report))
    log.info(audit_report.summary_line(report))
    for line in audit_report.warnings(report):
        log.warn(line)


def _load_pose_corrections(config: DensePipelineConfig, camera_records):
    """experimental['pose_corrections']: the records with the poses of that poses.json (core/poses.py: apply_corrections) - what a second run
    densifies with.  The reference views and their neighbours were chosen from the input poses, so both runs match the same pairs.  '' = the
    records as they are."""
    path = str(config.exp("pose_corrections"))
    if path == "":
        return camera_records
    from .core import poses as pose_report
    with open(path) as f:
        report = pose_report.from_json(f.read())
    out = pose_report.apply_corrections(camera_records, report, log)
    log.info(f"pose_corrections: {sum(a is not b for a, b in zip(out, camera_records))} camera poses taken from {path}")
    return out


def _write_poses(result, config: DensePipelineConfig) -> None:
    """The pose refinement of a run (experimental['pose_refine']): ``<output file>.poses.json`` - the knobs, one corrected
    world-to-camera pose per camera beside its input pose, every pair's counts and rms distance before and (predicted) after the step, the
    scene totals; no timing, so a device run and a host run write the same bytes - one summary line, and one warning per camera whose step
    is too large for a linear step.  A side output: ``result`` is not changed."""
    if str(config.exp("pose_refine")) == "off" or not _is_writer_rank():
        return
    from .core import poses as pose_report
    got = getattr(result, "pose_refine", None)
    if got is None:
        raise RuntimeError("experimental['pose_refine'] needs the run's normal equations: this result has none")
    with open(str(config.output_path) + ".poses.json", "w") as f:
        f.write(pose_report.to_json(got["report"]))
    log.info(pose_report.summary_line(got["report"]))
    for line in pose_report.warnings(got["report"]):
        log.warn(line)


def _far_shell_of(result, config: DensePipelineConfig, camera_records):
    """The run's FarShell, or None with the knob off (nothing runs)."""
    if str(config.exp("far_shell")) == "off":
        return None
    if result.streamed_path is not None or getattr(result, "far_shell", None) is None:
        raise RuntimeError("experimental['far_shell'] needs the cloud held as arrays and the run's direction table: this result has neither")
    return FarShell(result.far_shell, config, camera_records)


def _apply_consensus_filter(result, config: DensePipelineConfig, progress_callback=None):
    """The cross-reference consensus filter on the finished cloud (lfd_consensus_filter), where the points are: the device
    tensors of a GPU run through the device call, the host arrays of ``backend='host'`` through the twin.  Returns the result with the kept
    points (input order, same bits) and their per-reference counts in place of the cloud; everything downstream - cap, voxel filter, packing,
    writers - sees an ordinary result.  Off (experimental['min_consensus_refs'] = 0): the result itself, nothing runs."""
    min_refs = int(config.exp("min_consensus_refs"))
    if min_refs <= 0 or result.streamed_path is not None:
        return result
    from .core import hip_backend as hb
    from .core.sinks import PipelineResult
    import torch
    radius = float(config.exp("consensus_radius"))
    pts = result.device_points
    if pts is None:
        pts = tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in (result.xyz, result.rgb, result.err))
    counts = np.asarray(result.points_per_reference, np.int64)
    n_in = int(pts[0].shape[0])
    if int(counts.sum()) != n_in:
        raise RuntimeError(f"experimental['min_consensus_refs'] needs the whole cloud with its per-reference counts: this result holds {n_in:,} "
                           f"points, the counts add up to {int(counts.sum()):,} (a rank of a gather_to_root run that is not the root)")
    if progress_callback:
        progress_callback(92.0, "Applying consensus filter...")
    on_gpu = bool(pts[0].is_cuda)
    dens = hb.HipDensifier(pts[0].device) if on_gpu else hb.HostDensifier(int(config.exp("host_threads")))
    normals = result.device_normals                  # experimental['estimate_normals']: the filter's keep decision applies to them as well
    try:
        xyz, rgb, err, kept, cons = dens.consensus_filter(pts[0], pts[1], pts[2], counts, radius, min_refs, with_consensus=normals is not None)
        if normals is not None:
            # the compaction is the library's; its per-point count gives the rows it kept, and that is CHECKED, not assumed: the input
            # positions under the mask must be the kept positions bit for bit before the mask is applied to the normals
            keep = cons >= min_refs
            if int(keep.sum()) != int(xyz.shape[0]) or not torch.equal(pts[0][keep].view(torch.int32), xyz.view(torch.int32)):
                raise RuntimeError("consensus filter: the per-point counts do not name the rows the filter kept; the normals cannot follow the points")
            normals = normals[keep]
    except hb.ConsensusInputRefused as exc:
        raise RuntimeError(f"experimental['consensus_radius'] = {radius:g} is too small for the extent of this cloud: {exc}") from exc
    finally:
        dens.close()
    n_kept = int(xyz.shape[0])
    log.info(f"Consensus filter (radius {radius:.4f}, {min_refs} other reference{'s' if min_refs != 1 else ''}): {n_in:,} points in, {n_kept:,} kept")
    new_pts = (xyz, rgb, err)
    if on_gpu:
        clock = result._clock

        def loader(p=new_pts, clk=clock):
            if hasattr(clk, "stage"):
                with clk.stage("d2h"):
                    return tuple(t.cpu().numpy() for t in p)
            return tuple(t.cpu().numpy() for t in p)
        arrays = (None, None, None)
    else:
        loader, arrays = None, tuple(t.numpy() for t in new_pts)
    return PipelineResult(xyz=arrays[0], rgb=arrays[1], err=arrays[2], elapsed_seconds=result.elapsed_seconds, pairs_processed=result.pairs_processed,
                          pairs_matched=result.pairs_matched, points_per_reference=kept, device_points=new_pts, streamed_path=None,
                          clock=result._clock, loader=loader, device_normals=normals, match_grid=result.match_grid)


def _image_plane(config: DensePipelineConfig, cells_key: str, width: int, height: int, match_grid=None) -> Tuple[int, int]:
    """(pw, ph) of a plane over images of ``width`` x ``height``: experimental[``cells_key``] cells along the longer side - 0:
    ceil(sqrt(matches_per_ref)) in sampled mode, the longer side of the matcher's grid (``match_grid`` = (H, W)) in dense mode - and
    max(1, floor(cells * short / long + 0.5)) along the shorter."""
    cells = int(config.exp(cells_key))
    if cells == 0:
        if config.triangulation_mode == "dense":
            if match_grid is None:
                raise RuntimeError(f"experimental['{cells_key}'] = 0 takes the matcher's grid in dense mode, and this result does not record one")
            cells = int(max(match_grid))
        else:
            cells = int(math.ceil(math.sqrt(max(1, int(config.matches_per_ref)))))
    lng, sht = max(int(width), int(height)), min(int(width), int(height))
    other = max(1, int(math.floor(cells * sht / lng + 0.5)))
    return (cells, other) if int(width) >= int(height) else (other, cells)


def freespace_plane(config: DensePipelineConfig, width: int, height: int, match_grid=None) -> Tuple[int, int]:
    """(pw, ph) of the free-space filter's z-buffers: ``_image_plane`` by experimental['freespace_plane_cells']."""
    return _image_plane(config, "freespace_plane_cells", width, height, match_grid)


def depth_map_plane(config: DensePipelineConfig, width: int, height: int, match_grid=None) -> Tuple[int, int]:
    """(pw, ph) of the depth maps: ``_image_plane`` by experimental['depth_map_cells']."""
    return _image_plane(config, "depth_map_cells", width, height, match_grid)


def _apply_freespace_filter(result, config: DensePipelineConfig, camera_records, refs_local, progress_callback=None):
    """The free-space filter on the finished cloud (lfd_freespace_filter), where the points are, behind the consensus filter
    and in front of the point cap and the voxel filter.  Entry i of ``result.points_per_reference`` is reference ``refs_local[i]``, whose
    camera is ``camera_records[refs_local[i]]``.  Returns the result with the kept points (input order, same bits) and their per-reference
    counts in place of the cloud.  Off (experimental['min_freespace_violations'] = 0): the result itself, nothing runs."""
    min_v = int(config.exp("min_freespace_violations"))
    if min_v <= 0 or result.streamed_path is not None:
        return result
    from .core import hip_backend as hb
    from .core.sinks import PipelineResult
    import torch
    tol = float(config.exp("freespace_depth_tol_rel"))
    pts = result.device_points
    if pts is None:
        pts = tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in (result.xyz, result.rgb, result.err))
    counts = np.asarray(result.points_per_reference, np.int64)
    n_in = int(pts[0].shape[0])
    if int(counts.sum()) != n_in or counts.size != len(refs_local):
        raise RuntimeError(f"experimental['min_freespace_violations'] needs the whole cloud with its per-reference counts: this result holds {n_in:,} "
                           f"points, the counts of {counts.size} of {len(refs_local)} references add up to {int(counts.sum()):,} (a rank of a "
                           "gather_to_root run that is not the root)")
    cams = [camera_records[int(r)] for r in refs_local]
    cam_P = np.stack([np.asarray(c.P, np.float64).astype(np.float32).reshape(12) for c in cams])
    cam_wh = np.array([[int(c.width), int(c.height)] for c in cams], np.int32)
    plane = freespace_plane(config, cams[0].width, cams[0].height, result.match_grid)
    if progress_callback:
        progress_callback(93.0, "Applying free-space filter...")
    on_gpu = bool(pts[0].is_cuda)
    dens = hb.HipDensifier(pts[0].device) if on_gpu else hb.HostDensifier(int(config.exp("host_threads")))
    normals = result.device_normals                  # experimental['estimate_normals']: the filter's keep decision applies to them as well
    try:
        xyz, rgb, err, kept, viol, supp = dens.freespace_filter(pts[0], pts[1], pts[2], counts, cam_P, cam_wh, plane, tol, min_v,
                                                                with_counts=normals is not None)
        if normals is not None:
            # the compaction is the library's; its per-point counts give the rows it kept, and that is CHECKED, not assumed: the input
            # positions under the mask must be the kept positions bit for bit before the mask is applied to the normals
            keep = ~((viol >= min_v) & (viol > supp))
            if int(keep.sum()) != int(xyz.shape[0]) or not torch.equal(pts[0][keep].view(torch.int32), xyz.view(torch.int32)):
                raise RuntimeError("free-space filter: the per-point counts do not name the rows the filter kept; the normals cannot follow the points")
            normals = normals[keep]
    except hb.HipBackendError as exc:
        raise RuntimeError(f"experimental['min_freespace_violations']: {exc}") from exc
    finally:
        dens.close()
    n_kept = int(xyz.shape[0])
    log.info(f"Free-space filter (tolerance {tol:g}, {min_v} refuting reference{'s' if min_v != 1 else ''}, planes of {plane[0]} x {plane[1]} cells): "
             f"{n_in:,} points in, {n_kept:,} kept")
    new_pts = (xyz, rgb, err)
    if on_gpu:
        clock = result._clock

        def loader(p=new_pts, clk=clock):
            if hasattr(clk, "stage"):
                with clk.stage("d2h"):
                    return tuple(t.cpu().numpy() for t in p)
            return tuple(t.cpu().numpy() for t in p)
        arrays = (None, None, None)
    else:
        loader, arrays = None, tuple(t.numpy() for t in new_pts)
    return PipelineResult(xyz=arrays[0], rgb=arrays[1], err=arrays[2], elapsed_seconds=result.elapsed_seconds, pairs_processed=result.pairs_processed,
                          pairs_matched=result.pairs_matched, points_per_reference=kept, device_points=new_pts, streamed_path=None,
                          clock=result._clock, loader=loader, device_normals=normals, match_grid=result.match_grid)


def component_report(radius: float, min_points: int, n_in: int, n_out: int, summary) -> dict:
    """What ``<output file>.components.json`` holds: the knobs, the points in and out, the number of components, the largest one and the two
    histograms over the bins 2^b <= size < 2^(b + 1) (trailing empty bins left out).  No timing: a device run and a host run write the same
    bytes."""
    s = [int(v) for v in np.asarray(summary, np.int64).reshape(66)]
    top = max([b + 1 for b in range(32) if s[2 + b]] or [0])
    return {"component_radius": float(radius), "min_component_points": int(min_points), "points_in": int(n_in), "points_out": int(n_out),
            "n_components": s[0], "largest_component": s[1],
            "bins": [{"size_from": 1 << b, "size_below": 1 << (b + 1), "components": s[2 + b], "points": s[34 + b]} for b in range(top)]}


def _apply_component_filter(result, config: DensePipelineConfig, progress_callback=None):
    """The connected-component filter on the finished cloud (lfd_component_filter), where the points are, behind the consensus
    and free-space filters and in front of the depth maps, thinning, cap, fusion, Gaussian output and voxel filter.  Returns the result with
    the kept points (input order, same bits), their normals and their per-reference counts in place of the cloud, and writes
    ``<output file>.components.json``.  Off (experimental['min_component_points'] = 0): the result itself, nothing runs."""
    min_points = int(config.exp("min_component_points"))
    if min_points <= 0 or result.streamed_path is not None:
        return result
    from .core import hip_backend as hb
    from .core.sinks import PipelineResult
    import torch
    radius = float(config.exp("component_radius"))
    pts = result.device_points
    if pts is None:
        pts = tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in (result.xyz, result.rgb, result.err))
    counts = np.asarray(result.points_per_reference, np.int64)
    n_in = int(pts[0].shape[0])
    if int(counts.sum()) != n_in:
        raise RuntimeError(f"experimental['min_component_points'] needs the whole cloud with its per-reference counts: this result holds {n_in:,} "
                           f"points, the counts add up to {int(counts.sum()):,} (a rank of a gather_to_root run that is not the root)")
    if progress_callback:
        progress_callback(93.5, "Applying component filter...")
    on_gpu = bool(pts[0].is_cuda)
    dens = hb.HipDensifier(pts[0].device) if on_gpu else hb.HostDensifier(int(config.exp("host_threads")))
    normals = result.device_normals                  # experimental['estimate_normals']: the filter's keep decision applies to them as well
    try:
        xyz, rgb, err, kept, sizes, labels, summary = dens.component_filter(pts[0], pts[1], pts[2], counts, radius, min_points,
                                                                            with_sizes=True, with_labels=True)
        keep = sizes >= min_points
        # a component's label is the index of one of its points: the dropped components are the dropped points that carry their own label
        heads = labels.long() == torch.arange(n_in, device=labels.device)
        n_dropped_components = int((heads & ~keep).sum())
        if normals is not None:
            # the compaction is the library's; its per-point size gives the rows it kept, and that is CHECKED, not assumed: the input
            # positions under the mask must be the kept positions bit for bit before the mask is applied to the normals
            if int(keep.sum()) != int(xyz.shape[0]) or not torch.equal(pts[0][keep].view(torch.int32), xyz.view(torch.int32)):
                raise RuntimeError("component filter: the per-point sizes do not name the rows the filter kept; the normals cannot follow the points")
            normals = normals[keep]
    except hb.ConsensusInputRefused as exc:
        raise RuntimeError(f"experimental['component_radius'] = {radius:g} is too small for the extent of this cloud: {exc}") from exc
    finally:
        dens.close()
    n_kept = int(xyz.shape[0])
    report = component_report(radius, min_points, n_in, n_kept, summary)
    if _is_writer_rank():
        with open(str(config.output_path) + ".components.json", "w") as f:
            f.write(json.dumps(report, indent=1) + "\n")
    log.info(f"Component filter (radius {radius:.4f}, at least {min_points:,} points): {n_in:,} points in {report['n_components']:,} components in; "
             f"{n_in - n_kept:,} points in {n_dropped_components:,} components dropped, {n_kept:,} points kept (largest component "
             f"{report['largest_component']:,} points)")
    new_pts = (xyz, rgb, err)
    if on_gpu:
        clock = result._clock

        def loader(p=new_pts, clk=clock):
            if hasattr(clk, "stage"):
                with clk.stage("d2h"):
                    return tuple(t.cpu().numpy() for t in p)
            return tuple(t.cpu().numpy() for t in p)
        arrays = (None, None, None)
    else:
        loader, arrays = None, tuple(t.numpy() for t in new_pts)
    return PipelineResult(xyz=arrays[0], rgb=arrays[1], err=arrays[2], elapsed_seconds=result.elapsed_seconds, pairs_processed=result.pairs_processed,
                          pairs_matched=result.pairs_matched, points_per_reference=kept, device_points=new_pts, streamed_path=None,
                          clock=result._clock, loader=loader, device_normals=normals, match_grid=result.match_grid)


def footprint_rows(camera_records, refs_local, match_grid) -> np.ndarray:
    """(n_refs, 5) f64, one row per reference as lfd_thin_footprint takes it: the third row of its world-to-camera [R | t] and the tangent of one
    cell of the matcher's grid (``match_grid`` = (H, W)), max(width / (fx W), height / (fy H))."""
    grid_h, grid_w = int(match_grid[0]), int(match_grid[1])
    rows = np.zeros((len(refs_local), 5), np.float64)
    for i, r in enumerate(refs_local):
        cam = camera_records[int(r)]
        K, R, t = (np.asarray(a, np.float64) for a in (cam.K, cam.R, cam.t))
        rows[i, :3] = R.reshape(3, 3)[2]
        rows[i, 3] = t.reshape(3)[2]
        rows[i, 4] = max(float(cam.width) / (K.reshape(3, 3)[0, 0] * grid_w), float(cam.height) / (K.reshape(3, 3)[1, 1] * grid_h))
    return rows


def _apply_footprint_thin(result, config: DensePipelineConfig, camera_records, refs_local, progress_callback=None):
    """Footprint-adaptive thinning of the finished cloud (lfd_thin_footprint), where the points are, behind the consensus and
    free-space filters and the depth maps, in front of the point cap, the fusion, the Gaussian output and the voxel filter.  Entry i of
    ``result.points_per_reference`` is reference ``refs_local[i]``, whose camera is ``camera_records[refs_local[i]]``.  Returns the result with
    the kept points (input order, same bits), their normals and their per-reference counts in place of the cloud.  Off
    (experimental['footprint_thin_cells'] = 0): the result itself, nothing runs."""
    thin_cells = float(config.exp("footprint_thin_cells"))
    if thin_cells <= 0.0 or result.streamed_path is not None:
        return result
    from .core import hip_backend as hb
    from .core.sinks import PipelineResult
    import torch
    if result.match_grid is None:
        raise RuntimeError("experimental['footprint_thin_cells'] sizes its cells by the matcher's grid, and this result does not record one")
    pts = result.device_points
    if pts is None:
        pts = tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in (result.xyz, result.rgb, result.err))
    counts = np.asarray(result.points_per_reference, np.int64)
    n_in = int(pts[0].shape[0])
    if int(counts.sum()) != n_in or counts.size != len(refs_local):
        raise RuntimeError(f"experimental['footprint_thin_cells'] needs the whole cloud with its per-reference counts: this result holds {n_in:,} "
                           f"points, the counts of {counts.size} of {len(refs_local)} references add up to {int(counts.sum()):,} (a rank of a "
                           "gather_to_root run that is not the root)")
    rows = footprint_rows(camera_records, refs_local, result.match_grid)
    if progress_callback:
        progress_callback(94.0, "Thinning by camera footprint...")
    on_gpu = bool(pts[0].is_cuda)
    dens = hb.HipDensifier(pts[0].device) if on_gpu else hb.HostDensifier(int(config.exp("host_threads")))
    try:
        keep, kept = dens.thin_footprint(pts[0], pts[2], counts, rows, thin_cells)
        points_per_level, cells_per_level, _side = dens.thin_stats
    except hb.HipBackendError as exc:
        raise RuntimeError(f"experimental['footprint_thin_cells']: {exc}") from exc
    finally:
        dens.close()
    new_pts = tuple(t[keep] for t in pts)               # (the index of the device route is a device tensor: it never leaves the GPU)
    normals = _take_rows(result.device_normals, keep)
    levels = ", ".join(f"level {l}: {int(points_per_level[l]):,} points in {int(cells_per_level[l]):,} cells" for l in np.flatnonzero(points_per_level))
    log.info(f"Footprint thinning ({thin_cells:g} cells): {n_in:,} points in, {int(keep.shape[0]):,} kept; {levels}")
    if on_gpu:
        clock = result._clock

        def loader(p=new_pts, clk=clock):
            if hasattr(clk, "stage"):
                with clk.stage("d2h"):
                    return tuple(t.cpu().numpy() for t in p)
            return tuple(t.cpu().numpy() for t in p)
        arrays = (None, None, None)
    else:
        loader, arrays = None, tuple(t.numpy() for t in new_pts)
    return PipelineResult(xyz=arrays[0], rgb=arrays[1], err=arrays[2], elapsed_seconds=result.elapsed_seconds, pairs_processed=result.pairs_processed,
                          pairs_matched=result.pairs_matched, points_per_reference=kept, device_points=new_pts, streamed_path=None,
                          clock=result._clock, loader=loader, device_normals=normals, match_grid=result.match_grid)


class OrientedFusionRefused(RuntimeError):
    """experimental['fuse_voxel_size']: the library refused the cloud (a non-finite coordinate, a voxel key range beyond 63 bits)."""


def _apply_oriented_fusion(config: DensePipelineConfig, xyz, normals, rgb, progress_callback=None):
    """Oriented voxel fusion of the capped cloud (lfd_fuse_oriented), where the points are: device tensors through the device
    call, host arrays (``backend='host'``) through the twin.  Returns ``(xyz, normals, rgb)`` of the fused rows, of the kind that came in
    (tensors on the device, NumPy arrays on the host).  The caller has checked that experimental['fuse_voxel_size'] is > 0."""
    from .core import hip_backend as hb
    import torch
    h = float(config.exp("fuse_voxel_size"))
    if normals is None:
        raise RuntimeError("experimental['fuse_voxel_size'] needs the normals of experimental['estimate_normals']; this result carries none")
    on_gpu = isinstance(xyz, torch.Tensor) and bool(xyz.is_cuda)
    as_tensor = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))      # noqa: E731
    t = tuple(as_tensor(a) for a in (xyz, normals, rgb))
    if not on_gpu:
        t = tuple(a.cpu() for a in t)
    if progress_callback:
        progress_callback(94.0, "Fusing oriented points...")
    n_in = int(t[0].shape[0])
    dens = hb.HipDensifier(t[0].device) if on_gpu else hb.HostDensifier(int(config.exp("host_threads")))
    try:
        rows = dens.fuse_oriented(t[0], t[1], t[2], h)
        n_vox = int(dens.fuse_voxels)
    except hb.FuseInputRefused as exc:
        raise OrientedFusionRefused(f"experimental['fuse_voxel_size'] = {h:g} cannot be applied to this cloud: {exc}") from exc
    finally:
        dens.close()
    n_rows = int(rows[0].shape[0])
    log.info(f"Oriented fusion ({h:.4f}): {n_in:,} points in, {n_rows:,} rows out, {n_vox:,} voxels, {n_rows - n_vox:,} two-sided")
    return rows if on_gpu else tuple(r.numpy() for r in rows)


class GaussianInitRefused(RuntimeError):
    """experimental['gaussian_init']: the library refused the cloud (fewer than four points, a non-finite coordinate, a cell key range beyond the
    grid's limits).  No file of another format is written in its place."""


def _write_gaussians(config: DensePipelineConfig, path: str, xyz, normals, rgb, clock=None, progress_callback=None) -> None:
    """The output file of experimental['gaussian_init'] in place of the 27-byte point file: the exact 3-nearest-neighbour scale
    (lfd_knn_dist2) and the 68-byte records (lfd_pack_gaussians) where the final cloud is - device tensors through the device calls, host arrays
    (``backend='host'``) through the twin -, so that only the file payload crosses PCIe."""
    from .core import hip_backend as hb
    from .core.stages import NULL_CLOCK
    from .core.writers import write_gaussian_ply_packed
    import torch
    if normals is None:
        raise RuntimeError("experimental['gaussian_init'] needs the normals of experimental['estimate_normals']; this result carries none")
    if not _is_writer_rank():
        return
    clock = clock if clock is not None else NULL_CLOCK
    on_gpu = isinstance(xyz, torch.Tensor) and bool(xyz.is_cuda)
    as_tensor = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))      # noqa: E731
    t = tuple(as_tensor(a) for a in (xyz, normals, rgb))
    if not on_gpu:
        t = tuple(a.cpu() for a in t)
    if progress_callback:
        progress_callback(96.0, "Initialising Gaussians...")
    n = int(t[0].shape[0])
    dens = hb.HipDensifier(t[0].device) if on_gpu else hb.HostDensifier(int(config.exp("host_threads")))
    try:
        try:
            dist2 = dens.knn_dist2(t[0])
        except hb.KnnInputRefused as exc:
            raise GaussianInitRefused(f"experimental['gaussian_init'] cannot be applied to this cloud of {n:,} points: {exc}") from exc
        h, cells, fullest, brute = dens.knn_stats
        with clock.stage("d2h"):                # the file payload - 68 bytes per point - is what crosses PCIe
            body = dens.pack_gaussians(t[0], t[1], t[2], dist2, opacity=float(config.exp("gaussian_opacity")),
                                       flatten=float(config.exp("gaussian_flatten")), max_scale=float(config.exp("gaussian_max_scale")))
            body = body.cpu().numpy().tobytes()
    finally:
        dens.close()
    log.info(f"Gaussian initialisation: {n:,} points, cell size {h:.6g}, {cells:,} occupied cells, fullest cell {fullest:,}, {brute:,} points by brute force")
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with clock.stage("write", sync=False):
        write_gaussian_ply_packed(path, n, body)


DEPTH_MAP_BYTES = 256 << 20      # _write_depth_maps renders as many cameras per call as keep the maps of a call below this


def _write_depth_maps(result, config: DensePipelineConfig, camera_records, progress_callback=None) -> None:
    """Per-camera depth and normal maps of the finished cloud (lfd_render_depth), rendered where the points are, behind the
    consensus and free-space filters and in front of the point cap, the fusion and the voxel filter.  EVERY record of ``camera_records`` gets
    ``<stem of its image file>.npy`` - f32 (ph, pw), depth along its z axis in scene units, 0 = no data - and, when the run estimated normals,
    ``<stem>_normal.npy`` - f32 (ph, pw, 3), world frame, 0 0 0 = no data - in experimental['depth_maps_dir'] (relative: to the output file's
    directory), next to ``depth_maps.json``.  A side output: ``result`` is not changed.  Off (''): nothing runs."""
    maps_dir = str(config.exp("depth_maps_dir"))
    if maps_dir == "" or not _is_writer_rank():
        return
    import json
    from .core import hip_backend as hb
    import torch
    if result.streamed_path is not None:
        raise RuntimeError("experimental['depth_maps_dir'] renders the cloud held as arrays: this result was streamed to its file")
    if not os.path.isabs(maps_dir):
        maps_dir = os.path.join(os.path.dirname(os.path.abspath(config.output_path)), maps_dir)
    stems = {}                                       # stem -> its record, in the order of the records
    for rec in camera_records:
        stem = os.path.splitext(os.path.basename(str(rec.image_path)))[0]
        if stem == "" or stem in stems:
            raise RuntimeError(f"experimental['depth_maps_dir'] names a camera's maps after its image file: {stems.get(stem, rec).image_path!r} and "
                               f"{rec.image_path!r} both give {stem!r}")
        stems[stem] = rec
    xyz = result.device_points[0] if result.device_points is not None else torch.from_numpy(np.ascontiguousarray(result.xyz, np.float32))
    normals = result.device_normals                  # experimental['estimate_normals']: on the device the points are on
    cam_P = np.stack([np.asarray(c.P, np.float64).astype(np.float32).reshape(12) for c in camera_records])
    cam_wh = np.array([[int(c.width), int(c.height)] for c in camera_records], np.int32)
    plane = depth_map_plane(config, camera_records[0].width, camera_records[0].height, result.match_grid)
    r, R, tol = int(config.exp("depth_map_splat_cells")), int(config.exp("depth_map_window_cells")), float(config.exp("depth_map_tol_rel"))
    if progress_callback:
        progress_callback(94.0, "Rendering depth maps...")
    os.makedirs(maps_dir, exist_ok=True)
    per_call = max(1, DEPTH_MAP_BYTES // (plane[0] * plane[1] * (16 if normals is not None else 4)))
    dens = hb.HipDensifier(xyz.device) if xyz.is_cuda else hb.HostDensifier(int(config.exp("host_threads")))
    names, entries = list(stems), []
    try:
        for c0 in range(0, len(camera_records), per_call):
            c1 = min(len(camera_records), c0 + per_call)
            depth, _, normal = dens.render_depth(xyz, normals, cam_P[c0:c1], cam_wh[c0:c1], plane, r, R, tol)
            depth = depth.cpu().numpy()
            normal = None if normal is None else normal.cpu().numpy()
            for c in range(c0, c1):
                rec, stem = camera_records[c], names[c]
                d = depth[c - c0]
                np.save(os.path.join(maps_dir, stem + ".npy"), d)
                if normal is not None:
                    np.save(os.path.join(maps_dir, stem + "_normal.npy"), normal[c - c0])
                valid = d > 0
                entries.append({"image": os.path.basename(str(rec.image_path)), "depth": stem + ".npy",
                                "normal": stem + "_normal.npy" if normal is not None else None, "width": int(rec.width), "height": int(rec.height),
                                "valid_cells": int(valid.sum()), "depth_min": float(d[valid].min()) if valid.any() else None,
                                "depth_max": float(d[valid].max()) if valid.any() else None})
    except hb.HipBackendError as exc:
        raise RuntimeError(f"experimental['depth_maps_dir']: {exc}") from exc
    finally:
        dens.close()
    with open(os.path.join(maps_dir, "depth_maps.json"), "w") as f:
        json.dump({"plane": {"width": int(plane[0]), "height": int(plane[1])}, "splat_cells": r, "window_cells": R, "tol_rel": tol,
                   "points": int(xyz.shape[0]), "normals": normals is not None, "no_data": 0.0, "cameras": entries}, f, indent=1)
    log.info(f"Depth maps ({plane[0]} x {plane[1]} cells, splat {r}, window {R}, tolerance {tol:g}): {len(entries)} cameras -> {maps_dir}")


def _is_writer_rank() -> bool:
    """True unless this process is a non-zero rank of an initialised torch.distributed job."""
    try:
        import torch.distributed as dist
        return not (dist.is_available() and dist.is_initialized()) or dist.get_rank() == 0
    except Exception:
        return True


def _write_output(path: str, xyz, rgb, err, device_points=None, clock=None, as_ply: Optional[bool] = None, normals=None) -> None:
    """``.ply`` -> upstream's PLY, anything else -> upstream's points3D.bin (densify.py:129-135); ``as_ply`` overrides the suffix.  When
    the points are still on the GPU the records are quantised and packed there (lfd_pack_*) and only
    the final bytes are copied to the host; the files are byte-identical either way.  ``normals`` (experimental['estimate_normals'], a PLY
    only): one per point, where the points are - the vertices then are the 27-byte x y z nx ny nz r g b."""
    if not _is_writer_rank():        # sharded run: every rank holds the gathered cloud, rank 0 alone writes the file
        return
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    as_ply = path.lower().endswith(".ply") if as_ply is None else bool(as_ply)
    if device_points is not None and device_points[0].is_cuda and int(device_points[0].shape[0]) == int(xyz.shape[0]):
        from .core import hip_backend as hb
        from .core.writers import write_ply_packed, write_points3D_bin_packed
        from .core.stages import NULL_CLOCK
        clock = clock if clock is not None else NULL_CLOCK
        dens = hb.HipDensifier(device_points[0].device)
        try:
            n = int(xyz.shape[0])
            with clock.stage("d2h"):            # the file payload - 15 / 43 bytes per point - is what crosses PCIe
                if normals is not None:
                    packed = dens.pack_ply_normals(device_points[0], normals, device_points[1])
                else:
                    packed = dens.pack_ply(device_points[0], device_points[1]) if as_ply else dens.pack_points3d(*device_points)
                body = packed.cpu().numpy().tobytes()
            with clock.stage("write", sync=False):
                if normals is not None:
                    write_ply_packed(path, n, body, normals=True)
                else:
                    (write_ply_packed if as_ply else write_points3D_bin_packed)(path, n, body)
        finally:
            dens.close()
        return
    rgb8 = to_uint8_rgb(rgb)
    if normals is not None:
        write_ply(path, xyz, rgb8, normals.cpu().numpy() if hasattr(normals, "cpu") else normals)
    elif as_ply:
        write_ply(path, xyz, rgb8)
    else:
        write_points3D_bin(path, xyz, rgb8, err)


def _write_final(shell, path: str, xyz, rgb, err, device_points=None, normals=None, **kw) -> None:
    """``_write_output`` with the far-field shell (experimental['far_shell'], ``FarShell`` or None) placed around the cloud as it is written, in
    front of packing: 'file' writes the shell beside an untouched main file, 'merge' appends its records behind the cloud's."""
    if shell is None:
        _write_output(path, xyz, rgb, err, device_points, normals=normals, **kw)
        return
    import torch
    on_dev = device_points is not None and device_points[0].is_cuda and int(device_points[0].shape[0]) == int(xyz.shape[0])
    sx, srgb, snrm = shell.emit(device_points[0] if on_dev else xyz, normals is not None)
    if shell.mode == "file":
        _write_output(path, xyz, rgb, err, device_points, normals=normals, **kw)
        _write_shell_file(shell.shell_path, sx, srgb, snrm, kw.get("clock"))
        return
    if on_dev:
        dev = device_points[0].device
        device_points = (torch.cat([device_points[0], sx.to(dev)]), torch.cat([device_points[1], srgb.to(dev)]))
        normals = torch.cat([normals.to(dev), snrm.to(dev)]) if normals is not None else None
        xyz = np.empty((int(device_points[0].shape[0]), 0), np.float32)
    else:
        host = lambda a: a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)      # noqa: E731
        xyz, rgb = np.concatenate([host(xyz), host(sx)]), np.concatenate([host(rgb), host(srgb)])
        normals = np.concatenate([host(normals), host(snrm)]) if normals is not None else None
        err, device_points = None, None
    _write_output(path, xyz, rgb, err, device_points, normals=normals, **kw)


def _cap_device_points(device_points, keep):
    """The GPU copy under the cap's index (``_cap_keep``)."""
    if device_points is None or keep is None:
        return device_points
    return tuple(_take_rows(t, keep) for t in device_points)


def _was_cancelled(cb) -> bool:
    if cb is None:
        return False
    try:
        return bool(cb())
    except Exception as exc:
        log.warn(f"Cancellation callback failed: {exc}")
        return False


# ---- entry points ------------------------------------------------------------------------------------
def plan_scene(args):
    """What upstream's CLI derives from the scene before the pipeline starts (densify.py:154-165 there): the camera records, the reference
    views (greedy visibility cover of the sparse points, k-centres on the poses if that fails) and the neighbour table.
    Returns ``(records, refs_local, nn_table, sparse_dir)``."""
    scene_root = os.path.abspath(args.scene_root)
    sparse_dir = os.path.join(scene_root, "sparse", "0")
    images_dir = image_dir(scene_root, args.images_subdir)
    rec, cams, imgs = load_reconstruction(sparse_dir)
    records, img_ids = camera_records_from_colmap(cams, imgs, images_dir)
    flat = _flat_pose_stack(records)
    want = max(1, _num_refs(args.num_refs, len(img_ids)))
    try:
        by_id = {iid: i for i, iid in enumerate(img_ids)}
        refs_local = [by_id[r] for r in select_cameras_by_visibility(rec, want) if r in by_id]
    except Exception as exc:
        log.warn(f"Visibility-based selection failed: {exc}")
        refs_local = select_cameras_kcenters(flat, want)
    nn_table = nearest_neighbors(flat, max(1, args.nns_per_ref))
    return records, refs_local, nn_table, sparse_dir


def dense_init(args, progress_callback: Optional[Callable[[float, str], None]] = None, debug_state=None,
               cancel_requested: Optional[Callable[[], bool]] = None, **pipeline_kwargs) -> int:
    """CLI / COLMAP entry point.  Returns 0 on success, 2 when cancelled; raises on error.  ``pipeline_kwargs``: the injection points of
    ``run_dense_pipeline`` (a warm matcher, a stage clock), as ``dense_init_from_lfs`` takes them."""
    records, refs_local, nn_table, sparse_dir = plan_scene(args)
    config = DensePipelineConfig(
        output_path=os.path.join(sparse_dir, args.out_name), roma_setting=args.roma_setting, num_refs=args.num_refs,
        nns_per_ref=args.nns_per_ref, matches_per_ref=args.matches_per_ref, certainty_thresh=args.certainty_thresh,
        reproj_thresh=args.reproj_thresh, sampson_thresh=args.sampson_thresh, min_parallax_deg=args.min_parallax_deg,
        max_points=args.max_points, no_filter=args.no_filter, seed=args.seed, viz_interval=0,
        prefetch_packages=args.prefetch_packages, pack_workers=args.pack_workers,
        triangulation_mode=getattr(args, "triangulation_mode", "sampled"),
        refs_per_launch=getattr(args, "refs_per_launch", 0), backend=getattr(args, "backend", "device"),
        stream_output=bool(getattr(args, "stream_output", False)), device_image_prep=bool(getattr(args, "device_image_prep", False)),
        experimental=_experimental_from_args(args))
    _check_audit_maps(config, records)
    records = _load_pose_corrections(config, records)      # (experimental['pose_corrections']: the poses of an earlier run's poses.json)
    try:
        result = run_dense_pipeline(records, refs_local, nn_table, config, progress_callback=progress_callback,
                                    on_sequential_viz=None, debug_state=debug_state, cancel_requested=cancel_requested, **pipeline_kwargs)
    except PipelineCancelled:
        if progress_callback:
            progress_callback(0.0, "Cancelled")
        return 2
    if _was_cancelled(cancel_requested):
        if progress_callback:
            progress_callback(0.0, "Cancelled")
        return 2
    _write_audit(result, config, records)               # (experimental['epipolar_audit']: a side output about the poses; moves nothing)
    _write_poses(result, config)                        # (experimental['pose_refine']: likewise)
    shell = _far_shell_of(result, config, records)      # (experimental['far_shell']: placed around the final cloud, where it is written)
    result = _apply_gain_compensation(result, config, records, refs_local, progress_callback)      # (while the counts are still the loop's)
    result = _apply_consensus_filter(result, config, progress_callback)      # (in front of the point cap: it has to see the whole cloud)
    result = _apply_freespace_filter(result, config, records, refs_local, progress_callback)      # (behind it: what it removed cannot "see through" a surface)
    result = _apply_component_filter(result, config, progress_callback)      # (behind the filters that need a second witness: what is left and isolated)
    _write_depth_maps(result, config, records, progress_callback)      # (a side output of the densest filtered cloud, in front of cap, fusion and voxel filter)
    result = _apply_footprint_thin(result, config, records, refs_local, progress_callback)      # (in front of cap, fusion, Gaussian output and voxel filter)
    if progress_callback:
        progress_callback(95.0, "Writing output...")
    if result.streamed_path == config.output_path:      # config.stream_output: the file is already complete (and no cap applies to it)
        n_points = result.n_points
    else:
        n_points = _finish_on_device(result, config.output_path, args.max_points, args.seed, clock=pipeline_kwargs.get("stage_clock"), config=config,
                                     progress_callback=progress_callback, shell=shell)
        if n_points is None:
            keep = _cap_keep(result.xyz, result.err, args.max_points, args.seed, progress_callback=progress_callback, **_cap_args(config))
            normals = _take_rows(result.normals, keep)
            xyz, rgb, err = (_take_rows(a, keep) for a in (result.xyz, result.rgb, result.err))
            if float(config.exp("fuse_voxel_size")) > 0.0:
                xyz, normals, rgb = _apply_oriented_fusion(config, xyz, normals, rgb, progress_callback)
                err = None
            if bool(config.exp("gaussian_init")):
                _write_gaussians(config, config.output_path, xyz, normals, rgb, clock=pipeline_kwargs.get("stage_clock"), progress_callback=progress_callback)
                if shell is not None:
                    shell.write_file(xyz, normals is not None)
            else:
                _write_final(shell, config.output_path, xyz, rgb, err, None, normals=normals)
            n_points = int(xyz.shape[0])
    log.info(f"Dense reconstruction finished: {n_points:,} points -> {config.output_path}")
    if progress_callback:
        progress_callback(100.0, f"Done! {n_points:,} points")
    return 0


def dense_init_from_lfs(camera_nodes, config: DensePipelineConfig,
                        progress_callback: Optional[Callable[[float, str], None]] = None,
                        on_sequential_viz: Optional[Callable[[str], None]] = None, debug_state=None,
                        cancel_requested: Optional[Callable[[], bool]] = None, **pipeline_kwargs
                        ) -> Tuple[int, Optional[str]]:
    """GUI entry point.  Returns ``(0, output_path)``, ``(1, message)`` or ``(2, "Cancelled")``."""
    if progress_callback:
        progress_callback(2.0, "Extracting camera data from scene...")
    records = extract_cameras_from_lfs(camera_nodes)
    if not config.use_masks:
        for r in records:
            r.mask_path = None
    if len(records) < 2:
        return 1, "Need at least 2 cameras for dense initialization"
    flat = _flat_pose_stack(records)
    refs_local = select_cameras_kcenters(flat, max(1, _num_refs(config.num_refs, len(records))))
    nns = _effective_neighbor_count(config.nns_per_ref, len(records))
    if nns < 1:
        return 1, "Need at least 2 cameras for dense initialization"
    if nns != int(config.nns_per_ref):
        log.info(f"Clamping neighbors per reference from {config.nns_per_ref} to {nns} for {len(records)} ROI cameras")
    nn_table = nearest_neighbors(flat, nns)
    log.info(f"Prepared {len(records)} cameras (refs={len(refs_local)})")
    try:
        records = _load_pose_corrections(config, records)      # (experimental['pose_corrections']: the poses of an earlier run's poses.json)
    except (OSError, ValueError) as exc:
        return 1, str(exc)
    try:
        _check_audit_maps(config, records)
        result = run_dense_pipeline(records, refs_local, nn_table, config, progress_callback=progress_callback,
                                    on_sequential_viz=on_sequential_viz, debug_state=debug_state,
                                    cancel_requested=cancel_requested, **pipeline_kwargs)
    except PipelineCancelled:
        return 2, "Cancelled"
    except RuntimeError as exc:
        return 1, str(exc)
    if _was_cancelled(cancel_requested):
        return 2, "Cancelled"
    try:
        _write_audit(result, config, records)               # (experimental['epipolar_audit']: a side output about the poses; moves nothing)
        _write_poses(result, config)                        # (experimental['pose_refine']: likewise)
        shell = _far_shell_of(result, config, records)      # (experimental['far_shell']: placed around the final cloud, where it is written)
        result = _apply_gain_compensation(result, config, records, refs_local, progress_callback)      # (while the counts are still the loop's)
        result = _apply_consensus_filter(result, config, progress_callback)  # (in front of the point cap and the voxel filter: it has to see the whole cloud)
        result = _apply_freespace_filter(result, config, records, refs_local, progress_callback)   # (behind it, in front of cap and voxel filter)
        result = _apply_component_filter(result, config, progress_callback)   # (behind the filters that need a second witness)
        _write_depth_maps(result, config, records, progress_callback)      # (a side output of that cloud)
        result = _apply_footprint_thin(result, config, records, refs_local, progress_callback)   # (in front of cap, fusion, Gaussian output and voxel filter)
    except RuntimeError as exc:
        return 1, str(exc)
    if result.streamed_path == config.output_path:      # config.stream_output: the PLY is complete; neither a cap nor a voxel filter applies to it
        if progress_callback:
            progress_callback(95.0, "Writing output PLY...")
        log.info(f"Dense point cloud saved to {config.output_path} ({result.n_points:,} points)")
        if progress_callback:
            progress_callback(100.0, f"Done! {result.n_points:,} points")
        return 0, config.output_path
    if config.voxel_size <= 0.0 and config.output_path.lower().endswith(".ply") and result.device_points is not None and result.device_points[0].is_cuda:
        # nothing has to see the cloud on the host: the cap is applied and the file payload packed where the points are
        if progress_callback:
            progress_callback(95.0, "Writing output PLY...")
        try:
            n_written = _finish_on_device(result, config.output_path, config.max_points, config.seed, clock=pipeline_kwargs.get("stage_clock"),
                                          config=config, progress_callback=progress_callback, shell=shell)
        except (SpatialCapRefused, OrientedFusionRefused, GaussianInitRefused) as exc:
            return 1, str(exc)
        log.info(f"Dense point cloud saved to {config.output_path} ({n_written:,} points)")
        if progress_callback:
            progress_callback(100.0, f"Done! {n_written:,} points")
        return 0, config.output_path
    announced = False
    if config.voxel_size > 0.0 and result.device_points is not None and result.device_points[0].is_cuda:
        # the distance filter where the points are: only the PLY payload crosses PCIe (the host route below is taken if the library refuses the cloud)
        if progress_callback:
            progress_callback(93.0, "Applying distance filter...")
        announced = True
        try:
            keep = _cap_keep(result.device_points[0], result.device_points[2], config.max_points, config.seed, progress_callback=progress_callback,
                             **_cap_args(config))
        except SpatialCapRefused as exc:
            return 1, str(exc)
        voxels = _voxel_filter_on_device(_cap_device_points(result.device_points, keep), config.voxel_size)
        if voxels is not None:
            n_vox = int(voxels[0].shape[0])
            log.info(f"Distance filter ({config.voxel_size:.4f}): {n_vox:,} points remaining")
            if progress_callback:
                progress_callback(95.0, "Writing output PLY...")
            # upstream always writes a PLY here, whatever the name
            _write_final(shell, config.output_path, np.empty((n_vox, 0), np.float32), None, None, voxels, clock=pipeline_kwargs.get("stage_clock"),
                         as_ply=True)
            log.info(f"Dense point cloud saved to {config.output_path} ({n_vox:,} points)")
            if progress_callback:
                progress_callback(100.0, f"Done! {n_vox:,} points")
            return 0, config.output_path
    on_gpu = result.device_points is not None and result.device_points[0].is_cuda
    try:                                                # (one choice, made where the cloud is, for the host arrays and the GPU copy alike)
        keep = _cap_keep(result.device_points[0] if on_gpu else result.xyz, result.device_points[2] if on_gpu else result.err, config.max_points,
                         config.seed, progress_callback=progress_callback, **_cap_args(config))
    except SpatialCapRefused as exc:
        return 1, str(exc)
    normals = _take_rows(result.normals, keep)          # (None without experimental['estimate_normals'])
    xyz, rgb, err = (_take_rows(a, keep) for a in (result.xyz, result.rgb, result.err))
    dev_pts = _cap_device_points(result.device_points, keep)
    if float(config.exp("fuse_voxel_size")) > 0.0:         # (needs estimate_normals, which rules the voxel filter out)
        try:
            xyz, normals, rgb = _apply_oriented_fusion(config, xyz, normals, rgb, progress_callback)
        except OrientedFusionRefused as exc:
            return 1, str(exc)
        err = None
    if config.voxel_size > 0.0:
        if progress_callback and not announced:
            progress_callback(93.0, "Applying distance filter...")
        xyz, rgb = _voxel_downsample(xyz, rgb, config.voxel_size)
        dev_pts = None                                   # the voxel average lives on the host
        log.info(f"Distance filter ({config.voxel_size:.4f}): {xyz.shape[0]:,} points remaining")
    if progress_callback:
        progress_callback(95.0, "Writing output PLY...")
    out_path = config.output_path if config.output_path.lower().endswith(".ply") else config.output_path + ".ply"
    if out_path != config.output_path:                  # upstream always writes a PLY here, whatever the name
        d = os.path.dirname(config.output_path)
        if d:
            os.makedirs(d, exist_ok=True)
        if _is_writer_rank():
            write_ply(config.output_path, xyz, to_uint8_rgb(rgb))
        if shell is not None:                           # ('merge' needs a .ply name: this is 'file')
            shell.write_file(xyz, False)
    elif bool(config.exp("gaussian_init")):             # (needs estimate_normals, which makes output_path a .ply)
        try:
            _write_gaussians(config, config.output_path, xyz, normals, rgb, clock=pipeline_kwargs.get("stage_clock"), progress_callback=progress_callback)
        except GaussianInitRefused as exc:
            return 1, str(exc)
        if shell is not None:
            shell.write_file(xyz, normals is not None)
    else:
        _write_final(shell, config.output_path, xyz, rgb, err, dev_pts if normals is None else None, normals=normals)
    log.info(f"Dense point cloud saved to {config.output_path} ({xyz.shape[0]:,} points)")
    if progress_callback:
        progress_callback(100.0, f"Done! {xyz.shape[0]:,} points")
    return 0, config.output_path


def _experimental_from_args(args) -> dict:
    """The experimental knobs the command line reaches; a flag left at its default adds nothing."""
    exp = {}
    if float(getattr(args, "cycle_thresh_px", 0.0)) != 0.0:
        exp["cycle_thresh_px"] = float(args.cycle_thresh_px)
    if int(getattr(args, "min_support_views", 0)) != 0:
        exp["min_support_views"] = int(args.min_support_views)
    if float(getattr(args, "support_thresh_px", 0.0)) != 0.0:
        exp["support_thresh_px"] = float(args.support_thresh_px)
    if bool(getattr(args, "multiview_refine", False)):
        exp["multiview_refine"] = True
    if bool(getattr(args, "precision_weighted_refine", False)):
        exp["precision_weighted_refine"] = True
    if float(getattr(args, "max_depth_sigma_rel", 0.0)) != 0.0:
        exp["max_depth_sigma_rel"] = float(args.max_depth_sigma_rel)
    if float(getattr(args, "match_sigma_px", 0.0)) != 0.0:
        exp["match_sigma_px"] = float(args.match_sigma_px)
    if int(getattr(args, "min_consensus_refs", 0)) != 0:
        exp["min_consensus_refs"] = int(args.min_consensus_refs)
    if float(getattr(args, "consensus_radius", 0.0)) != 0.0:
        exp["consensus_radius"] = float(args.consensus_radius)
    if int(getattr(args, "min_component_points", 0)) != 0:
        exp["min_component_points"] = int(args.min_component_points)
    if float(getattr(args, "component_radius", 0.0)) != 0.0:
        exp["component_radius"] = float(args.component_radius)
    if int(getattr(args, "min_freespace_violations", 0)) != 0:
        exp["min_freespace_violations"] = int(args.min_freespace_violations)
    if getattr(args, "freespace_depth_tol_rel", None) is not None:
        exp["freespace_depth_tol_rel"] = float(args.freespace_depth_tol_rel)
    if int(getattr(args, "freespace_plane_cells", 0)) != 0:
        exp["freespace_plane_cells"] = int(args.freespace_plane_cells)
    if float(getattr(args, "footprint_thin_cells", 0.0) or 0.0) != 0.0:
        exp["footprint_thin_cells"] = float(args.footprint_thin_cells)
    if str(getattr(args, "depth_maps_dir", "") or "") != "":
        exp["depth_maps_dir"] = str(args.depth_maps_dir)
    for key, cast in (("depth_map_cells", int), ("depth_map_splat_cells", int), ("depth_map_window_cells", int), ("depth_map_tol_rel", float)):
        if getattr(args, key, None) is not None:
            exp[key] = cast(getattr(args, key))
    if bool(getattr(args, "undistort_images", False)):
        exp["undistort_images"] = True
    if bool(getattr(args, "fused_refiner_blocks", False)):
        exp["fused_refiner_blocks"] = True
    if bool(getattr(args, "fused_refiner_head", False)):
        exp["fused_refiner_head"] = True
    if str(getattr(args, "multiview_colour", None) or "off") != "off":
        exp["multiview_colour"] = str(args.multiview_colour)
    if str(getattr(args, "gain_compensation", None) or "off") != "off":
        exp["gain_compensation"] = str(args.gain_compensation)
    if str(getattr(args, "epipolar_audit", None) or "off") != "off":
        exp["epipolar_audit"] = str(args.epipolar_audit)
    for key in ("audit_certainty", "audit_min_samples", "audit_warn_px"):
        if getattr(args, key, None) is not None:
            exp[key] = getattr(args, key)
    if str(getattr(args, "audit_maps_dir", "") or "") != "":
        exp["audit_maps_dir"] = str(args.audit_maps_dir)
    if str(getattr(args, "pose_refine", None) or "off") != "off":
        exp["pose_refine"] = str(args.pose_refine)
    for key in ("pose_certainty", "pose_inlier_px", "pose_min_samples"):
        if getattr(args, key, None) is not None:
            exp[key] = getattr(args, key)
    if str(getattr(args, "pose_corrections", "") or "") != "":
        exp["pose_corrections"] = str(args.pose_corrections)
    if str(getattr(args, "far_shell", None) or "off") != "off":
        exp["far_shell"] = str(args.far_shell)
    for key in ("far_thresh_px", "far_certainty", "far_min_views", "far_shell_cells", "far_min_samples", "far_shell_radius"):
        if getattr(args, key, None) is not None:
            exp[key] = getattr(args, key)
    if float(getattr(args, "min_photo_ncc", 0.0) or 0.0) != 0.0:
        exp["min_photo_ncc"] = float(args.min_photo_ncc)
    for key, cast in (("photo_window_cells", int), ("photo_min_texture", float)):
        if getattr(args, key, None) is not None:
            exp[key] = cast(getattr(args, key))
    if bool(getattr(args, "estimate_normals", False)):
        exp["estimate_normals"] = True
    if getattr(args, "normal_radius_cells", None) is not None:
        exp["normal_radius_cells"] = int(args.normal_radius_cells)
    if getattr(args, "normal_depth_step_rel", None) is not None:
        exp["normal_depth_step_rel"] = float(args.normal_depth_step_rel)
    if float(getattr(args, "fuse_voxel_size", 0.0)) != 0.0:
        exp["fuse_voxel_size"] = float(args.fuse_voxel_size)
    if bool(getattr(args, "gaussian_init", False)):
        exp["gaussian_init"] = True
    for key in ("gaussian_flatten", "gaussian_opacity", "gaussian_max_scale"):
        if getattr(args, key, None) is not None:
            exp[key] = float(getattr(args, key))
    if str(getattr(args, "cap_mode", "random")) != "random":
        exp["cap_mode"] = str(args.cap_mode)
    return exp


def build_argparser() -> argparse.ArgumentParser:
    """Upstream's CLI flags and defaults (densify.py:318-415) plus the two launch-shape extensions."""
    ap = argparse.ArgumentParser("Dense COLMAP initializer (RoMa v2 matching + fused HIP filter/triangulate on MI355X)")
    ap.add_argument("--scene_root", type=str, required=True, help="Path containing images*/ and sparse/0/")
    ap.add_argument("--images_subdir", type=str, default="images_2", help="Which images dir to read under scene_root")
    ap.add_argument("--out_name", type=str, default="points3D_dense.ply", help="Output filename under sparse/0/")
    ap.add_argument("--roma_setting", type=str, default="fast", choices=["precise", "high", "base", "fast", "turbo"],
                    help="RoMaV2 quality/speed setting")
    ap.add_argument("--roma_model", type=str, default="outdoor", choices=["outdoor", "indoor"],
                    help="Legacy flag for compatibility (RoMaV2 is unified)")
    ap.add_argument("--num_refs", type=float, default=0.75, help="Fraction (<=1) or count (>1) of frames to use as references")
    ap.add_argument("--nns_per_ref", type=int, default=4, help="Nearest neighbors per reference (3-5 is robust)")
    ap.add_argument("--matches_per_ref", type=int, default=12000, help="Samples per ref after aggregation")
    ap.add_argument("--certainty_thresh", type=float, default=0.20, help="Min certainty floor before selection")
    ap.add_argument("--reproj_thresh", type=float, default=1.5, help="Max reprojection error (px)")
    ap.add_argument("--sampson_thresh", type=float, default=5.0, help="Max Sampson error (px^2) pre-triangulation (<=0 disables)")
    ap.add_argument("--min_parallax_deg", type=float, default=0.5, help="Min parallax angle in degrees")
    ap.add_argument("--no_filter", action="store_true", help="Disable geometric filtering (debug only)")
    ap.add_argument("--max_points", type=int, default=0, help="Optional cap on total points (0 = unlimited)")
    ap.add_argument("--prefetch_packages", type=int, default=8, help="Reference packages prefetched ahead of the GPU")
    ap.add_argument("--pack_workers", type=int, default=4, help="Threads used to load/resize images")
    ap.add_argument("--seed", type=int, default=0, help="Random seed")
    ap.add_argument("--triangulation_mode", type=str, default="sampled", choices=list(TRIANGULATION_MODES),
                    help="sampled = upstream behaviour; dense = every grid cell through the fused kernel")
    ap.add_argument("--refs_per_launch", type=int, default=0, help="references per kernel launch (dense mode) or per fused call (sampled mode, device backend: same results, same RNG stream); 0 = automatic (16 where possible, 1 when intermediate previews are written)")
    ap.add_argument("--backend", type=str, default="device", choices=["device", "host"],
                    help="device = the HIP kernels (needs a GPU); host = the CPU twin of the C-ABI + the host sampling stage "
                         "(upstream's CPU-only configuration); never chosen automatically")
    ap.add_argument("--stream_output", action="store_true",
                    help="write the PLY while the run proceeds (15-byte records packed on the device; needs a .ply --out_name and no --max_points)")
    ap.add_argument("--device_image_prep", action="store_true", help="resize / mask the decoded images on the GPU (Pillow's arithmetic, bit for bit)")
    ap.add_argument("--cycle_thresh_px", type=float, default=0.0,
                    help="forward-backward consistency filter: drop a match whose round trip A -> B -> A misses its start by more than this many "
                         "pixels of the match image (uses RoMa's backward warp; 0 = off)")
    ap.add_argument("--min_support_views", type=int, default=0,
                    help="multi-view support filter: keep a triangulated point only if at least this many OTHER loaded neighbours of its reference "
                         "confirm it (at most nns_per_ref - 1; 0 = off)")
    ap.add_argument("--support_thresh_px", type=float, default=0.0,
                    help="... within this many pixels of the neighbour's camera image (0 = 2 * reproj_thresh)")
    ap.add_argument("--multiview_refine", action="store_true",
                    help="multi-view re-triangulation: a point that other loaded neighbours of its reference confirm (within --support_thresh_px) is "
                         "triangulated again from all the views that see it; nothing is added or dropped")
    ap.add_argument("--precision_weighted_refine", action="store_true",
                    help="... with every view weighted by the precision matrix RoMa-v2 predicts for its match instead of equally (needs "
                         "--multiview_refine)")
    ap.add_argument("--max_depth_sigma_rel", type=float, default=0.0,
                    help="depth-uncertainty gate: keep a triangulated point only if the 1-sigma bound on its relative depth error, from the views "
                         "that placed it, is at most this (e.g. 0.05; 0 = off)")
    ap.add_argument("--match_sigma_px", type=float, default=0.0,
                    help="... with this isotropic match noise in pixels of the camera image (0 = the precision matrix RoMa-v2 predicts per match)")
    ap.add_argument("--min_consensus_refs", type=int, default=0,
                    help="cross-reference consensus filter on the final cloud: keep a point only if at least this many OTHER references put a point "
                         "within --consensus_radius of it (1 .. 8; runs in front of --max_points; 0 = off)")
    ap.add_argument("--consensus_radius", type=float, default=0.0,
                    help="... within this distance in scene units (required > 0 with --min_consensus_refs)")
    ap.add_argument("--min_component_points", type=int, default=0,
                    help="connected-component filter on the final cloud: keep a point only if the connected component it belongs to - points "
                         "linked when within --component_radius of each other - has at least this many points (>= 2; runs behind "
                         "--min_consensus_refs and --min_freespace_violations, in front of --max_points; 0 = off)")
    ap.add_argument("--component_radius", type=float, default=0.0,
                    help="... linked within this distance in scene units (required > 0 with --min_component_points)")
    ap.add_argument("--min_freespace_violations", type=int, default=0,
                    help="free-space filter on the final cloud: drop a point when at least this many OTHER references triangulated a surface behind it "
                         "on the same ray (they looked through it) and more refute than confirm it (1 .. 255; runs behind --min_consensus_refs and "
                         "in front of --max_points; 0 = off)")
    ap.add_argument("--freespace_depth_tol_rel", type=float, default=None,
                    help="... with this relative depth tolerance in (0, 1) (default 0.02; not below the depth noise you accept; needs "
                         "--min_freespace_violations)")
    ap.add_argument("--freespace_plane_cells", type=int, default=0,
                    help="... on z-buffers of this many cells along the longer image side (8 .. 4096; 0 = automatic: ceil(sqrt(matches_per_ref)) in "
                         "sampled mode, the matcher's grid in dense mode; needs --min_freespace_violations)")
    ap.add_argument("--footprint_thin_cells", type=float, default=0.0,
                    help="footprint-adaptive thinning of the final cloud (DESIGN.md 4.24): at most one point per octree cell, the cell sized to this "
                         "many match-grid cells of the point's own reference camera at its depth - constant density in image space, in front of "
                         "--max_points, fusion, the Gaussian output and the voxel filter (0 = off)")
    ap.add_argument("--depth_maps_dir", type=str, default="",
                    help="write a depth map - and with --estimate_normals a normal map - of the filtered cloud for EVERY loaded camera into this "
                         "directory (relative: to the output file's), <image stem>.npy / <image stem>_normal.npy and depth_maps.json; the point file "
                         "does not change ('' = off)")
    ap.add_argument("--depth_map_cells", type=int, default=None,
                    help="... on planes of this many cells along the longer image side (8 .. 4096; 0 = automatic, as --freespace_plane_cells; needs "
                         "--depth_maps_dir)")
    ap.add_argument("--depth_map_splat_cells", type=int, default=None,
                    help="... every point drawn as a square of 2 r + 1 cells at its depth (0 .. 3, default 1; needs --depth_maps_dir)")
    ap.add_argument("--depth_map_window_cells", type=int, default=None,
                    help="... a cell dropped when something nearer lies within this many cells (0 .. 8, default 3; 0 = no test; needs --depth_maps_dir)")
    ap.add_argument("--depth_map_tol_rel", type=float, default=None,
                    help="... nearer by more than this fraction of the nearer depth, in (0, 1) (default 0.02; needs --depth_maps_dir)")
    ap.add_argument("--undistort_images", action="store_true",
                    help="resample every image (and its mask) through its COLMAP camera's distortion model (SIMPLE_RADIAL, RADIAL, OPENCV, "
                         "FULL_OPENCV) into the pinhole image of the same intrinsics before it is matched; other distorted models are refused")
    ap.add_argument("--fused_refiner_blocks", action="store_true",
                    help="run the conv blocks of RoMa-v2's refiners (depthwise 5x5, BatchNorm, ReLU, 1x1) in this package's fused HIP kernel instead "
                         "of torch's separate kernels: more accurate than the bf16 autocast sequence, not bit-identical to it")
    ap.add_argument("--fused_refiner_head", action="store_true",
                    help="run what each of RoMa-v2's refiners computes behind its conv blocks (the two 1x1 heads, the warp update, softplus and the "
                         "precision conversion) in one launch of this package's HIP kernel instead of about twenty torch kernels: within rounding "
                         "of the model's own f32 tail, not bit-identical to it")
    ap.add_argument("--multiview_colour", choices=("off", "mean", "median"), default="off",
                    help="colour every point by the mean or the median, per channel, over the views that see it (its reference, the neighbour "
                         "that made it and every other neighbour that confirms it within the support threshold) instead of the reference alone")
    ap.add_argument("--gain_compensation", choices=("off", "luma", "rgb"), default="off",
                    help="bring the whole cloud to one exposure: solve one factor per image (luma) or per image and channel (rgb) from the "
                         "colours the confirming views have at the same points, multiply every point's colour by its reference's factor and "
                         "write <out_name>.gains.json")
    ap.add_argument("--min_photo_ncc", type=float, default=0.0,
                    help="photo-consistency gate: drop a triangulated point when the normalised cross-correlation of the two image patches its "
                         "match joins is below this (e.g. 0.8; in (0, 1], 0 = off).  Refutes mismatches of a few match pixels on textured "
                         "surfaces, not sub-pixel error")
    ap.add_argument("--photo_window_cells", type=int, default=None,
                    help="... over the (2 r + 1)^2 grid cells of this radius around the point's cell (1 .. 3; default 2)")
    ap.add_argument("--photo_min_texture", type=float, default=None,
                    help="... keeping points whose patches have a standard deviation below this many 8-bit grey levels (no evidence; default 2)")
    ap.add_argument("--epipolar_audit", choices=("off", "report"), default="off",
                    help="report on the camera poses from the run's own matches: every confident match is measured against its pair's epipolar "
                         "line; <output file>.audit.json holds per-pair medians and a score per camera, and every camera whose score exceeds "
                         "--audit_warn_px is logged as suspect.  Sees only the error across the epipolar lines; moves no point")
    ap.add_argument("--audit_certainty", type=float, default=None,
                    help="... raw certainty from which a match is counted, in (0, 1] (default 0.5, a design default; needs --epipolar_audit)")
    ap.add_argument("--audit_min_samples", type=int, default=None,
                    help="... confident matches a pair needs to be judged (default 256, a design default; needs --epipolar_audit)")
    ap.add_argument("--audit_warn_px", type=float, default=None,
                    help="... a camera is suspect above this many px (default 0 = reproj_thresh; needs --epipolar_audit)")
    ap.add_argument("--audit_maps_dir", type=str, default="",
                    help="... directory (relative: to the output file's) for one <image stem>_epi.npy per reference: the smallest distance any "
                         "confident neighbour reports per cell, NaN where none (needs --epipolar_audit)")
    ap.add_argument("--pose_refine", choices=("off", "report"), default="off",
                    help="corrected camera poses from the run's own matches: one Gauss-Newton step on the epipolar error of every confident match; "
                         "<output file>.poses.json holds one corrected world-to-camera pose per camera.  Moves no point of this run: hand the file "
                         "to a second run with --pose_corrections")
    ap.add_argument("--pose_certainty", type=float, default=None,
                    help="... raw certainty from which a match is counted, in (0, 1] (default 0.5, a design default; needs --pose_refine)")
    ap.add_argument("--pose_inlier_px", type=float, default=None,
                    help="... a match further than this many px from its epipolar line is an outlier, in (0, 64] (default 8, a design default; "
                         "needs --pose_refine)")
    ap.add_argument("--pose_min_samples", type=int, default=None,
                    help="... inliers a pair needs to enter the solve (default 256, a design default; needs --pose_refine)")
    ap.add_argument("--pose_corrections", type=str, default="",
                    help="a poses.json written by an earlier run with --pose_refine: its poses replace the cameras' before the run starts")
    ap.add_argument("--far_shell", choices=("off", "file", "merge"), default="off",
                    help="points at infinity for sky and distant background: the grid cells every confident neighbour sees where the rotation-only "
                         "transfer predicts become one point per direction cell on a sphere around the cameras - in <out_name stem>_shell.ply "
                         "(file) or behind the cloud's records in the main PLY (merge); writes <out_name>.shell.json")
    ap.add_argument("--far_thresh_px", type=float, default=None,
                    help="... agreement with infinity in px of the neighbour's camera image (default 0 = reproj_thresh; needs --far_shell)")
    ap.add_argument("--far_certainty", type=float, default=None,
                    help="... raw certainty from which a neighbour is confident, in (0, 1] (default 0.5, a design default; needs --far_shell)")
    ap.add_argument("--far_min_views", type=int, default=None, help="... confident neighbours a far cell needs, 1 .. 8 (default 2; needs --far_shell)")
    ap.add_argument("--far_shell_cells", type=int, default=None,
                    help="... direction cells along a cube face's side, 8 .. 512 (default 256; needs --far_shell)")
    ap.add_argument("--far_min_samples", type=int, default=None,
                    help="... samples a direction cell needs to become a point (default 2; needs --far_shell)")
    ap.add_argument("--far_shell_radius", type=float, default=None,
                    help="... radius of the sphere in scene units (default 0 = automatic; needs --far_shell)")
    ap.add_argument("--estimate_normals", action="store_true",
                    help="give every point a unit surface normal, fitted to its winning neighbour's warp around its grid cell and oriented towards "
                         "its reference's camera: the PLY then has x y z nx ny nz red green blue vertices (needs a .ply --out_name)")
    ap.add_argument("--normal_radius_cells", type=int, default=None,
                    help="... over the (2 r + 1)^2 window of this radius in grid cells (1 .. 4; default 3; needs --estimate_normals)")
    ap.add_argument("--normal_depth_step_rel", type=float, default=None,
                    help="... leaving out window cells whose depth differs from the point's by more than this fraction of it (> 0; default 0.05; "
                         "needs --estimate_normals)")
    ap.add_argument("--fuse_voxel_size", type=float, default=0.0,
                    help="oriented voxel fusion of the final cloud: merge the points of every voxel of this size (scene units) per side their normals "
                         "face - one oriented point per visible face of a voxel; runs behind the filters and --max_points (needs "
                         "--estimate_normals; 0 = off)")
    ap.add_argument("--gaussian_init", action="store_true",
                    help="write an initial Gaussian set instead of the point file: a PLY in the 3DGS point_cloud.ply layout at SH degree 0, the scale from "
                         "the exact distance to the three nearest neighbours, the rotation taking +z onto the normal (needs --estimate_normals)")
    ap.add_argument("--gaussian_flatten", type=float, default=None,
                    help="... extent along the normal relative to the extent in the plane, in (0, 1] (default 1 = isotropic, the 3DGS initialisation; "
                         "needs --gaussian_init)")
    ap.add_argument("--gaussian_opacity", type=float, default=None, help="... initial opacity in (0, 1) (default 0.1, the 3DGS value; needs --gaussian_init)")
    ap.add_argument("--gaussian_max_scale", type=float, default=None,
                    help="... upper bound on the initial extent in scene units (default 0 = none; needs --gaussian_init)")
    ap.add_argument("--cap_mode", type=str, default="random", choices=["random", "spatial"],
                    help="how --max_points chooses: 'random' is upstream's uniform draw; 'spatial' keeps one point per cell along a Morton curve over "
                         "the cloud - the point of smallest reprojection error -, so sparse regions are not starved (needs --max_points)")
    ap.add_argument("--keep_threads", action="store_true",
                    help="leave torch's intra-op thread count alone (by default it is lowered to the container's CPU quota; the count decides the last "
                         "bits of upstream's sampling normaliser, so a run compared bit for bit with upstream keeps upstream's setting)")
    return ap


def main(argv=None) -> int:
    """The command line (upstream densify.py:418-420).  As its own process it fits torch's intra-op threads to the container's CPU quota first
    (core/hostenv.py: a pool sized by the CPUs the container SEES gets the whole process throttled); inside LichtFeld Studio - ``dense_init`` /
    ``dense_init_from_lfs`` called by the plugin - process-wide settings are the host application's and nothing is touched."""
    from .core import hostenv
    args = build_argparser().parse_args(argv)
    if not args.keep_threads:
        import torch
        before = int(torch.get_num_threads())
        after = hostenv.fit_threads_to_quota(log=log.info)
        if after != before:
            log.info("note: upstream's sampling normaliser is a torch f32 sum whose last bits depend on the thread count - for draws bit-identical "
                     "to an upstream run on this machine pass --keep_threads or set OMP_NUM_THREADS to upstream's count")
    return dense_init(args)


if __name__ == "__main__":
    raise SystemExit(main())
