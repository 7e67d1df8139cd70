"""Boundary types of the dense-initialisation path.

``DensePipelineConfig`` keeps the 18 fields of the upstream dataclass with the same names, order and
defaults (upstream core/config.py:7-26) so that the GUI panel / CLI can construct it unchanged, and
adds twelve settings of this implementation *after* them (all defaulted, so positional construction still
works) plus one ``experimental`` dict for the knobs that exist only because an experiment was run.
``problem()`` names every combination that cannot run: nothing is silently ignored.
``CameraRecord`` keeps upstream's per-camera record (core/camera_models.py:10-28): f32 intrinsics and
world-to-camera pose, the projection ``P = K [R|t]`` and the centre ``C = -R^T t``.
"""
from __future__ import annotations

import dataclasses
from typing import Dict, Optional, Tuple

import numpy as np

TRIANGULATION_MODES = ("sampled", "dense")
AUTO_REFS_PER_LAUNCH = 16         # refs_per_launch = 0 (the default) where several references per launch are possible and nobody waits for previews

# Knobs that exist because an experiment was run: they stay reachable for the profiles and the tests that pin them, but they are not
# part of the configuration surface a caller is expected to touch.  ``DensePipelineConfig(experimental={...})``; an unknown key is an error.
EXPERIMENTAL_DEFAULTS = {
    # sharded runs (torch.distributed, world > 1): the exchange happens in ROUNDS beside the compute (core/distributed.py::OverlappedExchange)
    # instead of ONE exchange after the last reference; same sequence either way.  Not used together with stream_output (one communicator at a time).
    "exchange_overlap": True,
    # references per round of the overlapped exchange (0: refs_per_launch, at least 4)
    "exchange_round": 0,
    # what the overlapped exchange moves: "f32" the 28-byte rows of the result; "ply" the 15-byte PLY vertex records packed on the device
    # (positions exact, colours as the writer quantises them, no reprojection error: the result's rgb is then u8 / 255 and err zero);
    # "auto": "ply" when the output is a .ply and no voxel filter has to see f32 colours
    "exchange_records": "f32",
    # fraction of the reference list (its LAST references) computed by every rank that receives the cloud instead of exchanged
    # (core/distributed.py::plan_replication says when that pays: never with a real matcher in the loop)
    "exchange_replicate": 0.0,
    # sharded run + stream_output on ONE node: every rank writes its own byte ranges of the output file, only counts travel
    "stream_shared_file": False,
    # dense mode: the kernel with UNORDERED retirement + lfd_order_segments (bit-identical result, ~6 % less kernel time)
    "dense_tile_segments": False,
    # hand upstream's own fundamental matrices (np.linalg.inv products, computed on the host exactly as upstream computes them) to the
    # kernels instead of the closed-form F the library derives from the camera table (agrees to ~2e-6 relative, not bit for bit)
    "upstream_fundamental": True,
    # backend="host": threads of the CPU twin (0: all hardware threads)
    "host_threads": 0,
    # RoMa-v2's local correlation (the conv refiners' one custom operator, CUDA-only upstream) through lfd_local_corr instead of the model's
    # grid_sample fallback (core/local_corr.py): within the derived error bound of the fallback, not bit for bit - hence off
    "fused_local_corr": False,
    # the conv blocks of RoMa-v2's refiners (depthwise 5x5, eval-mode BatchNorm, ReLU, 1x1 convolution; 27 per direction and pair) through
    # lfd_refiner_block instead of torch's separate kernels (core/refiner_blocks.py): one read and one write of the activation.
    # Rounds less often than the bf16 autocast sequence - closer to the f32 evaluation, not bit-identical to the model's own path - hence off
    "fused_refiner_blocks": False,
    # what each of RoMa-v2's refiners runs behind its ninth block (f32 cast, two 1x1 convolutions, warp update, softplus, Cholesky-to-precision
    # conversion, addition of the previous state: about twenty torch kernels) through ONE lfd_refiner_head launch (core/refiner_head.py,
    # DESIGN.md 4.20).  Within the derived rounding bound of the model's own f32 tail, not bit for bit - hence off
    "fused_refiner_head": False,
    # forward-backward consistency filter on the matcher's two warps (lfd_cycle_gate): a cell whose round trip A -> B -> A misses
    # its start by more than this many pixels of the match image loses the pair (certainty exactly 0, as if mask_b had masked it out).
    # 0.0 = off: the backward warp is not asked for and no new code runs.  Needs a matcher that hands out warp_BA (supports_backward_warp).
    "cycle_thresh_px": 0.0,
    # multi-view support filter behind triangulation (lfd_support_filter): a triangulated point is kept only if at least this many
    # OTHER loaded neighbours of its reference - the ones the arg-max did not pick - see it where their own warp says the cell is.
    # 0 = off: no new code runs.  At most nns_per_ref - 1; a reference that loaded fewer than min_support_views + 1 neighbours keeps no point.
    "min_support_views": 0,
    # ... within this many pixels of the neighbour's camera image (the unit of reproj_thresh).  0.0 = 2 * reproj_thresh: the residual in a third
    # view carries that view's own matching noise plus the depth error of the two-view point.
    "support_thresh_px": 0.0,
    # multi-view re-triangulation of supported points (lfd_refine_multiview): a two-view point that OTHER loaded neighbours of its
    # reference confirm within support_threshold() is triangulated again from all the views that see it and moved there when the result still
    # passes the two-view tests and every confirming view still agrees.  Nothing is added or dropped.  False = off: no new code runs.
    "multiview_refine": False,
    # ... with every view's rows weighted by the 2x2 precision matrix RoMa-v2 predicts for the match (lfd_refine_multiview_weighted, DESIGN.md
    # 4.10) instead of equally.  Needs multiview_refine and a matcher that hands out the precision planes (supports_precision); a point with an
    # unusable plane in any of its views is solved unweighted.  Never changes which points are emitted.  False = off: no new code runs.
    "precision_weighted_refine": False,
    # depth-uncertainty gate behind triangulation (lfd_depth_sigma_filter): a point is kept only if the 1-sigma bound on its
    # relative depth error along the reference's ray - from the views that placed it, their geometry and their match precision - is at most
    # this.  The last stage behind support filter and re-triangulation.  0.0 = off: no new code runs.
    "max_depth_sigma_rel": 0.0,
    # ... with every match taken to have this isotropic 1-sigma noise in px of the camera image (the unit of reproj_thresh).  0.0 = RoMa-v2's
    # own 2x2 precision per match instead: needs a matcher that hands out the precision planes (supports_precision).
    "match_sigma_px": 0.0,
    # cross-reference consensus filter on the final cloud (lfd_consensus_filter): a point is kept only if at least this many
    # OTHER references put a point within consensus_radius of it - the one test that compares what different references say about the same
    # surface.  Runs once, behind the run and in front of the point cap and the voxel filter.  1 .. 8; 0 = off: no new code runs.
    "min_consensus_refs": 0,
    # ... within this distance, in scene units (the unit of voxel_size).  Required > 0 with the filter on, 0 with it off.
    "consensus_radius": 0.0,
    # undistort every image (and its mask) on its way in (lfd_undistort_image): a COLMAP camera with a SIMPLE_RADIAL, RADIAL,
    # OPENCV or FULL_OPENCV model is resampled into the pinhole image of the same K before anything matches it - every later stage assumes
    # pinhole cameras.  Pixels the photograph does not cover become masked.  Any other distorted model (the fisheye family, FOV) is refused
    # by name.  False = off: no new code runs (a camera with non-zero coefficients then draws one warning: its distortion is ignored).
    "undistort_images": False,
    # per-point surface normals from the resident warps (lfd_estimate_normals): every emitted point gets the unit normal of the
    # plane fitted to its winning neighbour's warp in a window of grid cells around its own cell, oriented towards its reference's camera; the
    # output PLY then has 27-byte x y z nx ny nz r g b vertices.  The last stage behind support filter, re-triangulation and depth gate; never
    # changes which points are emitted or where.  False = off: no new code runs and the output is the 15-byte file, byte for byte.
    "estimate_normals": False,
    # ... over the (2 r + 1)^2 window of this radius, 1 .. 4 grid cells.  With iid matching noise a 3 x 3 window is useless (tens of degrees);
    # the matcher's noise is smoother than iid, so the default is a judgement - DESIGN.md 4.14 records the measured error per radius.
    "normal_radius_cells": 3,
    # ... leaving out window cells whose depth in the reference differs from the point's by more than this fraction of it.  On a plane tilted
    # 80 degrees to the image, cells r apart differ in relative depth by r tan(80 deg) / f_cells (f_cells: the focal length in grid cells,
    # about 400 at 512^2): under 0.03 up to r = 2, 0.057 at r = 4.  At 0.05 only the outermost cells of the widest windows on the steepest
    # planes are cut, while a foreground / background step is far over 0.05.
    "normal_depth_step_rel": 0.05,
    # free-space filter on the final cloud (lfd_freespace_filter): every reference's own points are a sparse depth map of what it
    # saw; a point is dropped when at least this many OTHER references triangulated a surface behind it on the same ray - they looked through
    # it - and more references refute than confirm it.  Runs once, behind the consensus filter and in front of the point cap and the voxel
    # filter.  1 .. 255; 0 = off: no new code runs.
    "min_freespace_violations": 0,
    # ... with this relative depth tolerance, in (0, 1): a depth within it of a reference's z-buffer confirms, only a depth more than it in
    # front refutes.  The default is a judgement (the value the prototype scene of DESIGN.md 4.15 was checked at); do not set it below the
    # relative depth noise you accept, e.g. your max_depth_sigma_rel.  Refused with the filter off unless left at the default.
    "freespace_depth_tol_rel": 0.02,
    # ... on z-buffer planes of this many cells along the longer image side, 8 .. 4096.  0 = automatic: ceil(sqrt(matches_per_ref)) in sampled
    # mode (about one emitted point per cell), the longer side of the matcher's grid in dense mode.
    "freespace_plane_cells": 0,
    # oriented voxel fusion on the final cloud (lfd_fuse_oriented): the points of every occupied voxel of this size - scene
    # units, the unit of voxel_size - are merged per side their normals face: positions and colours averaged, normals summed and renormalised,
    # one oriented point per visible face of the voxel (the two faces of a thin wall stay two points).  Needs estimate_normals.  Runs once,
    # behind the consensus filter, the free-space filter and the point cap, in front of packing.  0 = off: no new code runs.
    "fuse_voxel_size": 0.0,
    # Gaussian-ready output (lfd_knn_dist2 + lfd_pack_gaussians): the output file is an initial Gaussian set - a PLY in the 3DGS
    # point_cloud.ply layout at SH degree 0 (x y z nx ny nz f_dc_0..2 opacity scale_0..2 rot_0..3, 68 bytes a vertex) - instead of the 27-byte
    # point file: the colour as the SH DC term, a constant opacity, the scale from the exact mean squared distance to the three nearest
    # neighbours (clamped below at 1e-7, as 3DGS does), the rotation taking +z onto the normal.  Needs estimate_normals.  The last stage, behind
    # the consensus filter, the free-space filter, the point cap and the oriented fusion.  False = off: no new code runs.
    "gaussian_init": False,
    # ... the Gaussian's extent along the normal relative to its extent in the plane, in (0, 1]: 1 is the isotropic 3DGS initialisation
    "gaussian_flatten": 1.0,
    # ... the initial opacity, in (0, 1): 0.1 is the 3DGS value
    "gaussian_opacity": 0.1,
    # ... an upper bound on the initial extent in scene units (what an isolated point would otherwise get is the distance to far neighbours); 0 = none
    "gaussian_max_scale": 0.0,
    # how max_points chooses.  "random": upstream's uniform draw, which keeps the cloud's density contrast - what many references
    # saw is kept many times over.  "spatial" (lfd_cap_spatial): one point per cell of the coarsest Morton level that has max_points occupied
    # cells, the cells picked evenly along the curve, each cell's point of smallest reprojection error; the kept points stay in input order.
    # Needs max_points > 0.  "random" = today's behaviour: no new code runs.
    "cap_mode": "random",
    # multi-view point colour (lfd_colour_multiview): a point's colour becomes the "mean" or the "median", per channel, over the
    # views that see it - its reference (upstream's colour), the neighbour that won it and every other loaded neighbour that the support
    # filter's test confirms within support_threshold() - instead of the one photograph's sample.  Rewrites rgb only: no point, count or order
    # changes, and it works with or without min_support_views.  Behind support filter, re-triangulation and depth gate, in front of the
    # normals.  "off" = today's colour: no new code runs and every output stays byte-identical.
    "multiview_colour": "off",
    # per-image exposure gains (lfd_gain_accumulate / lfd_gain_apply): while each reference is resident the colour of its points
    # and of every view that confirms them (the multi-view colour's views, within support_threshold()) is summed per (reference, neighbour);
    # at the end of the run one factor per image ("luma") or per image and channel ("rgb") is solved from those sums over the whole pair graph
    # and every point's colour is multiplied by its reference's factor: the cloud comes out at one exposure, and <output>.gains.json lists the
    # factors.  Rewrites rgb only, once, in front of the consensus filter.  "off" = no new code runs and every output stays byte-identical.
    "gain_compensation": "off",
    # photo-consistency gate behind triangulation (lfd_photo_gate): the one gate that looks at the pixels.  A point is dropped
    # when the zero-mean normalised cross-correlation of the two patches its match joins - the reference's around the point's cell, the winning
    # neighbour's where the dense warp sends those cells - is below this, provided at least half the window takes part and both patches are
    # textured.  Refutes gross mismatches of a few match pixels on textured surfaces (a match that slid along its epipolar line passes every
    # geometric gate); it does not refute sub-pixel error.  Behind the depth-uncertainty gate, in front of colour, gains and normals.
    # In (0, 1]; 0.0 = off: no new code runs and every output stays byte-identical.
    "min_photo_ncc": 0.0,
    # ... over the (2 r + 1)^2 window of this radius, 1 .. 3 grid cells.  Refused with the gate off unless left at the default.
    "photo_window_cells": 2,
    # ... a patch whose standard deviation is below this many 8-bit grey levels is no evidence either way: the point is kept.  >= 0.  A design
    # default, not a measurement.  Refused with the gate off unless left at the default.
    "photo_min_texture": 2.0,
    # per-camera depth and normal maps rendered from the final cloud (lfd_render_depth): a directory - relative to the output
    # file's own - that receives <image stem>.npy (f32 (ph, pw): depth along the camera's z axis in scene units, 0 = no data), with
    # estimate_normals <image stem>_normal.npy (f32 (ph, pw, 3): world frame, the PLY's normals, 0 0 0 = no data) and depth_maps.json, for EVERY
    # loaded camera, not only the references.  The cloud rendered is the one behind the consensus and free-space filters and in front of
    # max_points, fusion and the voxel filter; a side output: the point file does not change by a byte.  "" = off: no new code runs.
    "depth_maps_dir": "",
    # ... on planes of this many cells along the longer image side, 8 .. 4096; 0 = automatic, by freespace_plane_cells' rule: ceil(sqrt(
    # matches_per_ref)) in sampled mode, the longer side of the matcher's grid in dense mode.  All cameras share the plane of the first.
    "depth_map_cells": 0,
    # ... every point drawn as a square of 2 r + 1 cells at its own depth, r = 0 .. 3: closes the gaps between the points of one surface
    "depth_map_splat_cells": 1,
    # ... and a cell dropped when something nearer lies within this many cells, 0 .. 8 (0: no test): a cloud is not watertight, and this is
    # what keeps the back wall from showing through the gaps of the front wall.  Background this close to a silhouette is dropped too.
    "depth_map_window_cells": 3,
    # ... "nearer" meaning by more than this fraction of the nearer depth, in (0, 1).  The free-space filter's default and, like it, a
    # judgement, not a measurement; a surface whose depth changes by more across the window loses its far side.
    "depth_map_tol_rel": 0.02,
    # footprint-adaptive thinning of the final cloud (lfd_thin_footprint): at most one point per cell of an octree over the cloud,
    # where the cell a point falls into is this many match-grid cells of its OWN reference camera wide at the point's depth (rounded up to the
    # next octree level, so up to twice that): constant density in image space instead of world space - the table at 2 units and the trees at
    # 50 are both thinned to what their cameras resolved.  A cell keeps its point of smallest reprojection error; the kept points stay in
    # input order with their bits.  Runs once, behind the consensus and free-space filters and the depth maps, in front of max_points, fusion,
    # the Gaussian output and the voxel filter.  0.5 removes little more than the duplicates between references; 2 keeps about a third of a
    # lone reference's samples.  0 = off: no new code runs and every output stays byte-identical.
    "footprint_thin_cells": 0.0,
    # far-field shell (lfd_far_accumulate / lfd_far_emit): points at infinity for sky, skyline and distant background - the
    # cells every filter rightly drops because their depth is unknown.  A grid cell is FAR when every neighbour that matched it confidently
    # sees it where the rotation-only transfer predicts; far cells are summed into a cube map of direction cells, and at the end of the run
    # every occupied direction cell becomes one point on a sphere around the cameras, coloured by the mean of its samples.  "file" writes them
    # to <output stem>_shell.ply beside an unchanged main file, "merge" appends them behind the cloud's records in the main PLY; both write
    # <output file>.shell.json.  The positions are a convention, not depth.  "off" = no new code runs and every output stays byte-identical.
    "far_shell": "off",
    # ... a neighbour agrees with infinity within this many px of ITS camera image, as support_thresh_px; 0 = reproj_thresh
    "far_thresh_px": 0.0,
    # ... a neighbour is confident at a cell when its raw certainty is at least this, in (0, 1].  A design default, not a measurement.
    "far_certainty": 0.5,
    # ... at least min(this, the reference's neighbours) confident neighbours, all of which must agree, 1 .. 8
    "far_min_views": 2,
    # ... direction cells along a cube face's side, 8 .. 512 (6 S^2 cells in all)
    "far_shell_cells": 256,
    # ... a direction cell becomes a point when it holds at least this many samples, >= 1
    "far_min_samples": 2,
    # ... radius of the sphere in scene units; 0 = automatic: max(10 x the cameras' spread, 1.25 x the cloud's) around the cameras' mean centre
    "far_shell_radius": 0.0,
    # epipolar audit (lfd_epipolar_audit): a report on the camera poses from the run's own matches.  Every confident match is
    # measured against its pair's epipolar line as the poses give it, in eighths of a px of the neighbour's camera image, and counted per
    # (reference, neighbour) pair; at the end of the run <output file>.audit.json holds the histograms, per-pair medians, a score per camera
    # (the lower median of its pairs' medians) and the cameras whose score exceeds audit_warn_px - each of them is logged as a warning.  The
    # statistics move no point: cloud, counts and order are the knob-off run's.  It sees only the error ACROSS the epipolar lines, cannot tell
    # a pose from intrinsics or distortion (see undistort_images), and contains the matcher's own error.  "off" = no new code runs.
    "epipolar_audit": "off",
    # ... a neighbour is confident at a cell when its raw certainty is at least this, in (0, 1].  far_certainty's design default, not a measurement.
    "audit_certainty": 0.5,
    # ... a pair is judged when it has at least this many confident matches, >= 1.  A design default.
    "audit_min_samples": 256,
    # ... a camera is suspect when its score exceeds this many px of a camera image; 0 = reproj_thresh
    "audit_warn_px": 0.0,
    # ... directory (relative to the output file's) for one <image stem>_epi.npy per reference: f32 (H, W), the smallest distance any confident
    # neighbour reports for the cell in px of that neighbour's camera image, NaN where there is none - what moved between the photographs
    "audit_maps_dir": "",
    # pose corrections from the matches (lfd_pose_accumulate): one Gauss-Newton step on the epipolar error.  Every confident
    # match adds its row of the normal equations with respect to its pair's relative pose, as quantised integers, per (reference, neighbour)
    # pair; at the end of the run core/poses.py projects the gauge out, solves, and <output file>.poses.json holds one corrected
    # world-to-camera pose per camera.  The statistics move no point: cloud, counts and order are the knob-off run's; a SECOND run takes the
    # file through pose_corrections.  One linear step; sees only the error ACROSS the epipolar lines; cannot tell a pose from intrinsics;
    # contains the matcher's own error.  "off" = no new code runs.
    "pose_refine": "off",
    # ... a neighbour is confident at a cell when its raw certainty is at least this, in (0, 1].  audit_certainty's design default.
    "pose_certainty": 0.5,
    # ... a confident match further than this many px of the neighbour's camera image from its epipolar line is an outlier, in (0, 64].  The
    # audit's histogram range, a design default.
    "pose_inlier_px": 8.0,
    # ... a pair enters the solve when it has at least this many inliers, >= 1.  A design default.
    "pose_min_samples": 256,
    # a poses.json of an earlier run (path; "" = none): its poses replace the camera records' before anything else runs
    "pose_corrections": "",
    # connected-component filter on the final cloud (lfd_component_filter): the floater rule that needs no second witness.  Two
    # points are linked when they are within component_radius of each other; a point is kept only if the connected component it belongs to
    # has at least this many points - a clump of tens of points hanging in the air goes, a surface stays however few references saw it.
    # Exact: no statistic, no order dependence.  A floater within the radius of a surface joins it; a legitimately small isolated object
    # goes.  Runs once, behind the consensus and free-space filters, in front of the depth maps, thinning, cap, fusion, Gaussian output and
    # voxel filter; writes <output file>.components.json.  >= 2; 0 = off: no new code runs and every output stays byte-identical.
    "min_component_points": 0,
    # ... within this distance, in scene units (the unit of voxel_size).  Required > 0 with the filter on, 0 with it off.  One number for the
    # whole scene: in unbounded scenes far, sparse structure fragments - see footprint_thin_cells and far_shell for that end.
    "component_radius": 0.0,
}
POSE_MODES = ("off", "report")
POSE_KNOBS = ("pose_certainty", "pose_inlier_px", "pose_min_samples")
AUDIT_MODES = ("off", "report")
AUDIT_KNOBS = ("audit_certainty", "audit_min_samples", "audit_warn_px", "audit_maps_dir")
FAR_MODES = ("off", "file", "merge")
FAR_KNOBS = ("far_thresh_px", "far_certainty", "far_min_views", "far_shell_cells", "far_min_samples", "far_shell_radius")
CAP_MODES = ("random", "spatial")
COLOUR_MODES = ("off", "mean", "median")
GAIN_MODES = ("off", "luma", "rgb")
CONSENSUS_CAP = 8            # LFD_CONSENSUS_CAP of include/lfd_densify.h


@dataclasses.dataclass
class DensePipelineConfig:
    output_path: str
    roma_setting: str = "fast"
    roi_only_selected: bool = False
    num_refs: float = 0.8
    nns_per_ref: int = 3
    matches_per_ref: int = 10000
    certainty_thresh: float = 0.20
    reproj_thresh: float = 0.8
    sampson_thresh: float = 5.0
    min_parallax_deg: float = 0.5
    max_points: int = 0
    no_filter: bool = False
    use_masks: bool = True
    voxel_size: float = 0.0
    seed: int = 0
    viz_interval: int = 3
    prefetch_packages: int = 8
    pack_workers: int = 4
    # ---- extensions of this implementation (not present upstream; 12 + the experimental dict) -------------------------------------------
    # "sampled": upstream behaviour - coverage sampling picks ~0.85*M+tiles cells per reference and
    #            only those are triangulated.  "dense": every grid cell upstream's sampler COULD draw (best certainty after
    #            floor and masks not <= 0: a masked-out cell never is) goes through the fused kernel.
    triangulation_mode: str = "sampled"
    # references whose RoMa outputs are kept resident and triangulated by ONE kernel launch (dense mode) or ONE fused call (sampled mode: on
    # upstream's single RNG stream - lfd_triangulate_sampled_chain - or on per-reference streams; same results either way).  0 = automatic
    # (``launch_group``): AUTO_REFS_PER_LAUNCH where that is possible and nobody waits for intermediate results, else 1.
    refs_per_launch: int = 0
    # per-reference RNG stream (seed ^ uid) instead of upstream's single process-global stream;
    # forced on when references are sharded over several GPUs (results then do not depend on
    # the shard count).
    per_reference_rng: bool = False
    # where the coverage-sampling stage of the "sampled" mode runs: "device" (lfd_select_samples: the
    # whole per-reference path stays where the backend runs) or "host" (core/sampling.py: the library calls
    # upstream makes, including torch's own f32 sum as the normaliser).
    selection_backend: str = "device"
    # selection on the device, one RNG stream (upstream's mode), filter mode: normalise the sampling weights with upstream's OWN normaliser -
    # torch's CPU f32 `sum` of the weight map, computed on this host exactly as core/sampling.py:27-31 computes it - instead of the device's
    # correctly rounded exact sum (the cells drawn are then the ones upstream draws ON THE SAME MACHINE, bit for bit).  Per-reference
    # streams / sharded runs / no_filter / dense mode have no such normaliser and are not affected.
    upstream_normaliser: bool = True
    # dense mode: blend colours with upstream's f64 arithmetic (bit-identical rgb) instead of f32 (within 2.5e-7); sampled mode always does
    exact_colour: bool = False
    # write the output PLY while the run proceeds: every completed reference's survivors leave as 15-byte records packed on the device
    # (dense mode: written by the kernel itself, copied out on a side stream while the next launch computes) and are appended to
    # ``output_path``; the vertex count in the header is patched at the end.  Needs a .ply output and neither a point cap nor a voxel
    # filter (both have to see the whole cloud first).
    stream_output: bool = False
    # resize / mask / black-out the decoded images on the GPU (lfd_prepare_image / lfd_prepare_mask: Pillow's BILINEAR and
    # NEAREST arithmetic, bit for bit) instead of with PIL on the host pack threads; decoding stays on the host
    device_image_prep: bool = False
    # compute every camera's backbone (DINOv3) features once per run and share them between the references that list the camera
    # (core/scheduler.py); upstream recomputes a neighbour's features for every reference
    share_features: bool = True
    # neighbours of a reference matched per RoMa-v2 forward (1 = upstream's loop, core/matcher.py:175-188)
    pairs_per_forward: int = 1
    # where the per-reference hot path runs.  "device": the HIP kernels (needs a GPU; raises HipBackendError without one - there is
    # no fallback).  "host": the CPU twin of the C-ABI (lfd_create_host) with the host sampling stage - upstream's CPU-only configuration
    # (densify.py:148-212 run without a GPU, BASELINE config 1); chosen by the caller, never automatically.
    backend: str = "device"
    # how the survivors of a sharded run (torch.distributed, world > 1) reach the writer: "all_gather" leaves the whole cloud on
    # every rank (what BASELINE's north star names), "gather_to_root" sends every rank's records straight to their place in rank
    # 0's buffer (the other ranks return their own shard only)
    exchange: str = "all_gather"
    experimental: Dict[str, object] = dataclasses.field(default_factory=dict)

    def __post_init__(self) -> None:
        self.validate()

    def exp(self, key: str):
        """The value of an experimental knob (EXPERIMENTAL_DEFAULTS lists them)."""
        return self.experimental.get(key, EXPERIMENTAL_DEFAULTS[key])

    def support_threshold(self) -> float:
        """Threshold of the multi-view support filter in px of the neighbour's camera image (experimental['support_thresh_px'], 0 = 2 * reproj_thresh)."""
        tau = float(self.exp("support_thresh_px"))
        return tau if tau > 0.0 else 2.0 * float(self.reproj_thresh)

    def audit_warn_threshold(self) -> float:
        """The score above which the epipolar audit calls a camera suspect, in px (experimental['audit_warn_px'], 0 = reproj_thresh)."""
        tau = float(self.exp("audit_warn_px"))
        return tau if tau > 0.0 else float(self.reproj_thresh)

    def far_threshold(self) -> float:
        """Threshold of the far-field shell's agreement test in px of the neighbour's camera image (experimental['far_thresh_px'], 0 = reproj_thresh)."""
        tau = float(self.exp("far_thresh_px"))
        return tau if tau > 0.0 else float(self.reproj_thresh)

    def exchange_record_format(self) -> str:
        rec = str(self.exp("exchange_records"))
        if rec == "auto":
            return "ply" if (str(self.output_path).lower().endswith(".ply") and float(self.voxel_size) <= 0.0) else "f32"
        return rec

    def launch_group(self, world: int = 1, previews: bool = False) -> int:
        """The references per launch / fused call a run uses.  An explicit ``refs_per_launch`` is taken as it is.  Automatic (0): one reference at
        a time - upstream's cadence - when somebody watches the run proceed (intermediate previews), on the host backend, with the host selection
        stage in sampled mode, and in sharded runs (every rank has to derive the same number from the configuration alone); else
        AUTO_REFS_PER_LAUNCH: the results are the same, the references' kernels run side by side instead of one after the other."""
        n = int(self.refs_per_launch)
        if n > 0:
            return n
        if previews or int(world) > 1 or self.backend != "device":
            return 1
        if self.triangulation_mode != "dense" and self.selection_backend != "device":
            return 1
        return AUTO_REFS_PER_LAUNCH

    def problem(self) -> Optional[str]:
        """Why this combination of settings cannot run, or None.  Every pair of settings either works together or is named here: nothing
        is silently ignored (tests/test_config_matrix.py generates the pairs)."""
        if self.triangulation_mode not in TRIANGULATION_MODES:
            return f"triangulation_mode must be one of {TRIANGULATION_MODES}, got {self.triangulation_mode!r}"
        if int(self.refs_per_launch) < 0:
            return "refs_per_launch must be >= 1 (or 0: automatic)"
        if int(self.pairs_per_forward) < 1:
            return "pairs_per_forward must be >= 1"
        if self.selection_backend not in ("device", "host"):
            return "selection_backend must be 'device' or 'host'"
        if self.backend not in ("device", "host"):
            return "backend must be 'device' or 'host'"
        if self.exchange not in ("all_gather", "gather_to_root"):
            return "exchange must be 'all_gather' or 'gather_to_root'"
        if not isinstance(self.experimental, dict):
            return "experimental must be a dict"
        unknown = sorted(set(self.experimental) - set(EXPERIMENTAL_DEFAULTS))
        if unknown:
            return f"unknown experimental setting(s) {unknown}; known: {sorted(EXPERIMENTAL_DEFAULTS)}"
        if self.exp("exchange_records") not in ("f32", "ply", "auto"):
            return "experimental['exchange_records'] must be 'f32', 'ply' or 'auto'"
        if int(self.exp("exchange_round")) < 0:
            return "experimental['exchange_round'] must be >= 0"
        if not (0.0 <= float(self.exp("exchange_replicate")) <= 1.0):
            return "experimental['exchange_replicate'] must be a fraction in [0, 1]"
        try:
            tau = float(self.exp("cycle_thresh_px"))
        except (TypeError, ValueError):
            return "experimental['cycle_thresh_px'] must be a number (px of the match image; 0 = off)"
        if not (0.0 <= tau < float("inf")):
            return "experimental['cycle_thresh_px'] must be finite and >= 0 (px of the match image; 0 = off)"
        dense = self.triangulation_mode == "dense"
        m_sup = self.exp("min_support_views")
        if isinstance(m_sup, bool) or not isinstance(m_sup, (int, np.integer)) or int(m_sup) < 0:
            return "experimental['min_support_views'] must be a non-negative integer (other neighbours that have to confirm a point; 0 = off)"
        try:
            tau_sup = float(self.exp("support_thresh_px"))
        except (TypeError, ValueError):
            return "experimental['support_thresh_px'] must be a number (px of the neighbour's camera image; 0 = 2 * reproj_thresh)"
        if not (0.0 <= tau_sup < float("inf")):
            return "experimental['support_thresh_px'] must be finite and >= 0 (px of the neighbour's camera image; 0 = 2 * reproj_thresh)"
        if int(m_sup) > 0:
            if int(m_sup) > int(self.nns_per_ref) - 1:
                return (f"experimental['min_support_views'] = {int(m_sup)} asks for more confirming neighbours than a reference has beside the one "
                        f"that made the point (nns_per_ref - 1 = {int(self.nns_per_ref) - 1})")
            if not (self.support_threshold() > 0.0):
                return "experimental['min_support_views'] needs a threshold: experimental['support_thresh_px'] or, for its default, reproj_thresh must be > 0"
            if dense and self.stream_output:
                return ("experimental['min_support_views'] filters points held as arrays (xyz, cell, slot); dense mode with stream_output has the "
                        "kernel write PLY records instead")
            if self.exp("dense_tile_segments"):
                return "experimental['min_support_views'] needs the ordered dense result; experimental['dense_tile_segments'] retires tiles unordered"
            if self.exchange_record_format() == "ply":
                return "experimental['min_support_views'] filters f32 rows; experimental['exchange_records'] must be 'f32' with it"
        refine = self.exp("multiview_refine")
        if not isinstance(refine, (bool, np.bool_)):
            return "experimental['multiview_refine'] must be True or False"
        if refine:
            if self.no_filter:
                return "experimental['multiview_refine'] accepts a point by the two-view tests; no_filter switches them off"
            if not (float(self.reproj_thresh) > 0.0) or not (self.support_threshold() > 0.0):
                return "experimental['multiview_refine'] needs its thresholds: reproj_thresh must be > 0 (and experimental['support_thresh_px'] or its default)"
            if int(self.nns_per_ref) < 2:
                return "experimental['multiview_refine'] uses the neighbours beside the one that made a point: nns_per_ref must be at least 2"
            if dense and self.stream_output:
                return ("experimental['multiview_refine'] moves points held as arrays (xyz, cell, slot); dense mode with stream_output has the "
                        "kernel write PLY records instead")
            if self.exp("dense_tile_segments"):
                return "experimental['multiview_refine'] needs the ordered dense result; experimental['dense_tile_segments'] retires tiles unordered"
            if self.exchange_record_format() == "ply":
                return "experimental['multiview_refine'] moves f32 rows; experimental['exchange_records'] must be 'f32' with it"
        weighted = self.exp("precision_weighted_refine")
        if not isinstance(weighted, (bool, np.bool_)):
            return "experimental['precision_weighted_refine'] must be True or False"
        if weighted and not refine:
            return "experimental['precision_weighted_refine'] weights the rows of the multi-view re-triangulation: it needs experimental['multiview_refine'] = True"
        try:
            max_sigma = float(self.exp("max_depth_sigma_rel"))
        except (TypeError, ValueError):
            return "experimental['max_depth_sigma_rel'] must be a number (1-sigma relative depth error a point may have; 0 = off)"
        if not (0.0 <= max_sigma < float("inf")):
            return "experimental['max_depth_sigma_rel'] must be finite and >= 0 (1-sigma relative depth error a point may have; 0 = off)"
        try:
            iso_sigma = float(self.exp("match_sigma_px"))
        except (TypeError, ValueError):
            return "experimental['match_sigma_px'] must be a number (px of the camera image; 0 = the matcher's precision planes)"
        if not (0.0 <= iso_sigma < float("inf")):
            return "experimental['match_sigma_px'] must be finite and >= 0 (px of the camera image; 0 = the matcher's precision planes)"
        if iso_sigma > 0.0 and not max_sigma > 0.0:
            return "experimental['match_sigma_px'] is the match noise of the depth-uncertainty gate: it needs experimental['max_depth_sigma_rel'] > 0"
        if max_sigma > 0.0:
            if dense and self.stream_output:
                return ("experimental['max_depth_sigma_rel'] filters points held as arrays (xyz, cell, slot); dense mode with stream_output has the "
                        "kernel write PLY records instead")
            if self.exp("dense_tile_segments"):
                return "experimental['max_depth_sigma_rel'] needs the ordered dense result; experimental['dense_tile_segments'] retires tiles unordered"
            if self.exchange_record_format() == "ply":
                return "experimental['max_depth_sigma_rel'] filters f32 rows; experimental['exchange_records'] must be 'f32' with it"
        m_con = self.exp("min_consensus_refs")
        if isinstance(m_con, bool) or not isinstance(m_con, (int, np.integer)) or int(m_con) < 0:
            return "experimental['min_consensus_refs'] must be a non-negative integer (other references that have to put a point next to a point; 0 = off)"
        if int(m_con) > CONSENSUS_CAP:
            return f"experimental['min_consensus_refs'] = {int(m_con)} is more than the {CONSENSUS_CAP} references the filter counts (LFD_CONSENSUS_CAP)"
        try:
            r_con = float(self.exp("consensus_radius"))
        except (TypeError, ValueError):
            return "experimental['consensus_radius'] must be a number (scene units, the unit of voxel_size)"
        if not (0.0 <= r_con < float("inf")):
            return "experimental['consensus_radius'] must be finite and >= 0 (scene units, the unit of voxel_size)"
        if int(m_con) > 0 and not r_con > 0.0:
            return "experimental['min_consensus_refs'] needs a distance: experimental['consensus_radius'] must be > 0 (scene units, the unit of voxel_size)"
        if r_con > 0.0 and int(m_con) == 0:
            return "experimental['consensus_radius'] is the distance of the consensus filter: it needs experimental['min_consensus_refs'] >= 1"
        if int(m_con) > 0:
            if self.stream_output:
                return ("experimental['min_consensus_refs'] has to see the whole cloud before anything is written; stream_output writes the file "
                        "while the run proceeds")
            if self.exchange_record_format() == "ply":
                return "experimental['min_consensus_refs'] filters f32 rows; experimental['exchange_records'] must be 'f32' with it"
            if dense and self.exp("dense_tile_segments"):
                return ("experimental['min_consensus_refs'] needs the cloud as arrays with per-reference counts; dense mode with "
                        "experimental['dense_tile_segments'] retires tiles unordered")
        m_cmp = self.exp("min_component_points")
        if isinstance(m_cmp, (bool, np.bool_)) or not isinstance(m_cmp, (int, np.integer)) or not (0 <= int(m_cmp) <= 2 ** 31 - 1):
            return ("experimental['min_component_points'] must be an integer in 0 .. 2^31 - 1 (points a connected component has to have for its points "
                    "to stay; 0 = off)")
        if int(m_cmp) == 1:
            return "experimental['min_component_points'] = 1 keeps every point (a point is a component of its own): use 0 for off, or at least 2"
        try:
            r_cmp = float(self.exp("component_radius"))
        except (TypeError, ValueError):
            return "experimental['component_radius'] must be a number (scene units, the unit of voxel_size)"
        if not (0.0 <= r_cmp < float("inf")):
            return "experimental['component_radius'] must be finite and >= 0 (scene units, the unit of voxel_size)"
        if int(m_cmp) > 0 and not r_cmp > 0.0:
            return "experimental['min_component_points'] needs a distance: experimental['component_radius'] must be > 0 (scene units, the unit of voxel_size)"
        if r_cmp > 0.0 and int(m_cmp) == 0:
            return "experimental['component_radius'] is the link distance of the component filter: it needs experimental['min_component_points'] >= 2"
        if int(m_cmp) > 0:
            if self.stream_output:
                return ("experimental['min_component_points'] has to see the whole cloud before anything is written; stream_output writes the file "
                        "while the run proceeds")
            if self.exchange_record_format() == "ply":
                return "experimental['min_component_points'] filters f32 rows; experimental['exchange_records'] must be 'f32' with it"
            if self.exp("dense_tile_segments"):
                return ("experimental['min_component_points'] needs the cloud as arrays with per-reference counts; dense mode with "
                        "experimental['dense_tile_segments'] retires tiles unordered")
        m_fs = self.exp("min_freespace_violations")
        if isinstance(m_fs, bool) or not isinstance(m_fs, (int, np.integer)) or int(m_fs) < 0:
            return "experimental['min_freespace_violations'] must be a non-negative integer (other references that have to look through a point; 0 = off)"
        if int(m_fs) > 255:
            return f"experimental['min_freespace_violations'] = {int(m_fs)} is more than the 255 references the filter's counts hold"
        try:
            tol_fs = float(self.exp("freespace_depth_tol_rel"))
        except (TypeError, ValueError):
            return "experimental['freespace_depth_tol_rel'] must be a number (a relative depth, in (0, 1))"
        if not (0.0 < tol_fs < 1.0) or not (0.0 < float(np.float32(tol_fs)) < 1.0):
            return "experimental['freespace_depth_tol_rel'] must be in (0, 1) (a relative depth)"
        if int(m_fs) == 0 and tol_fs != float(EXPERIMENTAL_DEFAULTS["freespace_depth_tol_rel"]):
            return "experimental['freespace_depth_tol_rel'] is the tolerance of the free-space filter: it needs experimental['min_freespace_violations'] >= 1"
        c_fs = self.exp("freespace_plane_cells")
        if isinstance(c_fs, bool) or not isinstance(c_fs, (int, np.integer)) or (int(c_fs) != 0 and not 8 <= int(c_fs) <= 4096):
            return "experimental['freespace_plane_cells'] must be 0 (automatic) or an integer in 8 .. 4096 (z-buffer cells along the longer image side)"
        if int(c_fs) != 0 and int(m_fs) == 0:
            return "experimental['freespace_plane_cells'] is the z-buffer size of the free-space filter: it needs experimental['min_freespace_violations'] >= 1"
        if int(m_fs) > 0:
            if self.stream_output:
                return ("experimental['min_freespace_violations'] has to see the whole cloud before anything is written; stream_output writes the file "
                        "while the run proceeds")
            if self.exchange_record_format() == "ply":
                return "experimental['min_freespace_violations'] filters f32 rows; experimental['exchange_records'] must be 'f32' with it"
            if dense and self.exp("dense_tile_segments"):
                return ("experimental['min_freespace_violations'] needs the cloud as arrays with per-reference counts; dense mode with "
                        "experimental['dense_tile_segments'] retires tiles unordered")
        if not isinstance(self.exp("fused_refiner_blocks"), (bool, np.bool_)):
            return "experimental['fused_refiner_blocks'] must be True or False"
        if not isinstance(self.exp("fused_refiner_head"), (bool, np.bool_)):
            return "experimental['fused_refiner_head'] must be True or False"
        if not isinstance(self.exp("undistort_images"), (bool, np.bool_)):
            return "experimental['undistort_images'] must be True or False"
        normals = self.exp("estimate_normals")
        if not isinstance(normals, (bool, np.bool_)):
            return "experimental['estimate_normals'] must be True or False"
        r_nrm = self.exp("normal_radius_cells")
        if isinstance(r_nrm, bool) or not isinstance(r_nrm, (int, np.integer)) or not (1 <= int(r_nrm) <= 4):
            return "experimental['normal_radius_cells'] must be an integer in 1 .. 4 (grid cells around the point's own cell)"
        try:
            step_nrm = float(self.exp("normal_depth_step_rel"))
        except (TypeError, ValueError):
            return "experimental['normal_depth_step_rel'] must be a number (fraction of the point's depth in its reference)"
        if not (0.0 < step_nrm < float("inf")):
            return "experimental['normal_depth_step_rel'] must be finite and > 0 (fraction of the point's depth in its reference)"
        if not normals:
            if "normal_radius_cells" in self.experimental:
                return "experimental['normal_radius_cells'] is the window of the normal estimate: it needs experimental['estimate_normals'] = True"
            if "normal_depth_step_rel" in self.experimental:
                return "experimental['normal_depth_step_rel'] is the depth step of the normal estimate: it needs experimental['estimate_normals'] = True"
        else:
            if self.no_filter:
                return "experimental['estimate_normals'] takes a window cell by the two-view tests; no_filter switches them off"
            if not (float(self.reproj_thresh) > 0.0):
                return "experimental['estimate_normals'] needs the two-view threshold: reproj_thresh must be > 0"
            if self.stream_output:
                return ("experimental['estimate_normals'] writes 27-byte vertices from points held as arrays (xyz, cell, slot); stream_output "
                        "writes 15-byte records while the run proceeds")
            if self.exp("dense_tile_segments"):
                return "experimental['estimate_normals'] needs the ordered dense result; experimental['dense_tile_segments'] retires tiles unordered"
            if self.exchange_record_format() == "ply":
                return "experimental['estimate_normals'] adds a column to f32 rows; experimental['exchange_records'] must be 'f32' with it"
            if float(self.voxel_size) > 0.0:
                return ("experimental['estimate_normals'] cannot be combined with voxel_size: the voxel filter averages points, and what it should "
                        "do to their normals is not defined")
            if not str(self.output_path).lower().endswith(".ply"):
                return "experimental['estimate_normals'] writes the normals as PLY vertex properties: output_path must end in .ply"
        h_fuse = self.exp("fuse_voxel_size")
        if isinstance(h_fuse, (bool, np.bool_)) or not isinstance(h_fuse, (int, float, np.integer, np.floating)):
            return "experimental['fuse_voxel_size'] must be a number (scene units, the unit of voxel_size; 0 = off)"
        if not (0.0 <= float(h_fuse) < float("inf")):
            return "experimental['fuse_voxel_size'] must be finite and >= 0 (scene units, the unit of voxel_size; 0 = off)"
        if float(h_fuse) > 0.0 and not normals:
            return "experimental['fuse_voxel_size'] merges points by the side their normals face: it needs experimental['estimate_normals'] = True"
        g_init = self.exp("gaussian_init")
        if not isinstance(g_init, (bool, np.bool_)):
            return "experimental['gaussian_init'] must be True or False"
        number = lambda v: not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating))      # noqa: E731
        g_flat, g_op, g_max = self.exp("gaussian_flatten"), self.exp("gaussian_opacity"), self.exp("gaussian_max_scale")
        if not number(g_flat) or not (0.0 < float(g_flat) <= 1.0):
            return "experimental['gaussian_flatten'] must be a number in (0, 1] (extent along the normal relative to the extent in the plane; 1 = isotropic)"
        if not number(g_op) or not (0.0 < float(g_op) < 1.0):
            return "experimental['gaussian_opacity'] must be a number in (0, 1) (the initial opacity; 0.1 is the 3DGS value)"
        if not number(g_max) or not (0.0 <= float(g_max) < float("inf")):
            return "experimental['gaussian_max_scale'] must be a finite number >= 0 (scene units; 0 = none)"
        if not g_init:
            for key, what in (("gaussian_flatten", "flattening"), ("gaussian_opacity", "opacity"), ("gaussian_max_scale", "largest extent")):
                if float(self.exp(key)) != float(EXPERIMENTAL_DEFAULTS[key]):
                    return f"experimental['{key}'] is the {what} of the initial Gaussians: it needs experimental['gaussian_init'] = True"
        elif not normals:
            return "experimental['gaussian_init'] orients the Gaussians by the points' normals: it needs experimental['estimate_normals'] = True"
        cap_mode = self.exp("cap_mode")
        if not isinstance(cap_mode, str) or cap_mode not in CAP_MODES:
            return "experimental['cap_mode'] must be 'random' (upstream's draw) or 'spatial' (one point per cell along the Morton curve)"
        if cap_mode == "spatial" and int(self.max_points) <= 0:
            return "experimental['cap_mode'] = 'spatial' is how max_points chooses: it needs max_points > 0"
        colour = self.exp("multiview_colour")
        if not isinstance(colour, str) or colour not in COLOUR_MODES:
            return "experimental['multiview_colour'] must be 'off' (the reference's colour alone), 'mean' or 'median' (over the views that see the point)"
        if colour != "off":
            if not (self.support_threshold() > 0.0):
                return ("experimental['multiview_colour'] takes the other neighbours by the support filter's test: experimental['support_thresh_px'] or, "
                        "for its default, reproj_thresh must be > 0")
            if self.stream_output:
                return ("experimental['multiview_colour'] rewrites the colour of points held as arrays (xyz, rgb, cell, slot); stream_output writes "
                        "15-byte records while the run proceeds")
            if self.exp("dense_tile_segments"):
                return "experimental['multiview_colour'] needs the ordered dense result; experimental['dense_tile_segments'] retires tiles unordered"
            if self.exchange_record_format() == "ply":
                return "experimental['multiview_colour'] rewrites f32 rows; experimental['exchange_records'] must be 'f32' with it"
        try:
            photo_ncc = float(self.exp("min_photo_ncc"))
        except (TypeError, ValueError):
            return "experimental['min_photo_ncc'] must be a number (the ZNCC below which a match is refuted, in (0, 1]; 0 = off)"
        if not (0.0 <= photo_ncc <= 1.0):
            return "experimental['min_photo_ncc'] must be 0 (off) or in (0, 1] (the ZNCC below which a match is refuted)"
        photo_r = self.exp("photo_window_cells")
        if isinstance(photo_r, (bool, np.bool_)) or not isinstance(photo_r, (int, np.integer)) or not 1 <= int(photo_r) <= 3:
            return "experimental['photo_window_cells'] must be an integer in 1 .. 3 (radius of the photo-consistency window in grid cells)"
        try:
            photo_tex = float(self.exp("photo_min_texture"))
        except (TypeError, ValueError):
            return "experimental['photo_min_texture'] must be a number (standard deviation in 8-bit grey levels below which a patch is no evidence)"
        if not (0.0 <= photo_tex < float("inf")):
            return "experimental['photo_min_texture'] must be finite and >= 0 (standard deviation in 8-bit grey levels below which a patch is no evidence)"
        if not photo_ncc > 0.0:
            if int(photo_r) != int(EXPERIMENTAL_DEFAULTS["photo_window_cells"]):
                return "experimental['photo_window_cells'] is the window of the photo-consistency gate: it needs experimental['min_photo_ncc'] > 0"
            if photo_tex != float(EXPERIMENTAL_DEFAULTS["photo_min_texture"]):
                return "experimental['photo_min_texture'] is the texture floor of the photo-consistency gate: it needs experimental['min_photo_ncc'] > 0"
        else:
            if self.no_filter:
                return "experimental['min_photo_ncc'] is a filter: it cannot run with no_filter"
            if self.stream_output:
                return ("experimental['min_photo_ncc'] filters points held as arrays (xyz, rgb, cell, slot); stream_output writes 15-byte records "
                        "while the run proceeds")
            if self.exp("dense_tile_segments"):
                return "experimental['min_photo_ncc'] needs the ordered dense result; experimental['dense_tile_segments'] retires tiles unordered"
            if self.exchange_record_format() == "ply":
                return "experimental['min_photo_ncc'] filters f32 rows; experimental['exchange_records'] must be 'f32' with it"
        maps_dir = self.exp("depth_maps_dir")
        if not isinstance(maps_dir, str):
            return "experimental['depth_maps_dir'] must be a string (a directory for the per-camera depth maps; '' = off)"
        c_dm, r_dm, w_dm = self.exp("depth_map_cells"), self.exp("depth_map_splat_cells"), self.exp("depth_map_window_cells")
        integer = lambda v: not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, np.integer))      # noqa: E731
        if not integer(c_dm) or (int(c_dm) != 0 and not 8 <= int(c_dm) <= 4096):
            return "experimental['depth_map_cells'] must be 0 (automatic) or an integer in 8 .. 4096 (cells along the longer image side)"
        if not integer(r_dm) or not 0 <= int(r_dm) <= 3:
            return "experimental['depth_map_splat_cells'] must be an integer in 0 .. 3 (cells around a point's own that it is drawn into)"
        if not integer(w_dm) or not 0 <= int(w_dm) <= 8:
            return "experimental['depth_map_window_cells'] must be an integer in 0 .. 8 (cells around a cell in which nothing may be nearer; 0 = no test)"
        try:
            tol_dm = float(self.exp("depth_map_tol_rel"))
        except (TypeError, ValueError):
            return "experimental['depth_map_tol_rel'] must be a number (a relative depth, in (0, 1))"
        if isinstance(self.exp("depth_map_tol_rel"), (bool, np.bool_)) or not (0.0 < tol_dm < 1.0) or not (0.0 < float(np.float32(tol_dm)) < 1.0):
            return "experimental['depth_map_tol_rel'] must be in (0, 1) (a relative depth)"
        if maps_dir == "":
            for key, what in (("depth_map_cells", "plane size"), ("depth_map_splat_cells", "splat radius"), ("depth_map_window_cells", "visibility window"),
                              ("depth_map_tol_rel", "depth tolerance")):
                if float(self.exp(key)) != float(EXPERIMENTAL_DEFAULTS[key]):
                    return f"experimental['{key}'] is the {what} of the depth maps: it needs experimental['depth_maps_dir']"
        else:
            if self.stream_output:
                return ("experimental['depth_maps_dir'] renders the whole cloud, held as arrays; stream_output writes the file while the run proceeds "
                        "and keeps no cloud")
            if self.exchange_record_format() == "ply":
                return "experimental['depth_maps_dir'] renders f32 rows; experimental['exchange_records'] must be 'f32' with it"
            if self.exp("dense_tile_segments"):
                return ("experimental['depth_maps_dir'] needs the cloud as arrays; dense mode with experimental['dense_tile_segments'] retires tiles "
                        "into the file's records")
        thin = self.exp("footprint_thin_cells")
        if isinstance(thin, (bool, np.bool_)) or not isinstance(thin, (int, float, np.integer, np.floating)) or not np.isfinite(float(thin)) or float(thin) < 0.0:
            return ("experimental['footprint_thin_cells'] must be a finite number >= 0 (the cell of the thinning in match-grid cells of a point's own "
                    "reference camera; 0 = off)")
        if float(thin) > 0.0:
            if self.stream_output:
                return ("experimental['footprint_thin_cells'] has to see the whole cloud before anything is written; stream_output writes the file "
                        "while the run proceeds")
            if self.exchange_record_format() == "ply":
                return "experimental['footprint_thin_cells'] thins f32 rows; experimental['exchange_records'] must be 'f32' with it"
            if self.exp("dense_tile_segments"):
                return ("experimental['footprint_thin_cells'] needs the cloud as arrays with per-reference counts; dense mode with "
                        "experimental['dense_tile_segments'] retires tiles unordered")
        gain = self.exp("gain_compensation")
        if not isinstance(gain, str) or gain not in GAIN_MODES:
            return ("experimental['gain_compensation'] must be 'off', 'luma' (one exposure factor per image) or 'rgb' (one per image and "
                    "channel)")
        if gain != "off":
            if colour != "off":
                return ("experimental['gain_compensation'] cannot run with experimental['multiview_colour']: the blend would need each view's "
                        "factor before the solve exists; a two-pass driver is out of scope")
            if not (self.support_threshold() > 0.0):
                return ("experimental['gain_compensation'] takes the confirming views by the support filter's test: "
                        "experimental['support_thresh_px'] or, for its default, reproj_thresh must be > 0")
            if self.stream_output:
                return ("experimental['gain_compensation'] rewrites the colour of the collected cloud once the run's factors are solved; "
                        "stream_output writes 15-byte records while the run proceeds")
            if self.exp("dense_tile_segments"):
                return "experimental['gain_compensation'] needs the ordered dense result; experimental['dense_tile_segments'] retires tiles unordered"
            if self.exchange_record_format() == "ply":
                return "experimental['gain_compensation'] rewrites f32 rows; experimental['exchange_records'] must be 'f32' with it"
        far = self.exp("far_shell")
        if not isinstance(far, str) or far not in FAR_MODES:
            return ("experimental['far_shell'] must be 'off', 'file' (the shell in <output stem>_shell.ply) or 'merge' (its records behind the "
                    "cloud's in the main PLY)")
        number = lambda v: not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating)) and np.isfinite(float(v))  # noqa: E731
        whole = lambda v: not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, np.integer))      # noqa: E731
        if not number(self.exp("far_thresh_px")) or float(self.exp("far_thresh_px")) < 0.0:
            return "experimental['far_thresh_px'] must be a finite number >= 0 (px of the neighbour's camera image; 0 = reproj_thresh)"
        if not number(self.exp("far_certainty")) or not (0.0 < float(self.exp("far_certainty")) <= 1.0):
            return "experimental['far_certainty'] must be in (0, 1] (the raw certainty from which a neighbour is confident)"
        if not whole(self.exp("far_min_views")) or not 1 <= int(self.exp("far_min_views")) <= 8:
            return "experimental['far_min_views'] must be an integer in 1 .. 8 (confident neighbours a far cell needs)"
        if not whole(self.exp("far_shell_cells")) or not 8 <= int(self.exp("far_shell_cells")) <= 512:
            return "experimental['far_shell_cells'] must be an integer in 8 .. 512 (direction cells along a cube face's side)"
        if not whole(self.exp("far_min_samples")) or int(self.exp("far_min_samples")) < 1:
            return "experimental['far_min_samples'] must be an integer >= 1 (samples a direction cell needs to become a point)"
        if not number(self.exp("far_shell_radius")) or float(self.exp("far_shell_radius")) < 0.0:
            return "experimental['far_shell_radius'] must be a finite number >= 0 (scene units; 0 = automatic)"
        if far == "off":
            for key in FAR_KNOBS:
                if float(self.exp(key)) != float(EXPERIMENTAL_DEFAULTS[key]):
                    return f"experimental['{key}'] is a knob of the far-field shell: it needs experimental['far_shell'] = 'file' or 'merge'"
        else:
            if self.no_filter:
                return ("experimental['far_shell'] collects the cells the filters drop for want of parallax: with no_filter they are triangulated "
                        "and emitted at arbitrary depths already")
            if not (float(self.min_parallax_deg) > 0.0):
                return ("experimental['far_shell'] needs min_parallax_deg > 0: without the parallax gate the far cells also reach the cloud, at "
                        "depths nothing supports")
            if not (self.far_threshold() > 0.0):
                return "experimental['far_shell'] compares in pixels: experimental['far_thresh_px'] or, for its default, reproj_thresh must be > 0"
            if self.stream_output:
                return ("experimental['far_shell'] is placed around the finished cloud; stream_output writes the file while the run proceeds and "
                        "keeps no cloud")
            if self.exp("dense_tile_segments"):
                return ("experimental['far_shell'] needs the cloud as arrays; dense mode with experimental['dense_tile_segments'] retires tiles "
                        "into the file's records")
            if self.exchange_record_format() == "ply":
                return "experimental['far_shell'] measures the cloud's f32 rows; experimental['exchange_records'] must be 'f32' with it"
            if far == "merge":
                if self.exp("gaussian_init"):
                    return ("experimental['far_shell'] = 'merge' cannot run with experimental['gaussian_init']: a shell point has no neighbour "
                            "distance to take a scale from; use 'file'")
                if not str(self.output_path).lower().endswith(".ply"):
                    return "experimental['far_shell'] = 'merge' appends PLY records: output_path must end in .ply (use 'file' with other formats)"
        audit = self.exp("epipolar_audit")
        if not isinstance(audit, str) or audit not in AUDIT_MODES:
            return "experimental['epipolar_audit'] must be 'off' or 'report' (<output file>.audit.json and a warning per suspect camera)"
        if not number(self.exp("audit_certainty")) or not (0.0 < float(self.exp("audit_certainty")) <= 1.0):
            return "experimental['audit_certainty'] must be in (0, 1] (the raw certainty from which a match is counted)"
        if not whole(self.exp("audit_min_samples")) or int(self.exp("audit_min_samples")) < 1:
            return "experimental['audit_min_samples'] must be an integer >= 1 (confident matches a pair needs to be judged)"
        if not number(self.exp("audit_warn_px")) or float(self.exp("audit_warn_px")) < 0.0:
            return "experimental['audit_warn_px'] must be a finite number >= 0 (px of a camera image; 0 = reproj_thresh)"
        if not isinstance(self.exp("audit_maps_dir"), str):
            return "experimental['audit_maps_dir'] must be a string (a directory, relative to the output file's; '' = no maps)"
        if audit == "off":
            for key in AUDIT_KNOBS:
                if self.exp(key) != EXPERIMENTAL_DEFAULTS[key]:
                    return f"experimental['{key}'] is a knob of the epipolar audit: it needs experimental['epipolar_audit'] = 'report'"
        else:
            if not (self.audit_warn_threshold() > 0.0):
                return "experimental['epipolar_audit'] warns in pixels: experimental['audit_warn_px'] or, for its default, reproj_thresh must be > 0"
            if self.stream_output:
                return ("experimental['epipolar_audit'] is launched beside the point stages of a collected result; stream_output writes records "
                        "while the run proceeds and has no such site")
            if self.exp("dense_tile_segments"):
                return ("experimental['epipolar_audit'] is launched beside the ordered dense result; dense mode with "
                        "experimental['dense_tile_segments'] retires tiles into the file's records")
            if self.exchange_record_format() == "ply":
                return "experimental['epipolar_audit'] is launched beside f32 rows; experimental['exchange_records'] must be 'f32' with it"
        pose = self.exp("pose_refine")
        if not isinstance(pose, str) or pose not in POSE_MODES:
            return "experimental['pose_refine'] must be 'off' or 'report' (<output file>.poses.json: one corrected pose per camera)"
        if not number(self.exp("pose_certainty")) or not (0.0 < float(self.exp("pose_certainty")) <= 1.0):
            return "experimental['pose_certainty'] must be in (0, 1] (the raw certainty from which a match is counted)"
        if not number(self.exp("pose_inlier_px")) or not (0.0 < float(self.exp("pose_inlier_px")) <= 64.0):
            return "experimental['pose_inlier_px'] must be in (0, 64] (px of the neighbour's camera image from the epipolar line)"
        if not whole(self.exp("pose_min_samples")) or int(self.exp("pose_min_samples")) < 1:
            return "experimental['pose_min_samples'] must be an integer >= 1 (inliers a pair needs to enter the solve)"
        if not isinstance(self.exp("pose_corrections"), str):
            return "experimental['pose_corrections'] must be a string (the path of a poses.json; '' = none)"
        if pose == "off":
            for key in POSE_KNOBS:
                if self.exp(key) != EXPERIMENTAL_DEFAULTS[key]:
                    return f"experimental['{key}'] is a knob of the pose refinement: it needs experimental['pose_refine'] = 'report'"
        else:
            if self.stream_output:
                return ("experimental['pose_refine'] is launched beside the point stages of a collected result; stream_output writes records "
                        "while the run proceeds and has no such site")
            if self.exp("dense_tile_segments"):
                return ("experimental['pose_refine'] is launched beside the ordered dense result; dense mode with "
                        "experimental['dense_tile_segments'] retires tiles into the file's records")
            if self.exchange_record_format() == "ply":
                return "experimental['pose_refine'] is launched beside f32 rows; experimental['exchange_records'] must be 'f32' with it"
        if self.stream_output:
            if not str(self.output_path).lower().endswith(".ply"):
                return "stream_output writes a PLY while the run proceeds: output_path must end in .ply"
            if int(self.max_points) > 0:
                return "stream_output cannot be combined with max_points: the point cap has to see the whole cloud before anything is written"
            if float(self.voxel_size) > 0.0:
                return "stream_output cannot be combined with voxel_size: the voxel filter has to see the whole cloud before anything is written"
        if self.device_image_prep and self.backend != "device":
            return "device_image_prep resizes the images with the HIP kernels: it needs backend='device'"
        if dense and self.selection_backend == "host":
            return "selection_backend='host' names where the coverage sampling of the sampled mode runs; dense mode has no sampling stage"
        if not dense and int(self.refs_per_launch) > 1:
            if self.backend != "device" or self.selection_backend != "device":
                return ("refs_per_launch > 1 in sampled mode puts several references into one fused device call: it needs backend='device' and "
                        "selection_backend='device'")
        if not self.upstream_normaliser and not dense and (self.selection_backend == "host" or self.backend == "host"):
            return ("upstream_normaliser=False asks for the device selection's exact weight sum; the host selection stage "
                    "(selection_backend='host' or backend='host') always normalises with torch's own sum, as upstream does")
        if self.exp("dense_tile_segments"):
            if not dense:
                return "experimental['dense_tile_segments'] is a form of the dense kernel: it needs triangulation_mode='dense'"
            if self.backend != "device":
                return "experimental['dense_tile_segments'] is a form of the HIP kernel: it needs backend='device'"
        if float(self.exp("exchange_replicate")) > 0.0:
            if not self.exp("exchange_overlap"):
                return "experimental['exchange_replicate'] needs the overlapped exchange (experimental['exchange_overlap'])"
            if self.stream_output:
                return "experimental['exchange_replicate'] cannot be combined with stream_output: a streamed sharded run sends every reference to the writer"
        if self.exp("stream_shared_file") and not self.stream_output:
            return "experimental['stream_shared_file'] is a form of the streamed output: it needs stream_output"
        if self.exp("exchange_records") == "ply":
            if not self.exp("exchange_overlap"):
                return "experimental['exchange_records']='ply' is a format of the overlapped exchange (experimental['exchange_overlap'])"
            if self.stream_output:
                return ("experimental['exchange_records']='ply' cannot be combined with stream_output: a streamed sharded run exchanges its result "
                        "once, at the end, as f32 rows")
        return None

    def validate(self) -> None:
        msg = self.problem()
        if msg:
            raise ValueError(msg)


# Settings that were dataclass fields of this package before its round-5 layout and live in ``experimental`` now: still accepted as keywords and
# still readable as attributes (both with a DeprecationWarning), so that a caller written against the older surface keeps running.
_MOVED_TO_EXPERIMENTAL = ("exchange_overlap", "exchange_round", "exchange_records", "exchange_replicate", "stream_shared_file",
                          "dense_tile_segments", "upstream_fundamental")


def _accept_moved_settings(cls):
    import functools
    import warnings
    plain_init = cls.__init__

    @functools.wraps(plain_init)
    def __init__(self, *args, **kwargs):
        moved = {k: kwargs.pop(k) for k in _MOVED_TO_EXPERIMENTAL if k in kwargs}
        if moved:
            warnings.warn(f"DensePipelineConfig({', '.join(moved)}=...) moved to experimental={{...}}", DeprecationWarning, stacklevel=2)
            kwargs["experimental"] = {**moved, **dict(kwargs.get("experimental") or {})}
        plain_init(self, *args, **kwargs)

    cls.__init__ = __init__
    for name in _MOVED_TO_EXPERIMENTAL:
        def getter(self, _n=name):
            warnings.warn(f"DensePipelineConfig.{_n} moved to experimental[{_n!r}] (config.exp({_n!r}))", DeprecationWarning, stacklevel=2)
            return self.exp(_n)
        setattr(cls, name, property(getter))
    return cls


DensePipelineConfig = _accept_moved_settings(DensePipelineConfig)


@dataclasses.dataclass
class CameraRecord:
    uid: int
    image_path: str
    width: int
    height: int
    K: np.ndarray
    R: np.ndarray
    t: np.ndarray
    P: np.ndarray
    C: np.ndarray
    mask_path: Optional[str] = None
    # (fx, fy, cx, cy) + the eight coefficients (k1, k2, p1, p2, k3, k4, k5, k6) of the camera model in f64, as COLMAP stores them, or None:
    # what experimental['undistort_images'] resamples the image through.  ``K`` above stays the f32 pinhole part.
    distortion: Optional[Tuple[float, ...]] = None
    distortion_model: Optional[str] = None          # COLMAP's name of the model, kept so that an unsupported one can be named

    def active_distortion(self) -> Optional[Tuple[float, ...]]:
        """``distortion`` when any of its eight coefficients is not zero, else None: a camera without them is a pinhole camera already."""
        d = self.distortion
        return tuple(d) if d is not None and any(float(v) != 0.0 for v in d[4:]) else None

    def flat_pose(self) -> np.ndarray:
        """Row-major 4x4 world-to-camera matrix as a 16-vector (f64), the feature used for
        k-centres reference selection and nearest-neighbour lookup (upstream
        core/camera_models.py:23-28)."""
        pose = np.eye(4)
        pose[:3, :3] = self.R
        pose[:3, 3] = np.asarray(self.t).reshape(3)
        return pose.reshape(-1)

    @staticmethod
    def from_krt(uid: int, K, R, t, width: int, height: int, image_path: str = "",
                 mask_path: Optional[str] = None) -> "CameraRecord":
        """Build a record the way both upstream entry points do (densify.py:59-88,215-245):
        f32 ``K,R,t``; ``P = K @ [R|t]`` and ``C = -R^T t`` evaluated in f32."""
        K = np.asarray(K, np.float32).reshape(3, 3)
        R = np.asarray(R, np.float32).reshape(3, 3)
        t = np.asarray(t, np.float32).reshape(3, 1)
        P = K @ np.concatenate([R, t], axis=1)
        C = (-R.T @ t).reshape(3)
        return CameraRecord(uid=int(uid), image_path=image_path, width=int(width), height=int(height),
                            K=K, R=R, t=t, P=P, C=C, mask_path=mask_path)
