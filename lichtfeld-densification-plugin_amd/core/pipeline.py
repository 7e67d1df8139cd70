"""Dense-initialisation pipeline driver with the per-reference hot path on the GPU.

Drop-in for upstream ``core/pipeline.py::run_dense_pipeline`` (:783-928): same signature, same
callbacks, same result type, same exceptions.  What changes is where the work happens:

    upstream                                     here
    --------------------------------------       ----------------------------------------------
    RoMa outputs copied to the host, sync        stay on the GPU, consumed in place
    _collect_reference_matches epilogue (CPU)    folded into the HIP kernels (floor, masks)
    _triangulate_ref (torch-CPU + NumPy)         lfd_aggregate + lfd_triangulate_indexed  ("sampled")
                                                 or lfd_triangulate_dense                 ("dense")
    4 pack threads, completion order             ordered prefetch (results do not depend on timing)

The driver is four parts, each in a module of its own:
    core/packing.py     load / decode one reference and its neighbours; the ordered prefetcher
    core/hotpath.py     the per-run context of the C-ABI and the calls that triangulate a reference
    core/strategies.py  SampledLoop | DenseBatcher | DensePlyStreamer: how matched references are scheduled onto the hot path
    core/sinks.py       RunOutputs: accumulator, previews, streamed file, debug previews, the sharded run's exchange; PipelineResult
and this file is the loop that connects them (``run_dense_pipeline``).

Two triangulation modes (``DensePipelineConfig.triangulation_mode``):
  * "sampled" (default) reproduces upstream: coverage sampling picks ~0.85*M + <=625 cells per
    reference from the aggregated certainty, those cells are triangulated and emitted in upstream's
    per-neighbour group order.  With ``per_reference_rng=False`` and one GPU the legacy NumPy stream
    is consumed exactly as upstream consumes it (one stream, reference after reference).
  * "dense" sends every grid cell through the fused kernel (survivors in raster order per reference).

Multi-GPU: when ``torch.distributed`` is initialised with world_size > 1 the reference list is dealt
round-robin to the ranks and the survivors are exchanged in reference order
(core/distributed.py); sampling then uses one RNG stream per reference.
"""
from __future__ import annotations

import dataclasses
import gc
import os
import time
from typing import Callable, List, Optional

import numpy as np
import torch

from . import distributed as lfd_dist
from . import hip_backend as hb
from .debug_viz import MatchDebugState
from .hostlog import log
from .hotpath import HotPath
from .matcher import RomaMatcher, has_cached_romav2_weights, romav2_cached_weights_paths
from .packing import OrderedPrefetcher, PackedReference, PipelineCancelled, cancelled, pack_reference, raise_if_cancelled
from .scheduler import FeatureCache, PairSchedule
from .sinks import PipelineResult, RunOutputs, ShardPlan
from .stages import NULL_CLOCK
from .strategies import DenseBatcher, DensePlyStreamer, Matched, SampledLoop, reference_seed
from .types import CameraRecord, DensePipelineConfig

_HotPath = HotPath                       # (the name tests and profiles patch)
_reference_seed = reference_seed


def _estimate_total_pairs(refs_local, nn_table, uids, nns_per_ref) -> int:
    return sum(sum(1 for n in nn_table[r][:nns_per_ref] if uids[n] != uids[r]) for r in refs_local)


def _resolve_backend(config: DensePipelineConfig, backend: Optional[str], device):
    """(config with the effective backend, torch device).  A "device" run without a GPU raises: it never turns into a host run."""
    if backend is not None and str(backend) != config.backend:
        if backend not in ("device", "host"):
            raise ValueError("backend must be 'device' or 'host'")
        config = dataclasses.replace(config, backend=str(backend))        # (validated again: device-only settings on the host backend raise)
    if config.backend == "host":
        return config, torch.device("cpu")
    if not torch.cuda.is_available():
        raise hb.HipBackendError("no GPU visible: the dense-initialisation hot path has no CPU fallback "
                                 "(backend=\"host\" selects the CPU twin explicitly)")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise hb.HipBackendError(f"backend=\"device\" needs a cuda (HIP) device, got {dev}")
    return config, dev


def _make_matcher(config, dev, progress_callback):
    """upstream core/pipeline.py:795-812: the progress text depends on whether the weights are cached"""
    cached = has_cached_romav2_weights()
    _announce(progress_callback, cached)
    if not cached:
        log.info("RoMaV2 weights not found in cache; expected cache paths: " + ", ".join(romav2_cached_weights_paths()))
    matcher = RomaMatcher(device=str(dev), mode="outdoor", setting=config.roma_setting, pairs_per_forward=int(config.pairs_per_forward),
                          fused_local_corr=bool(config.exp("fused_local_corr")),
                          fused_refiner_blocks=bool(config.exp("fused_refiner_blocks")),
                          fused_refiner_head=bool(config.exp("fused_refiner_head")))
    if float(config.exp("cycle_thresh_px")) > 0.0:       # (a matcher built here starts with the backward warp off)
        matcher.set_backward_warp(True)
    if _wants_precision(config):                         # (... and hands out no precision planes)
        matcher.set_precision(True)
    if not cached and progress_callback is not None:
        progress_callback(10.0, "RoMa v2 model installation complete. Starting matching...")
    return matcher


def _wants_precision(config) -> bool:
    """Does the run read RoMa-v2's precision planes?  The weighted re-triangulation does, and the depth-uncertainty gate unless
    it is given an isotropic match noise."""
    return bool(config.exp("precision_weighted_refine")) or (float(config.exp("max_depth_sigma_rel")) > 0.0
                                                             and float(config.exp("match_sigma_px")) == 0.0)


def _announce(progress_callback, cached: bool) -> None:
    msg = "Initializing RoMa v2 model..." if cached else "Installing model weights..."
    if progress_callback is not None:
        progress_callback(10.0, msg)
    log.info(msg)


def _plan_undistortion(camera_records, refs_local, nn_table, config) -> bool:
    """What experimental['undistort_images'] means for this run, decided before anything is matched: True when images are
    going to be undistorted.  Knob on: a selected camera - a reference or one of the neighbours it loads - whose model the undistortion does
    not support, or whose image is not of the calibration's size, stops the run by name; no camera with distortion coefficients: one info
    line, nothing else happens.  Knob off: one warning when any camera's coefficients are being ignored."""
    distorted = [c for c in camera_records if c.active_distortion() is not None]
    if not bool(config.exp("undistort_images")):
        if distorted:
            log.warn(f"{len(distorted)} of {len(camera_records)} cameras have non-zero distortion coefficients ({distorted[0].distortion_model}): distortion "
                     "is ignored, the images are matched as they are and triangulated as pinhole images; experimental['undistort_images'] "
                     "(--undistort_images) undistorts them first")
        return False
    selected = sorted({int(r) for r in refs_local} | {int(n) for r in refs_local for n in nn_table[int(r)][:int(config.nns_per_ref)]})
    for i in selected:
        cam = camera_records[i]
        if cam.distortion is None and cam.distortion_model is not None:
            raise RuntimeError(f"experimental['undistort_images'] supports the camera models SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, RADIAL, OPENCV and "
                               f"FULL_OPENCV; image {cam.image_path} has a {cam.distortion_model} camera")
    if not distorted:
        log.info("experimental['undistort_images']: no camera carries distortion coefficients; the images are used as they are")
        return False
    from PIL import Image
    for i in selected:
        cam = camera_records[i]
        if cam.active_distortion() is None:
            continue
        try:
            with Image.open(cam.image_path) as im:          # (the header alone)
                size = tuple(im.size)
        except OSError:
            continue                                        # (an unreadable image is the loader's warning, as without the knob)
        if size != (int(cam.width), int(cam.height)):
            raise RuntimeError(f"experimental['undistort_images'] needs every image at the size its camera was calibrated at: image {cam.image_path} "
                               f"is {size[0]} x {size[1]}, its {cam.distortion_model} camera {int(cam.width)} x {int(cam.height)}")
    return True


def _match_reference(local_i: int, packed: PackedReference, matcher, hot: HotPath, outputs: RunOutputs, feat_cache, size_wh, want_debug: bool,
                     cancel) -> Optional[Matched]:
    """One package through the matcher (upstream core/pipeline.py:856-872): prepared on the device first when it came decoded; the maps stay
    where the matcher left them."""
    from PIL import Image
    dev, clock = hot.dev, hot.clock
    dev_images = bool(getattr(matcher, "accepts_device_images", False))
    if packed.raw:
        packed = hot.prepare_on_device(packed, size_wh, need_host=want_debug or not dev_images)
    kw_keys = {"keys": (packed.ref_index, list(packed.nbr_indices))} if feat_cache is not None else {}
    with clock.stage("match"):
        if packed.dev is not None and dev_images:
            results = matcher.match_grids_batch(packed.dev["image"], list(packed.dev["nbr_images"]), **kw_keys)
        else:
            results = matcher.match_grids_batch(Image.fromarray(np.ascontiguousarray(packed.image)),
                                                [Image.fromarray(np.ascontiguousarray(a)) for a in packed.nbr_images], **kw_keys)
        if feat_cache is not None:
            feat_cache.advance(local_i)
        raise_if_cancelled(cancel)
        if not results:
            return None
        first_pair = outputs.note_pairs(local_i, len(results))
        warps = [_as_device_map(r[0], dev) for r in results]
        certs = [_as_device_map(r[1], dev) for r in results]
    H, W = certs[0].shape
    outputs.match_grid = (int(H), int(W))
    axes = None
    ax = getattr(matcher, "reference_axes", None)
    if warps[0].shape[-1] == 2 and callable(ax):
        a0, a1 = ax(H, W)
        axes = (torch.as_tensor(a0).to(dev, torch.float32).contiguous(), torch.as_tensor(a1).to(dev, torch.float32).contiguous())
    if hot.cycle_thresh_px > 0.0:
        # forward-backward filter: the certainty planes are gated in place, right behind the matcher on its stream; everything downstream
        # sees a rejected cell as one mask_b masked out
        if any(len(r) < 3 for r in results):
            raise RuntimeError(f"experimental['cycle_thresh_px'] is set but {type(matcher).__name__}.match_grids_batch returned no backward warp")
        hot.cycle_gate(warps, certs, [_as_device_map(r[2], dev) for r in results], axes)
    precision = None
    if hot.refine_weighted or hot.sigma_planes:
        # RoMa-v2's precision planes: element 3 of the matcher's tuples, read in place by the weighted re-triangulation and by
        # the depth-uncertainty gate
        if any(len(r) < 4 or r[3] is None for r in results):
            knob = "precision_weighted_refine" if hot.refine_weighted else "max_depth_sigma_rel"
            raise RuntimeError(f"experimental['{knob}'] is set but "
                               f"{type(matcher).__name__}.match_grids_batch returned no precision plane")
        precision = [_as_device_map(r[3], dev) for r in results]
    return Matched(local_i, packed, hot.inputs(packed, warps, certs, precision), axes, int(H), int(W), first_pair, want_debug)


def _as_device_map(t, dev) -> torch.Tensor:
    """A matcher output as the contiguous f32 tensor on ``dev`` the kernels read in place - which it normally already is (no call, no copy then)."""
    if isinstance(t, torch.Tensor) and t.device == dev and t.dtype == torch.float32 and t.is_contiguous() and not t.requires_grad:
        return t
    return torch.as_tensor(t).detach().to(dev, torch.float32).contiguous()


def _make_strategy(config, plan: ShardPlan, hot: HotPath, outputs: RunOutputs, per_ref_rng: bool, debug_state, auto_group: bool = False):
    """``auto_group``: refs_per_launch was 0 - the strategy bounds the automatic group by the bytes its buffers take at the run's grid."""
    debug_on = debug_state is not None and debug_state.is_enabled()
    if DensePlyStreamer.applies(config, plan, hot.on_host, outputs, debug_on):
        return DensePlyStreamer(hot, outputs, config, auto_group)
    if config.triangulation_mode == "dense":
        return DenseBatcher(hot, outputs, config, auto_group)
    return SampledLoop(hot, outputs, config, per_ref_rng, auto_group)


def run_dense_pipeline(
    camera_records: List[CameraRecord],
    refs_local: List[int],
    nn_table: np.ndarray,
    config: DensePipelineConfig,
    progress_callback: Optional[Callable[[float, str], None]] = None,
    on_sequential_viz: Optional[Callable[[str], None]] = None,
    debug_state: Optional[MatchDebugState] = None,
    cancel_requested: Optional[Callable[[], bool]] = None,
    *,
    matcher=None,
    densifier: Optional[hb.HipDensifier] = None,
    device: Optional[torch.device] = None,
    backend: Optional[str] = None,
    stage_clock=None,
) -> PipelineResult:
    """See module docstring.  ``matcher`` / ``densifier`` / ``device`` are injection points for
    tests and for callers that keep a warm model; by default a RomaMatcher is created (and released)
    per run exactly like upstream.  ``backend`` ("device" | "host", default ``config.backend``): "host" runs the per-reference
    path on the CPU twin of the C-ABI (HostDensifier + core/sampling.py) - upstream's CPU-only configuration, chosen by the
    caller; a "device" run without a GPU raises HipBackendError, it never turns into a host run.  ``stage_clock``: a
    core.stages.StageClock that receives the run's time per stage (``PipelineResult.stages``)."""
    import torch.distributed as dist
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    rank = dist.get_rank() if world > 1 else 0
    config.validate()
    if world > 1 and bool(config.exp("estimate_normals")):
        # (a condition of the world, not of the configuration: every rank sees it and stops here, before anything is set up)
        raise ValueError("experimental['estimate_normals'] cannot run sharded over several GPUs: the exchange of a sharded run does not carry the "
                         "normals (rows of xyz, rgb, err or 15-byte records)")
    if world > 1 and str(config.exp("multiview_colour")) != "off":
        raise ValueError("experimental['multiview_colour'] cannot run sharded over several GPUs: like the normals it is a stage of the single-GPU "
                         "run, and the sharded schedules have not been taken through it")
    if world > 1 and float(config.exp("min_photo_ncc")) > 0.0:
        raise ValueError("experimental['min_photo_ncc'] cannot run sharded over several GPUs: like the multi-view colour it is a stage of the "
                         "single-GPU run, and the sharded schedules have not been taken through it")
    if world > 1 and str(config.exp("gain_compensation")) != "off":
        raise ValueError("experimental['gain_compensation'] cannot run sharded over several GPUs: like the multi-view colour it is a stage of the "
                         "single-GPU run, and the exchange of a sharded run does not carry the statistics")
    if world > 1 and str(config.exp("far_shell")) != "off":
        raise ValueError("experimental['far_shell'] cannot run sharded over several GPUs: the direction table is a statistic of the single-GPU "
                         "run, and the exchange of a sharded run does not carry it")
    if world > 1 and str(config.exp("epipolar_audit")) != "off":
        raise ValueError("experimental['epipolar_audit'] cannot run sharded over several GPUs: the histograms are a statistic of the single-GPU "
                         "run, and the exchange of a sharded run does not carry them")
    if world > 1 and str(config.exp("pose_refine")) != "off":
        raise ValueError("experimental['pose_refine'] cannot run sharded over several GPUs: the normal equations are a statistic of the single-GPU "
                         "run, and the exchange of a sharded run does not carry them")
    if world > 1 and str(config.exp("depth_maps_dir")) != "":
        raise ValueError("experimental['depth_maps_dir'] cannot run sharded over several GPUs: the maps are a stage of the single-GPU run, and with "
                         "gather_to_root only one rank would hold the cloud they are rendered from")
    if world > 1 and float(config.exp("footprint_thin_cells")) > 0.0:
        raise ValueError("experimental['footprint_thin_cells'] cannot run sharded over several GPUs: the thinning is a stage of the single-GPU run, and "
                         "with gather_to_root only one rank would hold the cloud and the per-reference counts it works on")
    if world > 1 and int(config.exp("min_component_points")) > 0:
        raise ValueError("experimental['min_component_points'] cannot run sharded over several GPUs: the filter is a stage of the single-GPU run, and "
                         "with gather_to_root only one rank would hold the cloud and the per-reference counts it works on")
    config, dev = _resolve_backend(config, backend, device)
    per_ref_rng = bool(config.per_reference_rng) or world > 1
    # refs_per_launch = 0 (the default): several references per launch where the results do not depend on it and nobody watches the run proceed
    previews = (on_sequential_viz is not None and int(config.viz_interval) > 0) or debug_state is not None
    auto_group = int(config.refs_per_launch) == 0
    if int(config.refs_per_launch) != config.launch_group(world, previews):
        config = dataclasses.replace(config, refs_per_launch=config.launch_group(world, previews))
    clock = stage_clock if stage_clock is not None else NULL_CLOCK
    undistort = _plan_undistortion(camera_records, refs_local, nn_table, config)
    uids = [c.uid for c in camera_records]
    total_pairs_est = _estimate_total_pairs(refs_local, nn_table, uids, config.nns_per_ref)
    if debug_state:
        debug_state.set_total_pairs(total_pairs_est)
    # What a sharded run exchanges while it proceeds is decided from the configuration and the world ALONE and set up here, before anything
    # can fail: every rank then reaches the matching finish() in `finally` whatever went wrong on it (core/sinks.py::ShardLink).
    plan = ShardPlan.make(config, len(refs_local), world, rank)
    outputs = RunOutputs(config, plan, dist, dev, camera_records, on_sequential_viz=on_sequential_viz, debug_state=debug_state,
                         cancel_requested=cancel_requested, total_pairs_est=total_pairs_est)
    t0 = time.time()
    own_matcher = matcher is None
    prefetch = hot = feat_cache = strategy = gain_rows = far_shell = epipolar_audit = pose_refine = None
    rank_status, rank_error = 0, None         # 0 fine, 1 cancelled, 2 failed: agreed on by all ranks before the exchange step (core/distributed.py)
    try:
        if own_matcher:
            matcher = _make_matcher(config, dev, progress_callback)
        else:
            # an injected matcher: the knob is handed to it, or refused - never ignored
            if bool(getattr(matcher, "supports_fused_local_corr", False)):
                matcher.set_fused_local_corr(bool(config.exp("fused_local_corr")))
            elif config.exp("fused_local_corr"):
                raise ValueError("experimental['fused_local_corr'] asks the matcher to run RoMa-v2's local correlation in the HIP kernel, but the "
                                 f"injected matcher ({type(matcher).__name__}) does not declare supports_fused_local_corr")
            if bool(getattr(matcher, "supports_fused_refiner_blocks", False)):
                matcher.set_fused_refiner_blocks(bool(config.exp("fused_refiner_blocks")))
            elif config.exp("fused_refiner_blocks"):
                raise ValueError("experimental['fused_refiner_blocks'] asks the matcher to run the conv blocks of RoMa-v2's refiners in the HIP kernel, "
                                 f"but the injected matcher ({type(matcher).__name__}) does not declare supports_fused_refiner_blocks")
            if bool(getattr(matcher, "supports_fused_refiner_head", False)):
                matcher.set_fused_refiner_head(bool(config.exp("fused_refiner_head")))
            elif config.exp("fused_refiner_head"):
                raise ValueError("experimental['fused_refiner_head'] asks the matcher to run the output head of RoMa-v2's refiners in the HIP kernel, "
                                 f"but the injected matcher ({type(matcher).__name__}) does not declare supports_fused_refiner_head")
            if bool(getattr(matcher, "supports_backward_warp", False)):
                matcher.set_backward_warp(float(config.exp("cycle_thresh_px")) > 0.0)
            elif float(config.exp("cycle_thresh_px")) > 0.0:
                raise ValueError("experimental['cycle_thresh_px'] asks for the forward-backward filter, which needs the matcher's backward warp, but the "
                                 f"injected matcher ({type(matcher).__name__}) does not declare supports_backward_warp")
            if bool(getattr(matcher, "supports_precision", False)):
                matcher.set_precision(_wants_precision(config))
            elif config.exp("precision_weighted_refine"):
                raise ValueError("experimental['precision_weighted_refine'] asks for the precision-weighted re-triangulation, which needs the matcher's "
                                 f"precision planes, but the injected matcher ({type(matcher).__name__}) does not declare supports_precision")
            elif _wants_precision(config):
                raise ValueError("experimental['max_depth_sigma_rel'] without experimental['match_sigma_px'] takes the match noise from the matcher's "
                                 f"precision planes, but the injected matcher ({type(matcher).__name__}) does not declare supports_precision")
            _announce(progress_callback, True)
        raise_if_cancelled(cancel_requested)
        size_wh = (int(matcher.w_resized), int(matcher.h_resized))
        hot = HotPath(camera_records, config, float(matcher.sample_thresh), size_wh[0], size_wh[1], dev, densifier, clock=clock)
        if not hot.on_host:
            hot.dens.seed_rng(int(config.seed))      # upstream: np.random.seed(config.seed) (core/pipeline.py:793); the host backend draws from its own RandomState
        # N4: every camera's backbone features once per run, kept exactly until their last use (core/scheduler.py)
        schedule = PairSchedule(refs_local, nn_table, uids, config.nns_per_ref, positions=plan.my_positions)
        if bool(getattr(matcher, "supports_feature_keys", False)):
            feat_cache = FeatureCache(schedule.last_use) if config.share_features else None
            matcher.set_feature_cache(feat_cache)    # always (re)set: an injected, warm matcher may still hold the cache of an earlier run
        stage = (lambda ci, im, mk: hot.stage_decoded(ci, size_wh, im, mk)) if config.device_image_prep else None
        jobs = [(lambda p=p: pack_reference(p, refs_local[p], camera_records, nn_table, config.nns_per_ref, size_wh, cancel_requested,
                                            raw=bool(config.device_image_prep), stage=stage, undistort=undistort)) for p in plan.my_positions]
        # (upstream's `prefetch_packages` bounds the queue of FINISHED packages while all of its workers keep loading: the look-ahead here is at
        # least one package per worker, so that none of them idles)
        prefetch = OrderedPrefetcher(jobs, workers=int(config.pack_workers), window=max(int(config.prefetch_packages), int(config.pack_workers)), clock=clock)
        outputs.open()
        strategy = _make_strategy(config, plan, hot, outputs, per_ref_rng, debug_state, auto_group)
        total_refs = len(plan.my_positions)
        for local_i, packed in enumerate(prefetch):
            raise_if_cancelled(cancel_requested)
            if progress_callback is not None:
                done = local_i + 1
                progress_callback(10.0 + (float(done - 1) / max(1, total_refs)) * 80.0,
                                  f"Matching {done}/{total_refs} | {done / max(0.001, time.time() - t0):.1f} it/s")
            if packed is None:
                if feat_cache is not None:
                    feat_cache.advance(local_i)       # a skipped reference is a schedule position too: its cameras' last uses pass
                continue
            raise_if_cancelled(cancel_requested)
            want_debug = debug_state is not None and debug_state.is_enabled()
            m = _match_reference(local_i, packed, matcher, hot, outputs, feat_cache, size_wh, want_debug, cancel_requested)
            if m is not None:
                strategy.submit(m)
        strategy.drain()
        if hot.cycle_thresh_px > 0.0:
            cells, rejected = hot.cycle_totals()
            log.info(f"Forward-backward filter: threshold {hot.cycle_thresh_px:g} px, {cells} cells, {100.0 * rejected / max(1, cells):.2f} % rejected")
        if hot.min_support > 0:
            n_in, n_dropped = hot.support_totals()
            log.info(f"Multi-view support filter: threshold {hot.support_thresh_px:g} px, at least {hot.min_support} other view(s), {n_in} points in, "
                     f"{n_dropped} dropped")
        if hot.refine:
            totals = hot.refine_totals()
            n_refined, n_fallback = totals[:2]
            log.info(f"Multi-view re-triangulation: threshold {hot.support_thresh_px:g} px, {n_refined} points refined, {n_fallback} confirmed points "
                     f"kept their two-view position")
        if hot.refine and hot.refine_weighted:
            log.info(f"Precision-weighted re-triangulation: {n_refined} points refined, {n_fallback} confirmed points kept their two-view position, "
                     f"{totals[2]} points solved with weighted rows")
        if hot.max_sigma > 0.0:
            n_in, n_kept = hot.sigma_totals()
            noise = f"isotropic match noise {hot.iso_sigma_px:g} px" if hot.iso_sigma_px > 0.0 else "the matcher's precision planes"
            log.info(f"Depth-uncertainty gate: relative depth sigma at most {hot.max_sigma:g} ({noise}), {n_in} points in, {n_kept} kept")
        if hot.photo:
            n_guard, n_sparse, n_flat, n_ok, n_refuted = hot.photo_totals()
            log.info(f"Photo-consistency gate: ZNCC at least {hot.photo_ncc:g} over {2 * hot.photo_window + 1} x {2 * hot.photo_window + 1} cells, "
                     f"texture floor {hot.photo_texture:g} grey levels: {n_guard} points guarded, {n_sparse} with under half a window, {n_flat} "
                     f"untextured, {n_ok} consistent, {n_refuted} refuted and dropped")
        if hot.colour:
            n_col, n_views = hot.colour_totals()
            log.info(f"Multi-view colour: {hot.colour_mode} over the confirming views (within {hot.support_thresh_px:g} px), {n_col} points blended, "
                     f"{(n_views / n_col if n_col else 0.0):.2f} views per point")
        if hot.gain:
            gain_rows = hot.gain_rows()
            log.info(f"Gain compensation: {int(gain_rows.table[:, 0].sum())} samples in {int((gain_rows.table[:, 0] > 0).sum())} of "
                     f"{gain_rows.table.shape[0]} (reference, neighbour) rows (within {hot.support_thresh_px:g} px)")
        if hot.far:
            far_shell = hot.far_result()
            t6 = far_shell["table"][:, 6]
            log.info(f"Far-field shell: {sum(far_shell['far_cells'].values())} far cells (every confident neighbour within {hot.far_thresh_px:g} px of "
                     f"the rotation-only transfer, certainty >= {hot.far_certainty:g}) in {int((t6 > 0).sum())} of {t6.numel()} direction cells, "
                     f"{far_shell['overlap']} of them also produced a point")
        if hot.audit:
            from . import audit as audit_report
            epipolar_audit = hot.audit_result()
            names = {int(c.uid): os.path.basename(str(c.image_path)) for c in camera_records}
            epipolar_audit["report"] = audit_report.build_report(epipolar_audit["rows"], names, int(config.exp("audit_min_samples")),
                                                                 config.audit_warn_threshold(), hot.audit_certainty)
        if hot.pose:
            from . import poses as pose_report
            pose_refine = hot.pose_result()
            names = {int(c.uid): os.path.basename(str(c.image_path)) for c in camera_records}
            pose_refine["report"] = pose_report.build_report(pose_refine["rows"], camera_records, int(config.exp("pose_min_samples")),
                                                             hot.pose_certainty, hot.pose_inlier_px, names)
        if hot.normals:
            n_fit, n_fell = hot.normal_totals()
            log.info(f"Surface normals: window radius {hot.normal_radius} cell(s), depth step {hot.normal_depth_step:g}, {n_fit} points fitted, "
                     f"{n_fell} with the view vector instead")
    except BaseException as exc:
        if world == 1:
            raise
        # sharded run: the other ranks are heading for the collectives below; tell them instead of leaving them blocked
        rank_status, rank_error = (1 if isinstance(exc, PipelineCancelled) else 2), exc
    finally:
        failed = _release(prefetch, strategy, feat_cache, matcher if own_matcher else None, matcher, outputs, hot, debug_state)
        if failed is not None and rank_status == 0:
            rank_status, rank_error = 2, failed

    if world > 1:
        if rank_status == 0 and cancelled(cancel_requested):
            rank_status = 1
        worst = lfd_dist.agree_on_status(rank_status, dist, dev)
        if worst:
            if rank_error is not None:
                raise rank_error
            raise PipelineCancelled("Cancelled") if worst == 1 else RuntimeError("dense pipeline failed on another rank")
    else:
        raise_if_cancelled(cancel_requested)
    if progress_callback:
        progress_callback(90.0, "Finalizing triangulation...")
    result = outputs.result(t0, clock)
    result.gain_rows = gain_rows          # experimental['gain_compensation']: the run's statistics, for the solve (densify.py)
    result.far_shell = far_shell          # experimental['far_shell']: the run's direction table, for the shell (densify.py)
    result.epipolar_audit = epipolar_audit      # experimental['epipolar_audit']: the pairs' histograms, the report and the cell maps (densify.py)
    result.pose_refine = pose_refine            # experimental['pose_refine']: the pairs' normal equations and the report (densify.py)
    return result


def _release(prefetch, strategy, feat_cache, own_matcher, matcher, outputs: RunOutputs, hot, debug_state) -> Optional[BaseException]:
    """The run's ``finally`` (upstream core/pipeline.py:900-907 + what a sharded run owes its peers).  Returns a failure of the exchange."""
    if prefetch is not None:
        prefetch.close()
    if strategy is not None:
        strategy.close()
    if feat_cache is not None:           # the features of this run's cameras: nothing of them outlives the run
        feat_cache.clear()
        try:
            matcher.set_feature_cache(None)
        except Exception as exc:
            log.warn(f"Releasing the feature cache failed: {exc}")
    if own_matcher is not None:
        try:
            own_matcher.close()
        except Exception as exc:
            log.warn(f"Matcher cleanup failed: {exc}")
    failed = outputs.finish()
    if hot is not None:
        hot.close()
    if debug_state:
        debug_state.release_waiters()
    # upstream's `gc.collect(); torch.cuda.empty_cache()` (core/pipeline.py:904-907) exists to give the model's memory back: the collection runs where a
    # model was torn down (this run built it; RomaMatcher.close collects too), the run's own buffers - no reference cycles - go back to the driver either way
    if own_matcher is not None:
        gc.collect()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()
    return failed
